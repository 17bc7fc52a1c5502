"""GPU recall of the table attack: k_table_count and k_prep_table through the scan API (set_table / load_table) and
dwpa_crack_table through its command line.

The all-plants method of tests/test_gpu_recall.py / tests/test_gpu_markov.py: EVERY candidate of every loaded window is
the PSK of one line per ESSID, the expected set comes from the CPU oracle, and the hits must equal it -- none missing,
none extra, none twice, ids and PMKs equal.  The candidates come from the reference of tests/table_plan.py
(itertools.product order over a prefix sum in plain ints), which tests/test_table_plan.py checks on the CPU; the
fixtures are its plans.  No two loads of one scan start at the same index, so no slot ever holds a candidate it held
before and a stale PMK cannot stand in for one the kernel skipped.  Batch sizes follow from the device's CU count, and
every scan test asserts which PBKDF2 kernel ran.
"""
import os
import random
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

import dwpa_amd  # noqa: E402
from dwpa_amd import _lib as L  # noqa: E402
from dwpa_amd.device import Dictionary  # noqa: E402
from tests import table_plan as T  # noqa: E402
from tests import test_gpu_recall as R  # noqa: E402
from tests.test_gpu_recall import sizes  # noqa: E402,F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC = R.NC
ONE = (b"table-recall",)


def plant(plan, windows, essids, seed):
    """One line per (essid, candidate) for the candidates of `windows` [(first, count)].  Returns (lines, expected hits
    {(line, cand, nc, endian, pmk)}, the PSK of each line)."""
    ids = [i for first, count in windows for i in range(first, first + count)]
    assert ids and max(ids) < plan.k and len(set(ids)) == len(ids)
    psks = [plan.candidate(i) for i in ids]
    assert len({p.rstrip(b"\0") for p in psks}) == len(psks), "a PSK twice, or two PSKs that are one HMAC key"
    lines, owner, pmks, found = R._plant_lines(psks, essids, random.Random(seed))
    exp = {(ln, ids[i], nc, en, pmk) for ln, ((e, i), (nc, en), pmk) in enumerate(zip(owner, found, pmks))}
    return lines, exp, [psks[i] for e, i in owner]


class Held:
    """The (slot, id) pairs a scan has loaded: a load that repeats one could be answered by a stale PMK."""

    def __init__(self):
        self.seen = set()

    def load(self, sc, first, count):
        assert first not in self.seen, "a slot would hold a candidate it held before"
        self.seen.add(first)
        sc.load_table(first, count)
        assert sc.loaded() == count


def set_table(sc, dev, plan):
    got = sc.set_table(dev.off.ptr, dev.data.ptr, len(plan.words), plan.table, plan.minlen, plan.maxlen, plan.word_max)
    assert got == (plan.k, plan.kept()), "keyspace and kept words from the count kernel against the reference"
    return got


def _windows(sc, held, exp, windows, mode, what):
    for first, count in windows:
        held.load(sc, first, count)
        R._scan_all(sc, mode)
        R._assert_same(R._hitset(sc.hits(cap=4096)), {p for p in exp if first <= p[1] < first + count},
                       (what, mode, first, count))


def recall(plan, lines, exp, windows, batch, mode, kernel, what):
    """set_table once, then every window: loaded() == count and the hits are exactly the window's plants."""
    dev = Dictionary.from_words(plan.words)
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(lines, nc=NC, batch=batch)
    try:
        set_table(sc, dev, plan)
        _windows(sc, Held(), exp, windows, mode, what)
    finally:
        sc.close()
    assert L.pbkdf2_kernels() == {kernel}


def _one(plan, name, windows, sizes, seed):
    lines, exp, _ = plant(plan, T.PLANTED[name], ONE, seed)
    recall(plan, lines, exp, windows, sizes["one"]["p"], "per_group", R.expected_kernel("one", "p"), name)


# ---------------------------------------------------------------------------------------------------------------
# the index: where a lane finds its word
# ---------------------------------------------------------------------------------------------------------------
def test_sixty_four_words_per_wave(sizes):
    """200 words of one candidate each: every lane of a wave has a word of its own, the last wave is partial, and
    windows start in the middle of a wave's words."""
    _one(T.PLAN_ONES, "ones", [(0, 200), (1, 64), (37, 130), (63, 2), (150, 50), (199, 1)], sizes, 0x71)


def test_one_word_over_waves_and_blocks(sizes):
    """One word of 3 * 5 * 7 * 11 = 1155 candidates: five blocks that all find the same word, radices that are no
    powers of two."""
    _one(T.PLAN_WIDE, "wide", [(0, 1155), (100, 300), (1154, 1), (640, 515)], sizes, 0x72)


def test_loads_that_begin_and_end_inside_a_word(sizes):
    """That word between 70 + 70 words of one candidate: a wave's first id lies in one word and its last in another,
    and `first` / `first + count` fall inside the wide word."""
    _one(T.PLAN_MIXED, "mixed", [(0, 100), (60, 200), (500, 300), (1000, 295), (69, 2), (1224, 2), (7, 1288)],
         sizes, 0x73)


def test_dropped_words_own_no_indices(sizes):
    """The first, the last and every second word dropped, by every reason of the plan (0, 7, 64 and 70 bytes; word_max
    + 1; 2^32; 2^64; 16^63): the count kernel's keyspace and kept count equal the reference's, and every index maps to
    a kept word's candidate.  Then the same list under word_max = 0: 2^32 and above stay dropped, 15 * 16^7 is kept."""
    plan = T.PLAN_DROPS
    lines, exp, _ = plant(plan, [(0, plan.k)], ONE, 0x74)
    dev = Dictionary.from_words(T.PLAN_DROPS_WIDE.words)  # the drops' list and one more word, which only `wide` names
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(lines, nc=NC, batch=sizes["one"]["p"])
    try:
        set_table(sc, dev, plan)
        _windows(sc, Held(), exp, [(0, plan.k), (1, 14), (15, 41)], "per_group", "drops")
        wide = T.PLAN_DROPS_WIDE
        assert set_table(sc, dev, wide) == (56 + 15 + 64 + 15 * 16**7, 11)
        sc.load_table(wide.k - 64, 64)
        assert sc.loaded() == 64
    finally:
        sc.close()
    assert L.pbkdf2_kernels() == {R.expected_kernel("one", "p")}


def test_window_clipped_at_the_end_of_the_index(sizes):
    """nkept = 1 (a list of three words, one kept, three candidates) and nkept = 65: the per-lane search stops at the
    last index entry."""
    _one(T.PLAN_ONE_KEPT, "one_kept", [(0, 3), (1, 2), (2, 1)], sizes, 0x75)
    _one(T.PLAN_65, "65", [(0, 65), (1, 64), (64, 1), (2, 63)], sizes, 0x76)


def test_bytes_counts_lengths_and_offsets(sizes):
    """Keys and values 0x00, 0x80 and 0xff, a key without identity, 1, 2, 3 and 16 alternatives, words of 8 and of 63
    bytes, words at odd byte offsets."""
    plan = T.PLAN_BYTES
    _one(plan, "bytes", [(0, plan.k), (190, 10), (197, 19)], sizes, 0x77)


def test_keyspace_above_2_32(sizes):
    """Three words of 2^31 candidates: 128 ids across each word boundary -- at 2^31, at 2^32 and up to K = 3 * 2^31."""
    plan = T.PLAN_BIG
    lines, exp, _ = plant(plan, T.BIG_WINDOWS, ONE, 0x78)
    recall(plan, lines, exp, T.BIG_WINDOWS, sizes["one"]["p"], "per_group", R.expected_kernel("one", "p"), "big")


# ---------------------------------------------------------------------------------------------------------------
# state
# ---------------------------------------------------------------------------------------------------------------
def test_set_table_twice_and_beside_a_mask(sizes):
    """On one scan: a table, another table over another list, then set_mask, load_table, load_mask -- the table and the
    mask do not disturb each other."""
    a, b = T.PLAN_65, T.PLAN_ONE_KEPT
    mask = b"mask-?d?d?d"
    pa = [a.candidate(i) for i in range(a.k)]
    pb = [b.candidate(i) for i in range(b.k)]
    pm = [b"mask-%03d" % i for i in range(100, 164)]
    psks = pa + pb + pm
    lines, owner, pmks, found = R._plant_lines(psks, ONE, random.Random(0x79))
    line_of = {psks[i]: ln for ln, (e, i) in enumerate(owner)}

    def expect(cands):
        return {(line_of[p], i, found[line_of[p]][0], found[line_of[p]][1], pmks[line_of[p]]) for i, p in cands}

    da, db = Dictionary.from_words(a.words), Dictionary.from_words(b.words)
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(lines, nc=NC, batch=sizes["one"]["p"])
    try:
        set_table(sc, da, a)
        sc.load_table(0, a.k)
        R._scan_all(sc, "per_group")
        R._assert_same(R._hitset(sc.hits(cap=4096)), expect(enumerate(pa)), "first table")
        set_table(sc, db, b)
        sc.load_table(0, b.k)
        assert sc.loaded() == b.k
        R._scan_all(sc, "per_group")
        R._assert_same(R._hitset(sc.hits(cap=4096)), expect(enumerate(pb)), "second table")
        with pytest.raises(L.DwpaError):  # the first table's keyspace is gone
            sc.load_table(0, a.k)
        set_table(sc, da, a)
        assert sc.set_mask(mask) == 1000
        sc.load_table(1, a.k - 1)
        assert sc.loaded() == a.k - 1
        R._scan_all(sc, "per_group")
        R._assert_same(R._hitset(sc.hits(cap=4096)), expect(list(enumerate(pa))[1:]), "table after set_mask")
        sc.load_mask(100, 64)
        R._scan_all(sc, "per_group")
        R._assert_same(R._hitset(sc.hits(cap=4096)), expect(zip(range(100, 164), pm)), "mask after load_table")
        sc.load_table(2, 40)
        R._scan_all(sc, "per_group")
        R._assert_same(R._hitset(sc.hits(cap=4096)), expect(list(enumerate(pa))[2:42]), "table after load_mask")
    finally:
        sc.close()
    assert L.pbkdf2_kernels() == {R.expected_kernel("one", "p")}


def test_run_over_three_essids(sizes):
    """run(): one multi-group launch over the three ESSIDs of test_gpu_recall, one of them 52 bytes long."""
    plan = T.PLAN_RUN
    lines, exp, _ = plant(plan, [(0, plan.k)], R.ESSIDS, 0x7a)
    assert len(lines) == 3 * 165
    recall(plan, lines, exp, [(0, plan.k), (20, 100), (134, 31)], sizes["mg"]["p"], "run", R.expected_kernel("mg", "p"),
           "run")


def test_refusals_on_a_live_scan(sizes):
    """A load before any table, first + count > K (also when the sum wraps), count above the batch, and a bad table or
    a bad call, which leave the table that was set in force."""
    plan = T.PLAN_ONE_KEPT
    lines, exp, _ = plant(plan, [(0, plan.k)], ONE, 0x7b)
    dev = Dictionary.from_words(plan.words)
    sc = dwpa_amd.Scan(lines, nc=NC, batch=sizes["one"]["p"])

    def refused(fn, *a, **kw):
        with pytest.raises(L.DwpaError) as e:
            fn(*a, **kw)
        assert e.value.code == L.DWPA_E_ARG, a

    try:
        refused(sc.load_table, 0, 1)
        refused(sc.load_table, 0, 0)
        set_table(sc, dev, plan)
        for first, count in ((0, plan.k + 1), (plan.k, 1), (plan.k + 1, 0), (2**64 - 1, 2), (1, plan.k),
                             (0, sizes["one"]["p"] + 64)):
            refused(sc.load_table, first, count)
        sc.load_table(plan.k, 0)
        assert sc.loaded() == 0
        refused(sc.set_table, dev.off.ptr, dev.data.ptr, len(plan.words), b"a=b\nnot a mapping\n")
        refused(sc.set_table, dev.off.ptr, dev.data.ptr, len(plan.words), b"")
        refused(sc.set_table, dev.off.ptr, dev.data.ptr, 2**32, plan.table)
        refused(sc.set_table, 0, 0, len(plan.words), plan.table)
        _windows(sc, Held(), exp, [(0, plan.k)], "per_group", "after the refusals")
    finally:
        sc.close()


# ---------------------------------------------------------------------------------------------------------------
# dwpa_crack_table through the command line
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cfiles(tmp_path_factory):
    """The mixed plan as files, and one hash file whose only line's PSK is a candidate of the last batch of 512."""
    d = tmp_path_factory.mktemp("gpu_table")
    plan = T.PLAN_MIXED
    target = plan.k - 40
    psk = plan.candidate(target)
    lines, owner, pmks, found = R._plant_lines([psk], ONE, random.Random(0x7c))
    (d / "h.hash").write_bytes(b"\n".join(lines) + b"\n")
    (d / "list").write_bytes(b"".join(w + b"\n" for w in plan.words))
    (d / "t.table").write_bytes(plan.table)
    (d / "bad.table").write_bytes(b"a=b\nnot a mapping\n")
    return {"dir": d, "plan": plan, "target": target, "record": R._records(lines, [psk])[0], "hash": str(d / "h.hash"),
            "list": str(d / "list"), "table": str(d / "t.table")}


def _table_cli(cf, out, *extra, table=None, hash_file=None):
    argv = [sys.executable, "-m", "dwpa_amd.table", hash_file or cf["hash"], cf["list"], "--table-file",
            table or cf["table"], "--batch", "512", "--nonce-error-corrections", str(NC), "-o", str(out), *extra]
    r = subprocess.run(argv, cwd=ROOT, capture_output=True, timeout=120)
    recs = out.read_bytes().split(b"\n") if out.exists() else [b""]
    assert recs.pop() == b""
    return r, recs


def test_crack_plant_in_the_last_batch(cfiles, tmp_path):
    """1295 candidates in batches of 512: three loads, the plant in the last one.  rc 0, the outfile record, nothing on
    stdout, the drop counts on stderr."""
    assert cfiles["target"] // 512 == (cfiles["plan"].k - 1) // 512 == 2
    r, recs = _table_cli(cfiles, tmp_path / "o.key")
    assert r.returncode == 0 and r.stdout == b"", r.stderr[-2000:]
    assert recs == [cfiles["record"]]
    assert b"141 of 141 words kept, 0 dropped for length, 0 for more than" in r.stderr
    assert b"1 hashlines cracked, 141 words" in r.stderr


def test_crack_windows_and_errors(cfiles, tmp_path):
    """-s / -l windows that exclude and include the plant: rc 1 with an empty outfile, rc 0 with the record; a bad
    table, a missing list and a skip at K: 255 and no outfile."""
    t = cfiles["target"]
    r, recs = _table_cli(cfiles, tmp_path / "a.key", "-s", "0", "-l", str(t))
    assert r.returncode == 1 and recs == [], r.stderr[-2000:]
    assert b"%d candidates" % t in r.stderr
    r, recs = _table_cli(cfiles, tmp_path / "b.key", "-s", str(t), "-l", "1")
    assert r.returncode == 0 and recs == [cfiles["record"]], r.stderr[-2000:]
    for extra, kw in ((("-s", str(cfiles["plan"].k)), {}), ((), {"table": str(cfiles["dir"] / "bad.table")}),
                      ((), {"hash_file": str(cfiles["dir"] / "missing.hash")})):
        out = tmp_path / "c.key"
        r, recs = _table_cli(cfiles, out, *extra, **kw)
        assert r.returncode == 255 and r.stdout == b"" and not out.exists(), (extra, kw, r.stderr[-2000:])
