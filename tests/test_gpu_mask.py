"""GPU recall of the mask attack: k_prep_mask through the scan API (set_mask / load_mask) and dwpa_crack_mask.

The all-plants method of tests/test_gpu_recall.py: EVERY loaded candidate is the PSK of one line per ESSID (kinds cycle
through PMKID and keyver 1/2/3 with planted nonce offsets), the expected set comes from the CPU oracle, and the hits
must equal it -- none missing, none extra, none twice, PMKs equal.  The candidates themselves come from the reference
expander of tests/test_mask.py (the built-in table and itertools.product order), not from the library.  Batch sizes
follow from the device's CU count as in that file, and every scan test asserts which PBKDF2 kernel ran.
"""
import json
import os
import random
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

import dwpa_amd  # noqa: E402
from dwpa_amd import _lib as L  # noqa: E402
from dwpa_amd import m22000 as M  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import test_gpu_recall as R  # noqa: E402
from tests.test_gpu_recall import sizes  # noqa: E402,F401  (the fixture)
from tests.test_mask import RAW, ref_candidate, ref_sets  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC = R.NC
ONE = (b"mask-recall",)
A_MASK, A_CUSTOM = b"pre??x?1?2?l", (b"ab", b"?dXY")  # K = 2 * 12 * 26 = 624; 8 positions: pre?x and three sets
A_WINDOWS = [(0, 1), (0, 63), (0, 64), (0, 65), (0, 256), (0, 257), (37, 130), (624 - 100, 100)]


def plant(mask, custom, ranges, essids, seed):
    """One line per (essid, candidate) for the candidates of `ranges` [(first, count)] of the mask.  Returns (lines,
    expected hits {(line, cand, nc, endian, pmk)}, the PSK of each line)."""
    sets, k = ref_sets(mask, custom)
    ids = [i for first, count in ranges for i in range(first, first + count)]
    assert ids and max(ids) < k and len(set(ids)) == len(ids)
    psks = [ref_candidate(sets, i) for i in ids]
    assert len(set(psks)) == len(psks), "a PSK twice"
    assert len({p.rstrip(b"\0") for p in psks}) == len(psks), "two PSKs that are one HMAC key"
    lines, owner, pmks, found = R._plant_lines(psks, essids, random.Random(seed))
    exp = {(ln, ids[i], nc, en, pmk) for ln, ((e, i), (nc, en), pmk) in enumerate(zip(owner, found, pmks))}
    return lines, exp, [psks[i] for e, i in owner]


def recall(lines, exp, mask, custom, windows, batch, mode, kernel):
    """set_mask once, then every window: loaded() == count and the hits are exactly the window's plants."""
    k = ref_sets(mask, custom)[1]
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(lines, nc=NC, batch=batch)
    try:
        assert sc.set_mask(mask, custom) == k
        for first, count in windows:
            sc.load_mask(first, count)
            assert sc.loaded() == count
            R._scan_all(sc, mode)
            R._assert_same(R._hitset(sc.hits(cap=4096)), {p for p in exp if first <= p[1] < first + count},
                           (mask, mode, first, count))
    finally:
        sc.close()
    assert L.pbkdf2_kernels() == {kernel}


@pytest.fixture(scope="module")
def fa():
    """a / f / g: every candidate of A_MASK planted under the three ESSIDs of test_gpu_recall (one of 52 bytes)."""
    lines, exp, psks = plant(A_MASK, A_CUSTOM, [(0, 624)], R.ESSIDS, 0xa)
    assert len(lines) == 3 * 624 and [p[1] for p in sorted(exp)][:624] == list(range(624))
    return {"lines": lines, "exp": exp, "psk": psks}


# ---------------------------------------------------------------------------------------------------------------
# a-e: the scan API
# ---------------------------------------------------------------------------------------------------------------
def test_lanes_and_waves_per_group(fa, sizes):
    """a. 1, 63, 64, 65, 256, 257 candidates from index 0, 130 from 37 and the last 100, pbkdf2(g) / verify(g) on one
    ESSID."""
    lines, exp = fa["lines"][:624], {p for p in fa["exp"] if p[0] < 624}
    recall(lines, exp, A_MASK, A_CUSTOM, A_WINDOWS, sizes["one"]["p"], "per_group", R.expected_kernel("one", "p"))


def test_lanes_and_waves_run(fa, sizes):
    """a. The same windows through run() over three ESSIDs, one of them 52 bytes long."""
    recall(fa["lines"], fa["exp"], A_MASK, A_CUSTOM, A_WINDOWS, sizes["mg"]["p"], "run", R.expected_kernel("mg", "p"))


def test_equal_to_the_numeric_path(sizes):
    """b. ?d x 8 at 99,999,900..99,999,999: the hits of load_mask and of load_numeric over the same lines are
    identical, ids included (and both are the planted set)."""
    first, count = 99_999_900, 100
    lines, exp, psks = plant(b"?d" * 8, (), [(first, count)], ONE, 0xb)
    assert psks == [b"%08d" % v for v in range(first, first + count)]
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(lines, nc=NC, batch=sizes["one"]["p"])
    try:
        assert sc.set_mask(b"?d" * 8) == 10**8
        sc.load_mask(first, count)
        assert sc.loaded() == count
        R._scan_all(sc, "per_group")
        by_mask = R._hitset(sc.hits(cap=4096))
        sc.load_numeric(first, count, 8)
        assert sc.loaded() == count
        R._scan_all(sc, "per_group")
        by_numeric = R._hitset(sc.hits(cap=4096))
    finally:
        sc.close()
    R._assert_same(by_mask, exp, "mask")
    assert by_mask == by_numeric
    assert L.pbkdf2_kernels() == {R.expected_kernel("one", "p")}


WRAP_MASK = b"?d?dA?dB?d?dC?dD?1?2?3?4"  # literals at byte lanes 2, 0, 3, 1 of their words; radices 2, 3, 5, 7 last
WRAP_CUSTOM = (b"ab", b"cde", b"fghij", b"klmnopq")
CARRIES = [(b"?a" * 8, (), [(2**32 - 50, 100), (95**8 - 100, 100)]),  # across index 2^32, and the top of the keyspace
           (b"?b?b?b?b?b?b?b?a", (), [(95 * 2**56 - 100, 100)]),     # the top of a keyspace just under 2^64
           (WRAP_MASK, WRAP_CUSTOM, [(210 * 100 - 65, 130)])]        # the four small radices wrap together


@pytest.mark.parametrize("case", range(len(CARRIES)))
def test_carries_and_wide_indices(sizes, case):
    """c. Windows that cross index 2^32, end at K - 1 for K up to 95 * 2^56, and carry through four positions of
    radices 2, 3, 5, 7 at once (on into ?d positions that literals separate: index 21,000 = 100 * 210)."""
    mask, custom, windows = CARRIES[case]
    if mask == WRAP_MASK:
        sets, k = ref_sets(mask, custom)
        assert [len(s) for s in sets[-4:]] == [2, 3, 5, 7] and k == 10**6 * 210
        assert {p % 4 for p, s in enumerate(sets) if len(s) == 1} == {0, 1, 2, 3}
    lines, exp, _ = plant(mask, custom, windows, ONE, 0xc0 + case)
    recall(lines, exp, mask, custom, windows, sizes["one"]["p"], "per_group", R.expected_kernel("one", "p"))


LONG = b"?h?H" + b"l" * 29 + b"?s?u" + b"r" * 28 + b"?d?l"
LENGTHS = [(b"?u?l" + b"x" * (n - 4) + b"?d?d", [(26 * 26 * 100 - 66, 66)]) for n in (8, 9, 10, 11)] + \
          [(LONG, [(0, 65), (16 * 16 * 33 * 26 * 10 * 26 - 65, 65)]), (b"?d", [(0, 10)])]


@pytest.mark.parametrize("case", range(len(LENGTHS)))
def test_lengths(sizes, case):
    """d. 8, 9, 10 and 11 positions (each tail of the last key word), 63 positions (57 literals, ?h ?H ?s ?u ?d ?l
    at the first, middle and last positions) and 1 position."""
    mask, windows = LENGTHS[case]
    sets, k = ref_sets(mask)
    if mask == LONG:
        assert len(sets) == 63 and sum(len(s) == 1 for s in sets) == 57
        assert [len(sets[p]) for p in (0, 1, 31, 32, 61, 62)] == [16, 16, 33, 26, 10, 26]
    assert windows[-1][0] + windows[-1][1] == k
    lines, exp, _ = plant(mask, (), windows, ONE, 0xd0 + case)
    recall(lines, exp, mask, (), windows, sizes["one"]["p"], "per_group", R.expected_kernel("one", "p"))


def test_bytes(sizes):
    """e. A custom set of the raw bytes 0x00 0x0a 0x7f 0x80 0xff 'a' (sign extension, NUL handling): passw?1?1?1,
    all 216 loaded.  36 candidates end in a NUL byte; as HMAC keys (zero-padded) they still equal nothing else here,
    which plant() asserts."""
    mask, custom = b"passw?1?1?1", (RAW,)
    lines, exp, psks = plant(mask, custom, [(0, 216)], ONE, 0xe)
    assert b"passw\0\0\0" in psks and b"passw\xff\x80\x7f" in psks
    recall(lines, exp, mask, custom, [(0, 216)], sizes["one"]["p"], "per_group", R.expected_kernel("one", "p"))


# ---------------------------------------------------------------------------------------------------------------
# f: argument errors on a live scan
# ---------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_scan_usable(fa, sizes):
    lines, exp = fa["lines"][:624], {p for p in fa["exp"] if p[0] < 624}
    batch = sizes["one"]["p"]
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(lines, nc=NC, batch=batch)

    def refused(first, count):
        with pytest.raises(L.DwpaError) as e:
            sc.load_mask(first, count)
        assert e.value.code == L.DWPA_E_ARG

    try:
        refused(0, 1)  # no mask set
        assert sc.set_mask(b"?d" * 8) == 10**8
        refused(0, sc.batch + 1)
        refused(10**8 - 1, 2)
        refused(10**8, 1)
        refused(2**64 - 1, 2)
        sc.load_mask(10**8 - 64, 64)  # a valid load of another mask: none of its candidates is a PSK here
        assert sc.loaded() == 64
        R._scan_all(sc, "per_group")
        assert sc.hits(cap=4096) == []
        assert sc.set_mask(A_MASK, A_CUSTOM) == 624  # replaces the first
        refused(624 - 1, 2)
        refused(2**64 - 1, 2)
        sc.load_mask(37, 130)
        assert sc.loaded() == 130
        R._scan_all(sc, "per_group")
        R._assert_same(R._hitset(sc.hits(cap=4096)), {p for p in exp if 37 <= p[1] < 167}, "after the errors")
        for bad in (b"?x", b"?d?", b"?3"):
            with pytest.raises(L.DwpaError) as e:
                sc.set_mask(bad)
            assert e.value.code == L.DWPA_E_ARG
    finally:
        sc.close()
    assert L.pbkdf2_kernels() == {R.expected_kernel("one", "p")}


# ---------------------------------------------------------------------------------------------------------------
# g: dwpa_crack_mask
# ---------------------------------------------------------------------------------------------------------------
def _crack(tmp_path, lines, mask, custom, **kw):
    hf, out = tmp_path / "h.hash", tmp_path / "o.key"
    hf.write_bytes(b"\n".join(lines) + b"\n")
    L.pbkdf2_kernels(reset=True)
    rc = dwpa_amd.crack_mask(str(hf), mask, custom, nonce_error_corrections=NC, out_file=str(out), batch=512, **kw)
    ran = L.pbkdf2_kernels()
    recs = out.read_bytes().split(b"\n") if out.exists() else [b""]
    assert recs.pop() == b""
    return rc, sorted(recs), ran


def test_crack_mask_cracks_every_line(fa, tmp_path):
    """g1. The all-plants hash file of A_MASK (three ESSIDs): rc 0, every line once with its PSK, words 0."""
    rc, recs, ran = _crack(tmp_path, fa["lines"], A_MASK, A_CUSTOM)
    assert rc == 0 and recs == sorted(R._records(fa["lines"], fa["psk"]))
    assert ran and ran <= R.MG_KERNELS, ran
    st = M.crack_stats()
    assert (st["words"], st["candidates"], st["hashes"], st["cracked"]) == (0, 624, 3 * 624, 3 * 624)
    ws = M.crack_worker_stats()
    assert len(ws) == 1 and ws[0]["candidates"] == 624 and ws[0]["items"] == 2 and ws[0]["words"] == 0


def test_crack_mask_exhausted(fa, tmp_path):
    """g2. One PSK outside the mask: rc 1, the other records present.  g3. A skip / limit window: rc 1 and exactly
    the lines whose PSK's index is inside it.  g4. skip >= K: rc -1, as is increment with skip."""
    rng = random.Random(0x62)
    lines, psks = fa["lines"][:624], fa["psk"][:624]
    outside = b"pre?xcXa"  # 'c' is not in ?1
    assert outside not in psks
    extra = R._line(0, 0, "LE", outside, R.ESSIDS[0], O.c_pbkdf2(outside, R.ESSIDS[0]), rng)
    rc, recs, _ = _crack(tmp_path, lines + [extra], A_MASK, A_CUSTOM)
    assert rc == 1 and recs == sorted(R._records(lines, psks))
    (tmp_path / "o.key").unlink()
    rc, recs, _ = _crack(tmp_path, lines, A_MASK, A_CUSTOM, skip=100, limit=300)
    inside = [k for k in range(624) if 100 <= k < 400]  # line k of the first ESSID holds candidate k
    assert rc == 1 and recs == sorted(R._records([lines[k] for k in inside], [psks[k] for k in inside]))
    assert M.crack_stats()["candidates"] == 300
    (tmp_path / "o.key").unlink()
    assert _crack(tmp_path, lines, A_MASK, A_CUSTOM, skip=624) == (-1, [], frozenset())
    assert _crack(tmp_path, lines, A_MASK, A_CUSTOM, skip=1, increment=(8, 9))[0] == -1
    assert _crack(tmp_path, lines, b"?d?d?d?d?d?d?d", ())[0] == -1  # 7 positions: skipped, nothing left to run


INC_MASK, INC_CUSTOM = b"?1" * 10, (b"01",)


@pytest.fixture(scope="module")
def finc():
    """Every candidate of the increment 8..10 run of INC_MASK (256 + 512 + 1024) is the PSK of one line."""
    lines, psks = [], []
    for n in (8, 9, 10):
        ln, _, ps = plant(b"?1" * n, INC_CUSTOM, [(0, 2**n)], ONE, 0x60 + n)
        lines += ln
        psks += ps
    assert len(lines) == 1792 and {len(p) for p in psks} == {8, 9, 10}
    return {"lines": lines, "psk": psks}


def test_crack_mask_increment(finc, tmp_path):
    """g5. Increment 8..10 over -1 01 ?1 x 10: the prefixes of 8, 9 and 10 positions, shortest first: rc 0."""
    rc, recs, ran = _crack(tmp_path, finc["lines"], INC_MASK, INC_CUSTOM, increment=(8, 10))
    assert rc == 0 and recs == sorted(R._records(finc["lines"], finc["psk"]))
    assert ran and ran <= R.MG_KERNELS, ran
    st = M.crack_stats()
    assert (st["words"], st["candidates"]) == (0, 1792)
    assert M.crack_worker_stats()[0]["items"] == 1 + 1 + 2  # batches of 512 never span two lengths
    (tmp_path / "o.key").unlink()
    rc, recs, _ = _crack(tmp_path, finc["lines"], INC_MASK, INC_CUSTOM, increment=(1, 9))  # 1..7 are skipped
    short = [k for k, p in enumerate(finc["psk"]) if len(p) <= 9]
    assert rc == 1 and recs == sorted(R._records([finc["lines"][k] for k in short], [finc["psk"][k] for k in short]))


_SHARDS_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import dwpa_amd
from dwpa_amd import m22000 as M
rc = dwpa_amd.crack_mask(sys.argv[2], "?1" * 10, (b"01",), increment=(8, 10), nonce_error_corrections=int(sys.argv[4]),
                         out_file=sys.argv[3], batch=512)
print(json.dumps({"rc": rc, "stats": M.crack_stats(), "workers": M.crack_worker_stats()}))
"""


def test_crack_mask_two_workers(finc, tmp_path):
    """g6. The same increment run with DWPA_CRACK_SHARDS_PER_DEVICE=2 (read per call; a child keeps this process's
    environment as it is): two workers share the cursor, every line is cracked exactly once, and the workers'
    candidates sum to the derived total."""
    hf, out = tmp_path / "h.hash", tmp_path / "o.key"
    hf.write_bytes(b"\n".join(finc["lines"]) + b"\n")
    env = dict(os.environ, DWPA_CRACK_SHARDS_PER_DEVICE="2")
    r = subprocess.run([sys.executable, "-c", _SHARDS_CHILD, ROOT, str(hf), str(out), str(NC)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["rc"] == 0
    recs = out.read_bytes().split(b"\n")
    assert recs.pop() == b"" and sorted(recs) == sorted(R._records(finc["lines"], finc["psk"]))
    assert len(res["workers"]) == 2 and len({w["device"] for w in res["workers"]}) == 1
    assert sum(w["candidates"] for w in res["workers"]) == res["stats"]["candidates"] == 1792
    assert res["stats"]["words"] == 0 and res["stats"]["cracked"] == 1792
