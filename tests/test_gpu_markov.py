"""GPU recall of the Markov-ordered mask attack: k_prep_markov through the scan API (set_mask(markov=, threshold=) /
load_mask) and dwpa_crack_mask_markov.

The all-plants method of tests/test_gpu_recall.py / tests/test_gpu_mask.py: EVERY candidate of every window is the PSK
of one line per ESSID, the expected set comes from the CPU oracle, and the hits must equal it -- none missing, none
extra, none twice, ids and PMKs equal.  The candidates come from the Python reference of tests/test_markov.py (train
-> counts -> ranking -> candidate), not from the library.  Batch sizes follow from the device's CU count, and every
scan test asserts which PBKDF2 kernel ran.  Byte 0x00 stays out of the last position (two PSKs that are one HMAC key).
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
from tests import test_gpu_recall as R  # noqa: E402
from tests.test_gpu_recall import sizes  # noqa: E402,F401  (the fixture)
from tests.test_mask import RAW, ref_candidate, ref_sets  # noqa: E402
from tests.test_markov import IDENTITY, mk_sets, plain, ref_counts, ref_keyspace, ref_markov, ref_order  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC = R.NC
ONE = (b"markov-recall",)
ALPHA = b"abcdefXY0123456789lmnopqrPASW" + RAW[:5]


def _words(seed, n=4000):
    """Words of 8..14 bytes over a small alphabet with the raw bytes in it: every (position, predecessor) row of the
    positions the masks below use is seen, with a ranking of its own; plus 40 words of 63 bytes."""
    rng = random.Random(seed)
    words = [bytes(rng.choice(ALPHA) for _ in range(rng.randint(8, 14))) for _ in range(n)]
    return words + [bytes(rng.choice(b"hHlr5 zQ") for _ in range(63)) for _ in range(40)]


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """Two models: {"n": reference counts, "img": image, "path": file}."""
    d = tmp_path_factory.mktemp("gpu_markov")
    out = []
    for k, seed in enumerate((0x6d31, 0x6d32)):
        words = _words(seed)
        (d / f"w{k}").write_bytes(b"".join(plain(w) + b"\n" for w in words))
        assert M.markov_train([str(d / f"w{k}")], str(d / f"m{k}.dwmk")) == len(words)
        out.append({"n": ref_counts(words), "img": M.markov_load(str(d / f"m{k}.dwmk")), "path": str(d / f"m{k}.dwmk")})
    assert out[0]["img"] != out[1]["img"]
    return out


def plant(model, mask, custom, t, ranges, essids, seed):
    """One line per (essid, candidate) for the candidates of `ranges` [(first, count)] of the mask in Markov order
    under threshold t.  Returns (lines, expected hits {(line, cand, nc, endian, pmk)}, the PSK of each line)."""
    sets = mk_sets(mask, custom)
    k = ref_keyspace(sets, t)
    ids = [i for first, count in ranges for i in range(first, first + count)]
    assert ids and max(ids) < k and len(set(ids)) == len(ids)
    psks = [ref_markov(model["n"], sets, t, i) for i in ids]
    assert len(set(psks)) == len(psks), "a PSK twice"
    assert len({p.rstrip(b"\0") for p in psks}) == len(psks), "two PSKs that are one HMAC key"
    lines, owner, pmks, found = R._plant_lines(psks, essids, random.Random(seed))
    exp = {(ln, ids[i], nc, en, pmk) for ln, ((e, i), (nc, en), pmk) in enumerate(zip(owner, found, pmks))}
    return lines, exp, [psks[i] for e, i in owner]


def _windows(sc, exp, windows, mode, what):
    for first, count in windows:
        sc.load_mask(first, count)
        assert sc.loaded() == count
        R._scan_all(sc, mode)
        R._assert_same(R._hitset(sc.hits(cap=4096)), {p for p in exp if first <= p[1] < first + count},
                       (what, mode, first, count))


def recall(model, lines, exp, mask, custom, t, windows, batch, mode, kernel):
    """set_mask with the model once, then every window: loaded() == count and the hits are exactly the plants."""
    k = ref_keyspace(mk_sets(mask, custom), t)
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(lines, nc=NC, batch=batch)
    try:
        assert sc.set_mask(mask, custom, markov=model["img"], threshold=t) == k
        _windows(sc, exp, windows, mode, (mask, t))
    finally:
        sc.close()
    assert L.pbkdf2_kernels() == {kernel}


A_MASK, A_CUSTOM, A_T = b"pre??x?1?2?l", (b"abcdef", b"?dXY"), 10  # K = 6 * 10 * 10: the threshold cuts 12 and 26
A_K = 600
A_WINDOWS = [(0, 1), (0, 63), (0, 64), (0, 65), (0, 256), (0, 257), (37, 130), (A_K - 100, 100)]


@pytest.fixture(scope="module")
def fa(models):
    """a / f / g: every candidate of A_MASK under A_T planted under the three ESSIDs of test_gpu_recall."""
    assert [len(s) for s in mk_sets(A_MASK, A_CUSTOM)] == [1, 1, 1, 1, 1, 6, 12, 26]
    lines, exp, psks = plant(models[0], A_MASK, A_CUSTOM, A_T, [(0, A_K)], R.ESSIDS, 0xa)
    assert len(lines) == 3 * A_K
    return {"lines": lines, "exp": exp, "psk": psks}


# ---------------------------------------------------------------------------------------------------------------
# a-e: the scan API
# ---------------------------------------------------------------------------------------------------------------
def test_lanes_and_waves_per_group(models, fa, sizes):
    """a. 1, 63, 64, 65, 256, 257 candidates from index 0, 130 from 37 and the last 100, on one ESSID."""
    lines, exp = fa["lines"][:A_K], {p for p in fa["exp"] if p[0] < A_K}
    recall(models[0], lines, exp, A_MASK, A_CUSTOM, A_T, A_WINDOWS, sizes["one"]["p"], "per_group",
           R.expected_kernel("one", "p"))


def test_lanes_and_waves_run(models, fa, sizes):
    """a. The same windows through run() over three ESSIDs, one of them 52 bytes long."""
    recall(models[0], fa["lines"], fa["exp"], A_MASK, A_CUSTOM, A_T, A_WINDOWS, sizes["mg"]["p"], "run",
           R.expected_kernel("mg", "p"))


B_CASES = [(b"PASSW0?1?2?3", (b"abcdef", b"ab", b"?d"), 0),       # radix 2 before the last position
           (b"PASSW0?1?2?3", (b"abcdef", b"abc", b"?d"), 7),      # radix 3, the last position cut to 7
           (b"PASSW?1?2?3x", (b"XY", b"abc", b"lmnopq"), 4)]      # the same one position further up, before a literal


@pytest.mark.parametrize("case", range(len(B_CASES)))
def test_predecessors_differ_inside_a_wave(models, sizes, case):
    """b. Consecutive lanes read different rows: the last position's ranking differs per predecessor."""
    mask, custom, t = B_CASES[case]
    n, sets = models[0]["n"], mk_sets(mask, custom)
    p = len(sets) - (2 if case == 2 else 1)
    rows = {bytes(b for b in ref_order(n, p, a) if b in sets[p]) for a in sets[p - 1]}
    assert len(rows) == len(sets[p - 1]) and IDENTITY not in {ref_order(n, p, a) for a in sets[p - 1]}
    k = ref_keyspace(sets, t)
    lines, exp, _ = plant(models[0], mask, custom, t, [(0, k)], ONE, 0xb0 + case)
    recall(models[0], lines, exp, mask, custom, t, [(0, k)], sizes["one"]["p"], "per_group", R.expected_kernel("one", "p"))


def test_high_bytes(models, sizes):
    """c. Predecessor bytes 0x80 and 0xff, and byte 0x00 as a real predecessor at position 1 (position 0's
    pseudo-predecessor value, another row): ?1?1?1passw over the raw bytes, all 216."""
    mask, custom = b"?1?1?1passw", (RAW,)
    n = models[0]["n"]
    assert ref_order(n, 1, 0) != ref_order(n, 0, 0) and ref_order(n, 1, 0x80) != ref_order(n, 1, 0xff) != IDENTITY
    lines, exp, psks = plant(models[0], mask, custom, 0, [(0, 216)], ONE, 0xc)
    assert b"\0\0\0passw" in psks and b"\xff\x80\x7fpassw" in psks
    recall(models[0], lines, exp, mask, custom, 0, [(0, 216)], sizes["one"]["p"], "per_group", R.expected_kernel("one", "p"))
    lines, exp, _ = plant(models[0], mask, custom, 5, [(0, 125)], ONE, 0xc1)
    recall(models[0], lines, exp, mask, custom, 5, [(0, 125)], sizes["one"]["p"], "per_group", R.expected_kernel("one", "p"))


WRAP_MASK = b"?d?dA?dB?d?dC?dD?1?2?3?4"  # literals at byte lanes 2, 1, 0, 3; radices 2, 3, 5, 6 last under t = 6
WRAP_CUSTOM = (b"ab", b"cde", b"fghij", b"klmnopq")
CARRIES = [(b"?a" * 8, (), 0, [(2**32 - 50, 100)]),                        # across index 2^32
           (b"?b?b?b?b?b?b?b?a", (), 255, [(255**7 * 95 - 100, 100)]),     # the top of a keyspace just under 2^64
           (WRAP_MASK, WRAP_CUSTOM, 6, [(180 * 100 - 65, 130)])]           # the four small radices wrap together


@pytest.mark.parametrize("case", range(len(CARRIES)))
def test_carries_and_wide_indices(models, sizes, case):
    """d. A window across index 2^32, the top 100 of a thresholded keyspace just under 2^64, and a carry through four
    positions of radices 2, 3, 5, 6 at once, on into thresholded ?d positions that literals separate."""
    mask, custom, t, windows = CARRIES[case]
    sets = mk_sets(mask, custom)
    k = ref_keyspace(sets, t)
    if case == 1:
        assert 2**62 < k < 2**64 and windows[0][0] + windows[0][1] == k
    if case == 2:
        assert [min(len(s), t) for s in sets[-4:]] == [2, 3, 5, 6] and k == 6**6 * 180
    lines, exp, _ = plant(models[0], mask, custom, t, windows, ONE, 0xd0 + case)
    recall(models[0], lines, exp, mask, custom, t, windows, sizes["one"]["p"], "per_group", R.expected_kernel("one", "p"))


LONG = b"?h?H" + b"l" * 29 + b"?s?u" + b"r" * 28 + b"?d?l"
LENGTHS = [(b"?u?l" + b"x" * (n - 4) + b"?d?d", 9, [(9**4 - 66, 66)]) for n in (8, 9, 10, 11)] + \
          [(LONG, 3, [(0, 65), (3**6 - 65, 65)])]


@pytest.mark.parametrize("case", range(len(LENGTHS)))
def test_lengths(models, sizes, case):
    """e. 8, 9, 10 and 11 positions (each tail of the last key word) and 63 positions with 57 literals, its first and
    last 65 candidates."""
    mask, t, windows = LENGTHS[case]
    sets = mk_sets(mask)
    assert windows[-1][0] + windows[-1][1] == ref_keyspace(sets, t)
    lines, exp, _ = plant(models[1], mask, (), t, windows, ONE, 0xe0 + case)
    recall(models[1], lines, exp, mask, (), t, windows, sizes["one"]["p"], "per_group", R.expected_kernel("one", "p"))


# ---------------------------------------------------------------------------------------------------------------
# f: state
# ---------------------------------------------------------------------------------------------------------------
def test_state(models, sizes):
    """f. On one scan: plain, with a model, another threshold, another model, plain again, each with the right hits;
    t = 0 over the whole keyspace finds the plain mask's PSK set."""
    mask, custom = b"Q-?1?2?l?dzz", (b"ab", b"XYZ")
    sets, k = ref_sets(mask, custom)
    assert k == 2 * 3 * 26 * 10
    steps = [("plain", None, 0, [(100, 130)]), ("m0 t4", models[0], 4, [(0, 96)]), ("m0 t3", models[0], 3, [(0, 54)]),
             ("m1 t3", models[1], 3, [(0, 54)]), ("m1 t0", models[1], 0, [(0, 257), (k - 300, 300)]),
             ("plain again", None, 0, [(300, 130)])]
    psk_of = {}  # every PSK any step plants -> one line
    wanted = []
    for what, model, t, windows in steps:
        ids = [i for f, c in windows for i in range(f, f + c)]
        cands = [ref_candidate(sets, i) if model is None else ref_markov(model["n"], mk_sets(mask, custom), t, i) for i in ids]
        wanted.append(dict(zip(ids, cands)))
        psk_of.update((c, None) for c in cands)
    psks = sorted(psk_of)
    lines, owner, pmks, found = R._plant_lines(psks, ONE, random.Random(0xf))
    line_of = {psks[i]: ln for ln, (e, i) in enumerate(owner)}
    assert [ref_markov(models[0]["n"], mk_sets(mask, custom), 3, i) for i in range(54)] != \
           [ref_markov(models[1]["n"], mk_sets(mask, custom), 3, i) for i in range(54)], "the two models agree"
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(lines, nc=NC, batch=sizes["one"]["p"])
    try:
        for (what, model, t, windows), want in zip(steps, wanted):
            if model is None:
                assert sc.set_mask(mask, custom) == k
            else:
                assert sc.set_mask(mask, custom, markov=model["img"], threshold=t) == ref_keyspace(mk_sets(mask, custom), t)
            for first, count in windows:
                sc.load_mask(first, count)
                assert sc.loaded() == count
                R._scan_all(sc, "per_group")
                exp = set()
                for i in range(first, first + count):
                    ln = line_of[want[i]]
                    exp.add((ln, i, found[ln][0], found[ln][1], pmks[ln]))
                R._assert_same(R._hitset(sc.hits(cap=4096)), exp, (what, first, count))
            with pytest.raises(L.DwpaError) as e:  # a refused set call leaves the mask that was set
                sc.set_mask(mask, custom, markov=b"not a model", threshold=2)
            assert e.value.code == L.DWPA_E_ARG
    finally:
        sc.close()
    assert L.pbkdf2_kernels() == {R.expected_kernel("one", "p")}


def test_threshold_zero_is_the_plain_set(models, sizes):
    """f. t = 0 over a whole small keyspace: the PSKs found are the plain mask's, every one once."""
    mask, custom = b"?1?2?1?2pass", (b"abc", b"01")
    sets, k = ref_sets(mask, custom)
    psks = [ref_candidate(sets, i) for i in range(k)]
    lines, owner, pmks, found = R._plant_lines(psks, ONE, random.Random(0xf0))
    sc = dwpa_amd.Scan(lines, nc=NC, batch=sizes["one"]["p"])
    try:
        assert sc.set_mask(mask, custom, markov=models[0]["img"]) == k == 36
        sc.load_mask(0, k)
        R._scan_all(sc, "per_group")
        hits = sc.hits(cap=4096)
    finally:
        sc.close()
    assert sorted(h["line"] for h in hits) == list(range(k))
    mk = mk_sets(mask, custom)
    assert all(ref_markov(models[0]["n"], mk, 0, h["cand"]) == psks[h["line"]] for h in hits)


# ---------------------------------------------------------------------------------------------------------------
# g: dwpa_crack_mask_markov
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


def test_crack_whole_keyspace_and_window(models, fa, tmp_path):
    """g. The all-plants hash file of A_MASK (three ESSIDs): rc 0, every line once with its PSK; then a -s / -l
    window of the thresholded keyspace: rc 1 and exactly the lines whose PSK's index is inside it."""
    rc, recs, ran = _crack(tmp_path, fa["lines"], A_MASK, A_CUSTOM, markov=models[0]["path"], threshold=A_T)
    assert rc == 0 and recs == sorted(R._records(fa["lines"], fa["psk"]))
    assert ran and ran <= R.MG_KERNELS, ran
    st = M.crack_stats()
    assert (st["words"], st["candidates"], st["hashes"], st["cracked"]) == (0, A_K, 3 * A_K, 3 * A_K)
    (tmp_path / "o.key").unlink()
    lines, psks = fa["lines"][:A_K], fa["psk"][:A_K]
    rc, recs, _ = _crack(tmp_path, lines, A_MASK, A_CUSTOM, markov=models[0]["path"], threshold=A_T, skip=100, limit=300)
    inside = range(100, 400)  # line k of the first ESSID holds candidate k
    assert rc == 1 and recs == sorted(R._records([lines[k] for k in inside], [psks[k] for k in inside]))
    assert M.crack_stats()["candidates"] == 300
    (tmp_path / "o.key").unlink()
    assert _crack(tmp_path, lines, A_MASK, A_CUSTOM, markov=models[0]["path"], threshold=A_T, skip=A_K)[0] == -1


def test_crack_model_errors(models, fa, tmp_path):
    """g. A missing or damaged model file, or a threshold above 256: DWPA_RC_ERROR before any launch."""
    (tmp_path / "cut.dwmk").write_bytes(models[0]["img"][:-1])
    twice = bytearray(models[0]["img"])
    twice[16 + 300] = twice[16 + 301]
    (tmp_path / "twice.dwmk").write_bytes(bytes(twice))
    lines = fa["lines"][:A_K]
    for path in ("missing.dwmk", "cut.dwmk", "twice.dwmk"):
        assert _crack(tmp_path, lines, A_MASK, A_CUSTOM, markov=str(tmp_path / path), threshold=A_T) == (-1, [], frozenset())
    lib = L.load()
    assert lib.dwpa_crack_mask_markov(str(tmp_path / "h.hash").encode(), A_MASK, None, models[0]["path"].encode(), 257, 0, 0,
                                      0, 0, NC, str(tmp_path / "o.key").encode(), None) == L.DWPA_RC_ERROR
    assert L.pbkdf2_kernels() == frozenset()


INC_MASK, INC_CUSTOM, INC_T = b"?1" * 10, (b"012",), 2


@pytest.fixture(scope="module")
def finc(models):
    """Every candidate of the increment 8..10 run of INC_MASK under threshold 2 (256 + 512 + 1024)."""
    lines, psks = [], []
    for n in (8, 9, 10):
        ln, _, ps = plant(models[1], b"?1" * n, INC_CUSTOM, INC_T, [(0, 2**n)], ONE, 0x60 + n)
        lines += ln
        psks += ps
    assert len(lines) == 1792 and {len(p) for p in psks} == {8, 9, 10}
    return {"lines": lines, "psk": psks}


def test_crack_increment(models, finc, tmp_path):
    """g. Increment 8..10: the prefixes of 8, 9 and 10 positions under one model, shortest first: rc 0."""
    rc, recs, ran = _crack(tmp_path, finc["lines"], INC_MASK, INC_CUSTOM, markov=models[1]["path"], threshold=INC_T,
                           increment=(8, 10))
    assert rc == 0 and recs == sorted(R._records(finc["lines"], finc["psk"]))
    assert ran and ran <= R.MG_KERNELS, ran
    assert M.crack_stats()["candidates"] == 1792
    assert M.crack_worker_stats()[0]["items"] == 1 + 1 + 2  # batches of 512 never span two lengths


_SHARDS_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import dwpa_amd
from dwpa_amd import m22000 as M
rc = dwpa_amd.crack_mask(sys.argv[2], "?1" * 10, (b"012",), increment=(8, 10), nonce_error_corrections=int(sys.argv[4]),
                         out_file=sys.argv[3], batch=512, markov=sys.argv[5], threshold=2)
print(json.dumps({"rc": rc, "stats": M.crack_stats(), "workers": M.crack_worker_stats()}))
"""


def test_crack_two_workers(models, finc, tmp_path):
    """g. The same increment run with two workers on one device (DWPA_CRACK_SHARDS_PER_DEVICE=2, in a child): every
    line is cracked exactly once and the workers' candidates sum to the derived total."""
    hf, out = tmp_path / "h.hash", tmp_path / "o.key"
    hf.write_bytes(b"\n".join(finc["lines"]) + b"\n")
    env = dict(os.environ, DWPA_CRACK_SHARDS_PER_DEVICE="2")
    r = subprocess.run([sys.executable, "-c", _SHARDS_CHILD, ROOT, str(hf), str(out), str(NC), models[1]["path"]],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["rc"] == 0
    recs = out.read_bytes().split(b"\n")
    assert recs.pop() == b"" and sorted(recs) == sorted(R._records(finc["lines"], finc["psk"]))
    assert len(res["workers"]) == 2 and len({w["device"] for w in res["workers"]}) == 1
    assert sum(w["candidates"] for w in res["workers"]) == res["stats"]["candidates"] == 1792
