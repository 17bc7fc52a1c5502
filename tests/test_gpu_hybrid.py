"""GPU recall of the hybrid attacks: k_prep_hybrid through the scan API (set_mask / load_hybrid) and dwpa_crack_hybrid.

The all-plants method of tests/test_gpu_recall.py: EVERY kept candidate (word x mask index) is the PSK of one line per
ESSID, the expected set comes from the CPU oracle, and the hits must equal it -- none missing, none extra, none twice,
ids and PMKs equal.  The mask candidates come from the reference expander of tests/test_mask.py, the joins and the
filter are restated here in Python.  Batch sizes follow from the device's CU count as in test_gpu_recall, and every
scan test asserts which PBKDF2 kernel ran.
"""
import gzip
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
from dwpa_amd.device import Dictionary  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import test_gpu_recall as R  # noqa: E402
from tests.join_plan import hybrid_join as join, kept_words  # noqa: E402,F401  (the join and the filter)
from tests.test_gpu_recall import sizes  # noqa: E402,F401  (the fixture)
from tests.test_mask import ref_candidate, ref_sets  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC = R.NC
ONE = (b"hybrid-recall",)
H_MASK, H_CUSTOM = b"?1x?2", (b"ab", b"cde")  # K = 6, P = 3


def plant(words, mask, custom, loads, mode, essids, seed):
    """One line per (essid, candidate) for the kept candidates of `loads` [(first_word, nwords, mask_first,
    mask_count)].  Returns (lines, expected hits {(line, id, nc, endian, pmk)}, the PSK of each line)."""
    sets, k = ref_sets(mask, custom)
    kept = set(kept_words(words, len(sets)))
    ids = sorted({w * k + j for fw, nw, mf, mc in loads for w in range(fw, fw + nw) if w in kept
                  for j in range(mf, mf + mc)})
    psks = [join(words[i // k], ref_candidate(sets, i % k), mode) for i in ids]
    assert ids and len(set(psks)) == len(psks), "a PSK twice"
    assert len({p.rstrip(b"\0") for p in psks}) == len(psks), "two PSKs that are one HMAC key"
    assert all(8 <= len(p) <= 63 for p in psks)
    lines, owner, pmks, found = R._plant_lines(psks, essids, random.Random(seed))
    exp = {(ln, ids[i], nc, en, pmk) for ln, ((e, i), (nc, en), pmk) in enumerate(zip(owner, found, pmks))}
    return lines, exp, [psks[i] for e, i in owner]


def window_ids(words, npos, k, load):
    """The ids of a load in slot order (the compaction keeps lane order: word-major, mask index fastest)."""
    fw, nw, mf, mc = load
    kept = set(kept_words(words, npos))
    return [w * k + j for w in range(fw, fw + nw) if w in kept for j in range(mf, mf + mc)]


def recall(lines, exp, words, mask, custom, loads, mode, batch, how, kernel):
    """set_mask once, then every load: loaded() == the kept count and the hits are exactly the load's plants."""
    sets, k = ref_sets(mask, custom)
    d = Dictionary.from_words(words)
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(lines, nc=NC, batch=batch)
    held = set()
    try:
        assert sc.set_mask(mask, custom) == k
        for load in loads:
            ids = window_ids(words, len(sets), k, load)
            slots = set(enumerate(ids))
            assert not slots & held, "a slot would hold a candidate it held before"
            held |= slots
            fw, nw, mf, mc = load
            sc.load_hybrid(d.off.ptr, d.data.ptr, fw, nw, mf, mc, mode)
            assert sc.loaded() == len(ids), load
            R._scan_all(sc, how)
            R._assert_same(R._hitset(sc.hits(cap=4096)), {p for p in exp if p[1] in set(ids)}, (mode, how, load))
    finally:
        sc.close()
    assert L.pbkdf2_kernels() == {kernel}


# ---------------------------------------------------------------------------------------------------------------
# fixture H
# ---------------------------------------------------------------------------------------------------------------
def _build_h():
    """Every length 0..66 once and one 300-byte word; 0..2 at the start, 3, 4 and 61..63 in the middle, 64..66 and
    300 at the end are dropped with P = 3, the 56 words of 5..60 bytes are kept.  The order of the kept lengths is
    the first shuffle under which they cover every (L % 4, offset % 4) pair."""
    for seed in range(1000):
        rng = random.Random(0x4859 + seed)
        mid = list(range(5, 61))
        rng.shuffle(mid)
        for pos, n in ((10, 3), (20, 61), (30, 4), (40, 62), (50, 63)):
            mid.insert(pos, n)
        lens = [0, 1, 2] + mid + [64, 65, 66, 300]
        off, pairs = 0, set()
        for n in lens:
            if 5 <= n <= 60:
                pairs.add((n % 4, off % 4))
            off += n
        if len(pairs) == 16:
            break
    else:
        raise AssertionError("no order covers every (L % 4, offset % 4) pair")
    seen, words = set(), []
    for i, n in enumerate(lens):
        words.append(R._word(rng, n, i % 5 == 3, seen) if n else b"")
    return words


@pytest.fixture(scope="module")
def fh():
    """Fixture H: all 336 candidates planted, mode 6 under the three ESSIDs of test_gpu_recall (one of 52 bytes),
    mode 7 under one."""
    words = _build_h()
    sets, k = ref_sets(H_MASK, H_CUSTOM)
    assert (len(sets), k) == (3, 6)
    kept = kept_words(words, 3)
    offs = [0]
    for w in words:
        offs.append(offs[-1] + len(w))
    assert sorted(len(w) for w in words) == list(range(67)) + [300]
    assert [len(words[i]) for i in kept] != sorted(len(words[i]) for i in kept)
    assert sorted(len(words[i]) for i in kept) == list(range(5, 61))
    assert {(len(words[i]) % 4, offs[i] % 4) for i in kept} == {(a, b) for a in range(4) for b in range(4)}
    dropped = [i for i in range(len(words)) if i not in kept]
    assert dropped[0] == 0 and dropped[-1] == len(words) - 1 and any(kept[0] < i < kept[-1] for i in dropped)
    assert kept != list(range(kept[0], kept[0] + len(kept)))  # slots move: ids[] must carry the id
    assert any(any(c >= 0x80 for c in words[i]) for i in kept)  # binary words among the kept
    assert not any(b"\n" in w or b"\r" in w for w in words)
    every = [(0, len(words), 0, 6)]
    l6, e6, p6 = plant(words, H_MASK, H_CUSTOM, every, 6, R.ESSIDS, 0x66)
    l7, e7, p7 = plant(words, H_MASK, H_CUSTOM, every, 7, ONE, 0x77)
    assert len(l6) == 3 * 336 and len(l7) == 336
    return {"words": words, "kept": kept, 6: {"lines": l6, "exp": e6, "psk": p6}, 7: {"lines": l7, "exp": e7, "psk": p7}}


def _span(kept, first_kept, n):
    """(first_word, nwords) of the words from kept word number first_kept to the n-th kept word after it."""
    return kept[first_kept], kept[first_kept + n - 1] + 1 - kept[first_kept]


def h_loads(fh):
    """Loads whose kept counts are 1, 63, 64, 65, 255, 258 and all 336.  With 56 kept words and K = 6 a load is a
    rectangle of at most 56 x 6: no load keeps 256 (2^8) or 257 (prime); 255 = 51 x 5 and 258 = 43 x 6 stand on
    either side of the 256-lane block and the four-wave boundary instead, and the raw lane counts (dropped words
    included) cross 256 as well.  Several loads have mask_first > 0 and mask_count in (3, 5), which are no powers of
    two; the 64-load starts at a dropped word inside the dictionary."""
    words, kept = fh["words"], fh["kept"]
    n = len(words)
    inner = next(i for i in range(kept[0], n) if i not in kept)  # a dropped word after the first kept one
    after = [i for i in kept if i > inner]
    loads = [(0, kept[0] + 1, 5, 1),                              # 1: three dropped words, then one lane kept
             (0, kept[20] + 1, 2, 3),                             # 63 = 21 x 3
             (inner, after[15] + 1 - inner, 1, 4),                # 64 = 16 x 4, from a dropped word
             (0, kept[12] + 1, 1, 5),                             # 65 = 13 x 5
             (*_span(kept, 2, 51), 1, 5),                         # 255 = 51 x 5
             (*_span(kept, 13, 43), 0, 6),                        # 258 = 43 x 6, to the last kept word
             (0, n, 0, 6)]                                        # all
    got = [len(window_ids(words, 3, 6, ld)) for ld in loads]
    assert got == [1, 63, 64, 65, 255, 258, 336], got
    assert any(ld[1] * ld[3] > 256 for ld in loads) and loads[2][0] not in kept and loads[2][0] > kept[0]
    return loads


# ---------------------------------------------------------------------------------------------------------------
# a: lanes and waves
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [6, 7])
def test_lanes_and_waves_per_group(fh, sizes, mode):
    """a. pbkdf2(g) / verify(g) on one ESSID, both modes."""
    f = fh[mode]
    lines, exp = f["lines"][:336], {p for p in f["exp"] if p[0] < 336}
    recall(lines, exp, fh["words"], H_MASK, H_CUSTOM, h_loads(fh), mode, sizes["one"]["p"], "per_group",
           R.expected_kernel("one", "p"))


def test_lanes_and_waves_run(fh, sizes):
    """a. The same loads through run() over three ESSIDs, one of them 52 bytes long (mode 6)."""
    recall(fh[6]["lines"], fh[6]["exp"], fh["words"], H_MASK, H_CUSTOM, h_loads(fh), 6, sizes["mg"]["p"], "run",
           R.expected_kernel("mg", "p"))


# ---------------------------------------------------------------------------------------------------------------
# b: long and short masks
# ---------------------------------------------------------------------------------------------------------------
LONG = b"?d" + b"L" * 53 + b"?l"  # P = 55, K = 260


def _printable(rng, lengths):
    seen = set()
    return [R._word(rng, n, False, seen) if n else b"" for n in lengths]


@pytest.mark.parametrize("mode", [6, 7])
def test_long_mask(sizes, mode):
    """b. P = 55 with words of 0..9 bytes: 0..8 are kept (55..63 bytes), 9 is dropped at 64.  A 10-index window
    that carries into the first position is planted for every kept word."""
    words = _printable(random.Random(0xb0), range(10))
    assert kept_words(words, 55) == list(range(9))
    loads = [(0, 10, 125, 10)]  # index 129 -> 130: ?l wraps, ?d steps
    lines, exp, psks = plant(words, LONG, (), loads, mode, ONE, 0xb0 + mode)
    assert len(lines) == 90 and {len(p) for p in psks} == set(range(55, 64))
    recall(lines, exp, words, LONG, (), loads, mode, sizes["one"]["p"], "per_group", R.expected_kernel("one", "p"))


@pytest.mark.parametrize("mode", [6, 7])
def test_short_mask(sizes, mode):
    """b. P = 1 with words of 6..63 bytes: 7..62 are kept.  Mask indices 0 and 9 are planted, all 10 are loaded."""
    words = _printable(random.Random(0xb1), range(6, 64))
    assert [len(words[i]) for i in kept_words(words, 1)] == list(range(7, 63))
    n = len(words)
    lines, exp, _ = plant(words, b"?d", (), [(0, n, 0, 1), (0, n, 9, 1)], mode, ONE, 0xb8 + mode)
    assert len(lines) == 112
    sc_loads = [(0, n, 0, 10)]
    d = Dictionary.from_words(words)
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(lines, nc=NC, batch=sizes["one"]["p"])
    try:
        assert sc.set_mask(b"?d") == 10
        sc.load_hybrid(d.off.ptr, d.data.ptr, *sc_loads[0], mode)
        assert sc.loaded() == 560
        R._scan_all(sc, "per_group")
        R._assert_same(R._hitset(sc.hits(cap=4096)), exp, ("short", mode))
    finally:
        sc.close()
    assert L.pbkdf2_kernels() == {R.expected_kernel("one", "p")}


# ---------------------------------------------------------------------------------------------------------------
# c: wide indices
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,loads", [(6, [(0, 1, 2**32 - 50, 100), (0, 1, 95**5 - 100, 100)]),
                                        (7, [(0, 1, 95**5 - 100, 100)])])
def test_wide_indices(sizes, mode, loads):
    """c. ?a x 5 (K = 95^5 > 2^32) with the single word abc: a window across index 2^32 and the last 100 indices."""
    lines, exp, _ = plant([b"abc"], b"?a" * 5, (), loads, mode, ONE, 0xc0 + mode)
    assert len(lines) == 100 * len(loads) and {p[1] for p in exp} == {i for ld in loads for i in range(ld[2], ld[2] + 100)}
    recall(lines, exp, [b"abc"], b"?a" * 5, (), loads, mode, sizes["one"]["p"], "per_group",
           R.expected_kernel("one", "p"))


# ---------------------------------------------------------------------------------------------------------------
# d: equal to the mask path
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,word,whole", [(6, b"pre", b"pre?d?d?d?d?d"), (7, b"suf", b"?d?d?d?d?dsuf")])
def test_equal_to_the_mask_path(sizes, mode, word, whole):
    """d. One word x ?d x 5 over a planted window gives the hits of the literal mask's load_mask, ids included."""
    first, count = 12_345, 100
    lines, exp, psks = plant([word], b"?d" * 5, (), [(0, 1, first, count)], mode, ONE, 0xd0 + mode)
    assert sorted(psks) == [join(word, b"%05d" % v, mode) for v in range(first, first + count)]
    d = Dictionary.from_words([word])
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(lines, nc=NC, batch=sizes["one"]["p"])
    try:
        assert sc.set_mask(b"?d" * 5) == 10**5
        sc.load_hybrid(d.off.ptr, d.data.ptr, 0, 1, first, count, mode)
        assert sc.loaded() == count
        R._scan_all(sc, "per_group")
        by_hybrid = R._hitset(sc.hits(cap=4096))
        assert sc.set_mask(whole) == 10**5
        sc.load_mask(first, count)
        assert sc.loaded() == count
        R._scan_all(sc, "per_group")
        by_mask = R._hitset(sc.hits(cap=4096))
    finally:
        sc.close()
    R._assert_same(by_hybrid, exp, "hybrid")
    assert by_hybrid == by_mask
    assert L.pbkdf2_kernels() == {R.expected_kernel("one", "p")}


# ---------------------------------------------------------------------------------------------------------------
# e: argument errors on a live scan
# ---------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_scan_usable(fh, sizes):
    f = fh[6]
    lines, exp = f["lines"][:336], {p for p in f["exp"] if p[0] < 336}
    words = fh["words"]
    d = Dictionary.from_words(words)
    n = len(words)
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(lines, nc=NC, batch=sizes["one"]["p"])

    def refused(*load, mode=6):
        with pytest.raises(L.DwpaError) as e:
            sc.load_hybrid(d.off.ptr, d.data.ptr, *load, mode)
        assert e.value.code == L.DWPA_E_ARG

    try:
        refused(0, 1, 0, 1)  # no mask set
        assert sc.set_mask(b"?d" * 19) == 10**19
        refused(2, 1, 0, 1)  # (first_word + nwords) * K = 3 * 10^19 is beyond 64 bits
        refused(2**64 - 1, 1, 0, 1)  # first_word + nwords wraps
        assert sc.set_mask(H_MASK, H_CUSTOM) == 6
        for mode in (0, 3, 5, 8, -6):
            refused(0, n, 0, 6, mode=mode)
        refused(0, sc.batch // 6 + 1, 0, 6)  # nwords * mask_count > batch
        refused(0, sc.batch + 1, 0, 1)
        refused(0, 2**32 - 1, 0, 6)  # the product is beyond 32 bits
        refused(0, n, 1, 6)  # mask_first + mask_count > K
        refused(0, n, 6, 1)
        refused(0, n, 7, 0)
        refused(0, n, 2**64 - 1, 2)  # the sum wraps
        load = (0, n, 1, 5)
        sc.load_hybrid(d.off.ptr, d.data.ptr, *load, 6)
        ids = window_ids(words, 3, 6, load)
        assert sc.loaded() == len(ids) == 280
        R._scan_all(sc, "per_group")
        R._assert_same(R._hitset(sc.hits(cap=4096)), {p for p in exp if p[1] in set(ids)}, "after the errors")
        sc.load_hybrid(d.off.ptr, d.data.ptr, 0, n, 6, 0, 6)  # an empty window is a load of nothing
        assert sc.loaded() == 0
    finally:
        sc.close()
    assert L.pbkdf2_kernels() == {R.expected_kernel("one", "p")}


# ---------------------------------------------------------------------------------------------------------------
# f: dwpa_crack_hybrid
# ---------------------------------------------------------------------------------------------------------------
def _crack(tmp_path, lines, dicts, mask, custom, mode, batch=512):
    hf, out = tmp_path / "h.hash", tmp_path / "o.key"
    hf.write_bytes(b"\n".join(lines) + b"\n")
    if out.exists():
        out.unlink()
    L.pbkdf2_kernels(reset=True)
    rc, st = dwpa_amd.crack_hybrid(str(hf), [str(p) for p in dicts], mask, custom, mode, NC, str(out), batch=batch)
    ran = L.pbkdf2_kernels()
    recs = out.read_bytes().split(b"\n") if out.exists() else [b""]
    assert recs.pop() == b"" and st == [L.DWPA_DICT_OK] * len(dicts)
    assert ran and ran <= R.MG_KERNELS, ran
    return rc, sorted(recs)


def _h_gzip(fh, path):
    """Fixture H as a .gz with CRLF endings in its first half and one $HEX[] entry."""
    words = list(fh["words"])
    hexed = fh["kept"][10]
    words[hexed] = b"$HEX[" + words[hexed].hex().encode() + b"]"
    half = len(words) // 2
    with gzip.open(path, "wb") as f:
        f.write(b"".join(w + b"\r\n" for w in words[:half]) + b"".join(w + b"\n" for w in words[half:]))


def test_crack_hybrid_word_mask(fh, tmp_path):
    """f1. Fixture H from a gzip dictionary, mode 6, three ESSIDs: rc 0, every line once with its PSK."""
    d = tmp_path / "h.txt.gz"
    _h_gzip(fh, d)
    rc, recs = _crack(tmp_path, fh[6]["lines"], [d], H_MASK, H_CUSTOM, 6)
    assert rc == 0 and recs == sorted(R._records(fh[6]["lines"], fh[6]["psk"]))
    st = M.crack_stats()
    assert (st["hashes"], st["cracked"]) == (3 * 336, 3 * 336) and st["candidates"] <= 336


def test_crack_hybrid_mask_word(fh, tmp_path):
    """f2. Mode 7 from a plain file."""
    d = tmp_path / "h.txt"
    d.write_bytes(b"".join(w + b"\n" for w in fh["words"]))
    rc, recs = _crack(tmp_path, fh[7]["lines"], [d], H_MASK, H_CUSTOM, 7)
    assert rc == 0 and recs == sorted(R._records(fh[7]["lines"], fh[7]["psk"]))


@pytest.mark.parametrize("mode", [6, 7])
def test_crack_hybrid_mask_wider_than_the_batch(tmp_path, mode):
    """f3. ?d?d?d (K = 1000) at batch 64, the smallest a scan takes: 16 launches per kept word, plants at mask indices
    0, 63, 64 and 999 of three kept words among dropped ones.  f4. With one more line whose PSK is no candidate the
    run is exhausted: rc 1, candidates = kept words x K, words = the lines read."""
    rng = random.Random(0xf3 + mode)
    words = _printable(rng, (2, 5, 61, 17, 0, 60, 300))
    kept = kept_words(words, 3)
    assert [len(words[i]) for i in kept] == [5, 17, 60]
    loads = [(0, len(words), j, 1) for j in (0, 63, 64, 999)]
    lines, _, psks = plant(words, b"?d?d?d", (), loads, mode, ONE, 0xf30 + mode)
    assert len(lines) == 12
    d = tmp_path / "d.txt"
    d.write_bytes(b"".join(w + b"\n" for w in words))
    rc, recs = _crack(tmp_path, lines, [d], b"?d?d?d", (), mode, batch=64)
    assert rc == 0 and recs == sorted(R._records(lines, psks))
    outside = join(words[kept[0]], b"12x", mode)
    extra = R._line(0, 0, "LE", outside, ONE[0], O.c_pbkdf2(outside, ONE[0]), rng)
    rc, recs = _crack(tmp_path, lines + [extra], [d], b"?d?d?d", (), mode, batch=64)
    assert rc == 1 and recs == sorted(R._records(lines, psks))
    st = M.crack_stats()
    assert (st["words"], st["candidates"], st["hashes"], st["cracked"]) == (len(words), 3 * 1000, 13, 12)
    ws = M.crack_worker_stats()
    assert len(ws) == 1 and ws[0]["candidates"] == 3000 and ws[0]["words"] == len(words)


def test_crack_hybrid_exhausted(fh, tmp_path):
    """f4. K <= batch: fixture H, mode 7, plus a line no candidate cracks: rc 1, the other records present,
    candidates = 56 kept words x 6, words = the 68 lines of the dictionary.  K = 1 (a literal mask) sizes the items as
    a plain dictionary run and finds its plants."""
    rng = random.Random(0xf4)
    d = tmp_path / "h.txt"
    d.write_bytes(b"".join(w + b"\n" for w in fh["words"]))
    outside = b"bxf-not-a-candidate"
    extra = R._line(0, 0, "LE", outside, ONE[0], O.c_pbkdf2(outside, ONE[0]), rng)
    rc, recs = _crack(tmp_path, fh[7]["lines"] + [extra], [d], H_MASK, H_CUSTOM, 7)
    assert rc == 1 and recs == sorted(R._records(fh[7]["lines"], fh[7]["psk"]))
    st = M.crack_stats()
    assert (st["words"], st["candidates"], st["cracked"]) == (len(fh["words"]), 56 * 6, 336)
    # K = 1: the candidates bxe + word of fixture H, mode 7, are index 5 of H_MASK
    at = [k for k, p in enumerate(fh[7]["psk"]) if p.startswith(b"bxe")]
    lines, psks = [fh[7]["lines"][k] for k in at], [fh[7]["psk"][k] for k in at]
    assert len(lines) == 56
    rc, recs = _crack(tmp_path, lines + [extra], [d], b"bxe", (), 7)
    assert rc == 1 and recs == sorted(R._records(lines, psks))
    st = M.crack_stats()
    assert (st["words"], st["candidates"], st["cracked"]) == (len(fh["words"]), 56, 56)


_SHARDS_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import dwpa_amd
from dwpa_amd import m22000 as M
rc, st = dwpa_amd.crack_hybrid(sys.argv[2], [sys.argv[5]], "?1x?2", (b"ab", b"cde"), 6,
                               nonce_error_corrections=int(sys.argv[4]), out_file=sys.argv[3], batch=64)
print(json.dumps({"rc": rc, "dict": st, "stats": M.crack_stats(), "workers": M.crack_worker_stats()}))
"""


def test_crack_hybrid_two_workers(fh, tmp_path):
    """f5. Fixture H, mode 6, with DWPA_CRACK_SHARDS_PER_DEVICE=2 (read per call; a child keeps this process's
    environment as it is): every line is cracked and each outfile record is written once."""
    hf, out, d = tmp_path / "h.hash", tmp_path / "o.key", tmp_path / "h.txt.gz"
    hf.write_bytes(b"\n".join(fh[6]["lines"]) + b"\n")
    _h_gzip(fh, d)
    env = dict(os.environ, DWPA_CRACK_SHARDS_PER_DEVICE="2")
    r = subprocess.run([sys.executable, "-c", _SHARDS_CHILD, ROOT, str(hf), str(out), str(NC), str(d)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["rc"] == 0 and res["dict"] == [L.DWPA_DICT_OK]
    recs = out.read_bytes().split(b"\n")
    assert recs.pop() == b"" and sorted(recs) == sorted(R._records(fh[6]["lines"], fh[6]["psk"]))
    assert len(res["workers"]) == 2 and len({w["device"] for w in res["workers"]}) == 1
    assert sum(w["candidates"] for w in res["workers"]) == res["stats"]["candidates"] <= 336
    assert sum(w["words"] for w in res["workers"]) == res["stats"]["words"] <= len(fh["words"])
    assert res["stats"]["cracked"] == 3 * 336
