"""GPU recall of the combinator attack: k_prep_combinator through the scan API (load_combinator) and
dwpa_crack_combinator.

The all-plants method of tests/test_gpu_recall.py and tests/test_gpu_hybrid.py: EVERY kept pair of a load is the PSK of
one line per ESSID, the expected set is restated here in Python (join, filter, order, id), and the hits must equal it
-- none missing, none extra, none twice, ids and PMKs equal -- while loaded() must equal the kept count.  Batch sizes
follow from the device's CU count as in test_gpu_recall, and every scan test asserts which PBKDF2 kernel ran.

A load is a rectangle (first_base, nbase, amp_first, amp_count) of one list (the base) x another (the amplifier); the
side says which of the two stands left in the join: 0 = base + amplifier word, 1 = amplifier word + base.
"""
import gzip
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import dwpa_amd  # noqa: E402
from dwpa_amd import _lib as L  # noqa: E402
from dwpa_amd import m22000 as M  # noqa: E402
from dwpa_amd.device import Dictionary  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import test_gpu_recall as R  # noqa: E402
from tests.join_plan import combi_join as join, keeps  # noqa: E402,F401  (the join and the filter)
from tests.test_gpu_recall import sizes  # noqa: E402,F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC = R.NC
ONE = (b"combi-recall",)
RIGHT, LEFT = L.DWPA_COMBI_AMP_RIGHT, L.DWPA_COMBI_AMP_LEFT
Y_LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 30, 31, 32, 33, 55, 56, 62, 63, 64, 300)


def load_pairs(base, amp, load):
    """The kept (base index, amplifier index) pairs of a load in slot order: the compaction keeps lane order, which
    is base-major with the amplifier index fastest."""
    fb, nb, af, ac = load
    return [(b, a) for b in range(fb, fb + nb) for a in range(af, af + ac) if keeps(base[b], amp[a])]


def plant(psks, essids, seed):
    """One line per (essid, PSK).  Returns (lines, [(psk, nc, endian, pmk) of each line])."""
    assert psks and len(set(psks)) == len(psks), "a PSK twice"
    assert len({p.rstrip(b"\0") for p in psks}) == len(psks), "two PSKs that are one HMAC key"
    assert all(8 <= len(p) <= 63 for p in psks)
    lines, owner, pmks, found = R._plant_lines(psks, essids, random.Random(seed))
    return lines, [(psks[i], nc, en, pmk) for (e, i), (nc, en), pmk in zip(owner, found, pmks)]


def expected(recs, base, amp, side, pairs=None):
    """The hits {(line, id, nc, endian, pmk)} of the planted lines whose PSK is a pair of `pairs` (default: every
    kept pair), id = base index * A + amplifier index."""
    if pairs is None:
        pairs = load_pairs(base, amp, (0, len(base), 0, len(amp)))
    ids = {join(base[b], amp[a], side): b * len(amp) + a for b, a in pairs}
    assert len(ids) == len(pairs)
    return {(ln, ids[psk], nc, en, pmk) for ln, (psk, nc, en, pmk) in enumerate(recs) if psk in ids}


def recall(lines, recs, base, amp, side, loads, batch, how, kernel):
    """Every load on one scan: loaded() == the kept count and the hits are exactly the load's plants."""
    db, da = Dictionary.from_words(base), Dictionary.from_words(amp)
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(lines, nc=NC, batch=batch)
    held = set()
    try:
        for load in loads:
            pairs = load_pairs(base, amp, load)
            slots = set(enumerate(pairs))
            assert not slots & held, "a slot would hold a candidate it held before"
            held |= slots
            fb, nb, af, ac = load
            sc.load_combinator(db.off.ptr, db.data.ptr, fb, nb, da.off.ptr, da.data.ptr, len(amp), af, ac, side)
            assert sc.loaded() == len(pairs), load
            R._scan_all(sc, how)
            exp = expected(recs, base, amp, side, pairs)
            assert len(exp) == len(pairs) * len(lines) // len({r[0] for r in recs})
            R._assert_same(R._hitset(sc.hits(cap=4096)), exp, (side, how, load))
    finally:
        sc.close()
    assert L.pbkdf2_kernels() == {kernel}


# ---------------------------------------------------------------------------------------------------------------
# the fixture: lists X and Y
# ---------------------------------------------------------------------------------------------------------------
def _build_lists():
    """X: every length 0..66 once and one 300-byte word.  The words of 0..63 bytes are each kept with some word of Y;
    those of 64, 65, 66 and 300 bytes never are and stand first (64), inside (65, 66) and last (300).  The order of
    the others is the first shuffle under which they cover every (length % 4, byte offset % 4) pair.
    Y: the 19 lengths of Y_LENGTHS, shuffled; its two never-kept words stand first (64) and last (300) -- with two such
    words Y cannot also hold one inside, X does.  Binary bytes stand in every fifth word; no word is in both lists."""
    for seed in range(1000):
        rng = random.Random(0x4331 + seed)
        mid = list(range(64))
        rng.shuffle(mid)
        mid.insert(20, 65)
        mid.insert(45, 66)
        xl = [64] + mid + [300]
        off, pairs = 0, set()
        for n in xl:
            if 1 <= n <= 63:
                pairs.add((n % 4, off % 4))
            off += n
        if len(pairs) == 16:
            break
    else:
        raise AssertionError("no order covers every (L % 4, offset % 4) pair")
    yl = [n for n in Y_LENGTHS if n < 64]
    rng.shuffle(yl)
    yl = [64] + yl + [300]
    seen = set()
    xs = [R._word(rng, n, i % 5 == 3, seen) if n else b"" for i, n in enumerate(xl)]
    ys = [R._word(rng, n, i % 5 == 2, seen) if n else b"" for i, n in enumerate(yl)]
    return xs, ys


@pytest.fixture(scope="module")
def fc():
    """Lists X and Y with all 653 kept pairs planted: as x + y under the three ESSIDs of test_gpu_recall (one of 52
    bytes), as y + x under one."""
    xs, ys = _build_lists()
    assert sorted(len(w) for w in xs) == list(range(67)) + [300] and len(xs) == 68
    assert sorted(len(w) for w in ys) == sorted(Y_LENGTHS) and len(ys) == 19
    assert not any(b"\n" in w or b"\r" in w for w in xs + ys)
    assert any(any(c >= 0x80 for c in w) for w in xs) and any(any(c >= 0x80 for c in w) for w in ys)
    dead = lambda ws: [i for i, w in enumerate(ws) if len(w) > 63]  # noqa: E731
    assert dead(xs)[0] == 0 and dead(xs)[-1] == len(xs) - 1 and any(0 < i < len(xs) - 1 for i in dead(xs))
    assert dead(ys) == [0, len(ys) - 1]
    offs = [0]
    for w in xs:
        offs.append(offs[-1] + len(w))
    assert {(len(w) % 4, offs[i] % 4) for i, w in enumerate(xs) if 1 <= len(w) <= 63} == \
        {(a, b) for a in range(4) for b in range(4)}
    pairs = load_pairs(xs, ys, (0, len(xs), 0, len(ys)))
    assert len(xs) * len(ys) == 1292 and len(pairs) == 653
    lens = {(len(xs[b]), len(ys[a])) for b, a in pairs}
    assert {(lx % 4, ly % 4) for lx, ly in lens} == {(a, b) for a in range(4) for b in range(4)}
    every = {(len(x), len(y)) for x in xs for y in ys}
    for lr in ((0, 63), (63, 0), (0, 8), (8, 0), (1, 62), (62, 1), (31, 32), (32, 31)):
        assert lr in lens, lr
    for lr in ((0, 7), (7, 0), (0, 64), (64, 0), (32, 32), (63, 1), (1, 63), (300, 8), (8, 300), (300, 300)):
        assert lr in every and lr not in lens, lr
    # kept pairs do not stand in one run: slots move, ids[] must carry the id
    ids = [b * len(ys) + a for b, a in pairs]
    assert ids != list(range(ids[0], ids[0] + len(ids)))
    xy = [xs[b] + ys[a] for b, a in pairs]
    yx = [ys[a] + xs[b] for b, a in pairs]
    lxy, rxy = plant(xy, R.ESSIDS, 0xc1)
    lyx, ryx = plant(yx, ONE, 0xc2)
    assert len(lxy) == 3 * 653 and len(lyx) == 653
    return {"x": xs, "y": ys, "xy": {"lines": lxy, "recs": rxy}, "yx": {"lines": lyx, "recs": ryx}}


def _counts(base, amp):
    """cnt[fb, eb, af, ea]: the kept pairs of the load rectangle base[fb:eb] x amp[af:ea], for every rectangle."""
    k = np.array([[keeps(b, a) for a in amp] for b in base], dtype=np.int64)
    p = np.zeros((len(base) + 1, len(amp) + 1), dtype=np.int64)
    p[1:, 1:] = k.cumsum(0).cumsum(1)
    fb, eb, af, ea = np.ix_(*[np.arange(n + 1) for n in (len(base), len(base), len(amp), len(amp))])
    cnt = p[eb, ea] - p[fb, ea] - p[eb, af] + p[fb, af]
    valid = (eb > fb) & (ea > af)
    raw = (eb - fb) * (ea - af)
    return cnt, valid, raw, (fb, eb, af, ea)


def combi_loads(base, amp):
    """The loads of test a, searched among ALL load rectangles of base x amp: kept counts 1, the achievable counts
    nearest 64 on both sides (and 64 itself if a rectangle gives it), the achievable counts nearest 256 on both sides
    with more than 256 raw lanes, and everything.  Where a rectangle with the wanted property exists it is taken:
    the 1-load starts at a base word that keeps nothing, the load under 64 has amp_count in {1, 3, 5}, the load over
    64 has amp_first > 0, and with an amplifier of 64 words or more the load over 256 has 64 <= amp_count that is no
    multiple of 64 and not the whole amplifier (_checked_loads asserts what each pair of lists gives).  No load puts a
    pair into a slot in which another load has it."""
    cnt, valid, raw, (fb, eb, af, ea) = _counts(base, amp)
    got = np.unique(cnt[valid])
    wide = np.unique(cnt[valid & (raw > 256)])
    n_all = int(cnt[0, len(base), 0, len(amp)])
    targets = [1, int(got[got < 64].max())] + ([64] if 64 in got else []) + \
        [int(got[got > 64].min()), int(wide[wide < 256].max()), int(wide[wide > 256].min()), n_all]
    dead_start = np.array([len(w) > 63 for w in base] + [False])[fb]
    small_ac = np.isin(ea - af, (1, 3, 5))
    odd_big = ((ea - af) >= 64) & ((ea - af) % 64 != 0) & ((ea - af) < len(amp))
    wish = {1: dead_start, targets[1]: small_ac, targets[-4]: af > 0, targets[-3]: raw > 256,
            targets[-2]: (raw > 256) & (odd_big if len(amp) >= 64 else True)}
    loads, held = {}, set()
    for t in [n_all] + targets[:-1]:  # the whole product first: the others then avoid its slots
        ok = valid & (cnt == t)
        if t == n_all:
            ok = ok & (fb == 0) & (eb == len(base)) & (af == 0) & (ea == len(amp))
        if (ok & wish.get(t, True)).any():  # the property is a wish: not every count has a rectangle with it
            ok = ok & wish.get(t, True)
        for f, e, a, z in np.argwhere(ok):
            load = (int(f), int(e - f), int(a), int(z - a))
            slots = set(enumerate(load_pairs(base, amp, load)))
            if not slots & held:
                held |= slots
                loads[t] = load
                break
        else:
            raise AssertionError("no load keeps %d pairs with its property" % t)
    loads = [loads[t] for t in targets]
    if len(amp) >= 64 and not any(64 <= c < len(amp) and c % 64 for f, n, a, c in loads):
        # one more load, for a wave that holds one base word only: the first rectangle with such an amp_count
        for f, e, a, z in np.argwhere(valid & odd_big & (cnt > 64)):
            load = (int(f), int(e - f), int(a), int(z - a))
            slots = set(enumerate(load_pairs(base, amp, load)))
            if not slots & held:
                loads.insert(-1, load)
                targets.insert(-1, len(slots))
                break
    assert [len(load_pairs(base, amp, ld)) for ld in loads] == targets
    return loads, targets


# ---------------------------------------------------------------------------------------------------------------
# a: lanes and waves
# ---------------------------------------------------------------------------------------------------------------
def _config(fc, which):
    """(planted set, base, amplifier, side): X streamed against Y for both sides, and Y streamed against X."""
    return {"x*y right": (fc["xy"], fc["x"], fc["y"], RIGHT),   # x + y
            "x*y left": (fc["yx"], fc["x"], fc["y"], LEFT),     # y + x
            "y*x right": (fc["yx"], fc["y"], fc["x"], RIGHT)}[which]  # y + x, the wide amplifier


def _checked_loads(base, amp):
    loads, targets = combi_loads(base, amp)
    if len(amp) == 19:
        assert targets == [1, 63, 64, 65, 255, 257, 653], targets
        assert any(ld[3] in (1, 3, 5) for ld in loads) and any(ld[2] > 0 for ld in loads)
    else:
        assert targets == [1, 63, 64, 65, 255, 257, 108, 653], targets  # 108: the one more load
        assert any(64 <= ld[3] < len(amp) and ld[3] % 64 for ld in loads)
    assert len(base[loads[0][0]]) > 63  # the 1-load starts at a base word that keeps nothing
    assert any(ld[1] * ld[3] > 256 and len(load_pairs(base, amp, ld)) < 256 for ld in loads)
    return loads


@pytest.mark.parametrize("which", ["x*y right", "x*y left", "y*x right"])
def test_lanes_and_waves_per_group(fc, sizes, which):
    """a. pbkdf2(g) / verify(g) on one ESSID: both sides with X as the base, and Y as the base of the 68-word X."""
    f, base, amp, side = _config(fc, which)
    lines, recs = f["lines"][:653], f["recs"][:653]
    recall(lines, recs, base, amp, side, _checked_loads(base, amp), sizes["one"]["p"], "per_group",
           R.expected_kernel("one", "p"))


def test_lanes_and_waves_run(fc, sizes):
    """a. The same loads through run() over three ESSIDs, one of them 52 bytes long (amplifier right)."""
    f, base, amp, side = _config(fc, "x*y right")
    recall(f["lines"], f["recs"], base, amp, side, _checked_loads(base, amp), sizes["mg"]["p"], "run",
           R.expected_kernel("mg", "p"))


# ---------------------------------------------------------------------------------------------------------------
# b: wide ids
# ---------------------------------------------------------------------------------------------------------------
_B62 = b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz"


def _four(i, lead):
    """The i-th distinct 4-byte word of a list: a lead byte and three base-62 digits."""
    return bytes([lead[i // 62**3], _B62[i // 3844 % 62], _B62[i // 62 % 62], _B62[i % 62]])


@pytest.mark.parametrize("side", [RIGHT, LEFT])
def test_wide_ids(sizes, side):
    """b. Two lists of 70,000 distinct 4-byte words and one load of a single base word x 100 amplifier words whose ids
    run across 2^32: 61,356 x 70,000 + 47,296 = 2^32."""
    n, fb, af, ac = 70_000, 61_356, 47_246, 100
    base, amp = [_four(i, b"ab") for i in range(n)], [_four(i, b"yz") for i in range(n)]
    assert len(set(base)) == n and len(set(amp)) == n
    assert fb * n + af < 2**32 <= fb * n + af + ac - 1 and fb * n + 47_296 == 2**32
    load = (fb, 1, af, ac)
    pairs = load_pairs(base, amp, load)
    assert len(pairs) == ac
    lines, recs = plant([join(base[b], amp[a], side) for b, a in pairs], ONE, 0xb0 + side)
    exp = expected(recs, base, amp, side, pairs)
    assert sorted(p[1] for p in exp) == list(range(2**32 - 50, 2**32 + 50))
    recall(lines, recs, base, amp, side, [load], sizes["one"]["p"], "per_group", R.expected_kernel("one", "p"))


# ---------------------------------------------------------------------------------------------------------------
# c: equal to the hybrid path and to the dictionary path
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side,mode", [(RIGHT, 6), (LEFT, 7)])
def test_equal_to_the_hybrid_path(sizes, side, mode):
    """c. One base word x the amplifier list 000..999 over a planted window of 100 gives the hits of set_mask(?d?d?d)
    + load_hybrid of the same word and window, ids included."""
    first, count, word = 345, 100, b"combi"
    amp = [b"%03d" % v for v in range(1000)]
    pairs = [(0, a) for a in range(first, first + count)]
    lines, recs = plant([join(word, amp[a], side) for b, a in pairs], ONE, 0xc0 + side)
    exp = expected(recs, [word], amp, side, pairs)
    db, da = Dictionary.from_words([word]), Dictionary.from_words(amp)
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(lines, nc=NC, batch=sizes["one"]["p"])
    try:
        sc.load_combinator(db.off.ptr, db.data.ptr, 0, 1, da.off.ptr, da.data.ptr, 1000, first, count, side)
        assert sc.loaded() == count
        R._scan_all(sc, "per_group")
        by_combi = R._hitset(sc.hits(cap=4096))
        assert sc.set_mask(b"?d?d?d") == 1000
        sc.load_hybrid(db.off.ptr, db.data.ptr, 0, 1, first, count, mode)
        assert sc.loaded() == count
        R._scan_all(sc, "per_group")
        by_hybrid = R._hitset(sc.hits(cap=4096))
    finally:
        sc.close()
    R._assert_same(by_combi, exp, "combinator")
    assert by_combi == by_hybrid
    assert L.pbkdf2_kernels() == {R.expected_kernel("one", "p")}


@pytest.mark.parametrize("side", [RIGHT, LEFT])
def test_equal_to_the_dictionary_path(sizes, side):
    """c. The list 00000..99999 as the base with a one-word amplifier gives load_dict's hits over the joined words:
    with A = 1 the id of a pair is its base index, which is the joined word's index."""
    first, count, amp = 12_345, 100, [b"one"]
    base = [b"%05d" % v for v in range(10**5)]
    joined = [join(w, amp[0], side) for w in base]
    pairs = [(b, 0) for b in range(first, first + count)]
    lines, recs = plant([joined[b] for b, a in pairs], ONE, 0xc8 + side)
    exp = expected(recs, base, amp, side, pairs)
    assert {p[1] for p in exp} == set(range(first, first + count))
    db, da, dj = Dictionary.from_words(base), Dictionary.from_words(amp), Dictionary.from_words(joined)
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(lines, nc=NC, batch=sizes["one"]["p"])
    try:
        sc.load_combinator(db.off.ptr, db.data.ptr, first, count, da.off.ptr, da.data.ptr, 1, 0, 1, side)
        assert sc.loaded() == count
        R._scan_all(sc, "per_group")
        by_combi = R._hitset(sc.hits(cap=4096))
        sc.load_dict(dj.off.ptr, dj.data.ptr, first, count)
        assert sc.loaded() == count
        R._scan_all(sc, "per_group")
        by_dict = R._hitset(sc.hits(cap=4096))
    finally:
        sc.close()
    R._assert_same(by_combi, exp, "combinator")
    assert by_combi == by_dict
    assert L.pbkdf2_kernels() == {R.expected_kernel("one", "p")}


# ---------------------------------------------------------------------------------------------------------------
# d: argument errors on a live scan
# ---------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_scan_usable(fc, sizes):
    f, base, amp, side = _config(fc, "x*y left")
    lines, recs = f["lines"], f["recs"]
    db, da = Dictionary.from_words(base), Dictionary.from_words(amp)
    nb, na = len(base), len(amp)
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(lines, nc=NC, batch=sizes["one"]["p"])

    def load(fb, n, words, af, ac, amp_side=side):
        sc.load_combinator(db.off.ptr, db.data.ptr, fb, n, da.off.ptr, da.data.ptr, words, af, ac, amp_side)

    def refused(*args, **kw):
        with pytest.raises(L.DwpaError) as e:
            load(*args, **kw)
        assert e.value.code == L.DWPA_E_ARG

    try:
        for bad in (2, 3, 6, 7, -1):
            refused(0, nb, na, 0, na, amp_side=bad)
        refused(0, sc.batch // na + 1, na, 0, na)  # nbase * amp_count > batch
        refused(0, sc.batch + 1, na, 0, 1)
        refused(0, 1, 2**40, 0, sc.batch + 1)
        refused(0, 2**32 - 1, na, 0, na)  # the product is beyond 32 bits
        refused(0, 2**16, 2**40, 0, 2**16)  # exactly 2^32
        refused(0, nb, na, 1, na)  # amp_first + amp_count > A
        refused(0, nb, na, na, 1)
        refused(0, nb, na, na + 1, 0)
        refused(0, nb, na, 2**64 - 1, 2)  # the sum wraps
        refused(0, nb, 0, 0, 1)  # A == 0 with amp_count > 0
        refused(2, 1, 10**19, 0, 1)  # (first_base + nbase) * A = 3 * 10^19 is beyond 64 bits
        refused(2**64 - 1, 1, na, 0, 1)  # first_base + nbase wraps
        rect = (3, nb - 3, 1, na - 2)
        pairs = load_pairs(base, amp, rect)
        load(rect[0], rect[1], na, rect[2], rect[3])
        assert sc.loaded() == len(pairs) > 500
        R._scan_all(sc, "per_group")
        R._assert_same(R._hitset(sc.hits(cap=4096)), expected(recs, base, amp, side, pairs), "after the errors")
        load(0, nb, na, na, 0)  # an empty window is a load of nothing
        assert sc.loaded() == 0
        load(0, 0, na, 0, na)
        assert sc.loaded() == 0
        load(0, 0, 0, 0, 0)
        assert sc.loaded() == 0
    finally:
        sc.close()
    assert L.pbkdf2_kernels() == {R.expected_kernel("one", "p")}


# ---------------------------------------------------------------------------------------------------------------
# e: dwpa_crack_combinator
# ---------------------------------------------------------------------------------------------------------------
def _crack(tmp_path, lines, left, right, side, batch=512):
    hf, out = tmp_path / "h.hash", tmp_path / "o.key"
    hf.write_bytes(b"\n".join(lines) + b"\n")
    if out.exists():
        out.unlink()
    L.pbkdf2_kernels(reset=True)
    rc, st = dwpa_amd.crack_combinator(str(hf), str(left), str(right), side, NC, str(out), batch=batch)
    ran = L.pbkdf2_kernels()
    recs = out.read_bytes().split(b"\n") if out.exists() else [b""]
    assert recs.pop() == b"" and st == [L.DWPA_DICT_OK] * 2
    assert ran and ran <= R.MG_KERNELS, ran
    return rc, sorted(recs)


def _plain_file(path, words):
    path.write_bytes(b"".join(w + b"\n" for w in words))
    return path


def _gzip_file(path, words, hexed):
    """A .gz with CRLF endings in its first half and word number `hexed` as $HEX[]."""
    words = list(words)
    words[hexed] = b"$HEX[" + words[hexed].hex().encode() + b"]"
    half = len(words) // 2
    with gzip.open(path, "wb") as f:
        f.write(b"".join(w + b"\r\n" for w in words[:half]) + b"".join(w + b"\n" for w in words[half:]))
    return path


def _psks(recs):
    return [r[0] for r in recs]


def test_crack_combinator_amp_right(fc, tmp_path):
    """e1. X from a gzip left list (CRLF in half of it, one $HEX[] word) and Y from a plain right list, three ESSIDs:
    rc 0, every line once with its PSK."""
    left = _gzip_file(tmp_path / "x.txt.gz", fc["x"], next(i for i, w in enumerate(fc["x"]) if len(w) == 20))
    right = _plain_file(tmp_path / "y.txt", fc["y"])
    f = fc["xy"]
    rc, recs = _crack(tmp_path, f["lines"], left, right, RIGHT)
    assert rc == 0 and recs == sorted(R._records(f["lines"], _psks(f["recs"])))
    st = M.crack_stats()
    assert (st["hashes"], st["cracked"]) == (3 * 653, 3 * 653) and st["candidates"] <= 653


def test_crack_combinator_amp_left(fc, tmp_path):
    """e2. Amplifier left: Y (held) + X (streamed) from plain files, one ESSID."""
    left, right = _plain_file(tmp_path / "y.txt", fc["y"]), _plain_file(tmp_path / "x.txt", fc["x"])
    f = fc["yx"]
    rc, recs = _crack(tmp_path, f["lines"], left, right, LEFT)
    assert rc == 0 and recs == sorted(R._records(f["lines"], _psks(f["recs"])))


@pytest.mark.parametrize("side", [RIGHT, LEFT])
def test_crack_combinator_amplifier_wider_than_the_batch(tmp_path, side):
    """e3. The amplifier w0000..w0999 (1000 words of 5 bytes) at batch 64, the smallest a scan takes: 16 launches per
    kept base word, plants at amplifier indices 0, 63, 64 and 999 of the three kept base words among dropped ones.
    With one more line that no pair cracks the run is exhausted: rc 1, words = the lines read, candidates = the kept
    pairs counted here, one worker entry that agrees."""
    rng = random.Random(0xe3 + side)
    seen = set()
    base = [R._word(rng, n, False, seen) if n else b"" for n in (2, 5, 58, 17, 0, 60, 300)]
    amp = [b"w%04d" % v for v in range(1000)]
    kept_base = [b for b, w in enumerate(base) if keeps(w, amp[0])]
    assert [len(base[b]) for b in kept_base] == [5, 58, 17]
    pairs = [(b, a) for b in kept_base for a in (0, 63, 64, 999)]
    psks = [join(base[b], amp[a], side) for b, a in pairs]
    lines, recs = plant(psks, ONE, 0xe30 + side)
    assert len(lines) == 12
    fb, fa = _plain_file(tmp_path / "base.txt", base), _plain_file(tmp_path / "amp.txt", amp)
    left, right = (fb, fa) if side == RIGHT else (fa, fb)
    rc, out = _crack(tmp_path, lines, left, right, side, batch=64)
    assert rc == 0 and out == sorted(R._records(lines, _psks(recs)))
    outside = join(base[kept_base[0]], b"w12x4", side)
    extra = R._line(0, 0, "LE", outside, ONE[0], O.c_pbkdf2(outside, ONE[0]), rng)
    rc, out = _crack(tmp_path, lines + [extra], left, right, side, batch=64)
    assert rc == 1 and out == sorted(R._records(lines, _psks(recs)))
    kept = sum(keeps(b, a) for b in base for a in amp)
    assert kept == 3000
    st = M.crack_stats()
    assert (st["words"], st["candidates"], st["hashes"], st["cracked"]) == (len(base), kept, 13, 12)
    ws = M.crack_worker_stats()
    assert len(ws) == 1 and ws[0]["candidates"] == kept and ws[0]["words"] == len(base)


def test_crack_combinator_exhausted(fc, tmp_path):
    """e4. X x Y plus a line no pair cracks, at the library's default batch: rc 1, the other records present,
    candidates = the 653 kept pairs exactly, words = the 68 lines of the streamed list."""
    rng = random.Random(0xe4)
    left, right = _plain_file(tmp_path / "y.txt", fc["y"]), _plain_file(tmp_path / "x.txt", fc["x"])
    f = fc["yx"]
    outside = b"no-pair-gives-this"
    extra = R._line(0, 0, "LE", outside, ONE[0], O.c_pbkdf2(outside, ONE[0]), rng)
    rc, recs = _crack(tmp_path, f["lines"] + [extra], left, right, RIGHT, batch=0)
    assert rc == 1 and recs == sorted(R._records(f["lines"], _psks(f["recs"])))
    st = M.crack_stats()
    assert (st["words"], st["candidates"], st["cracked"]) == (len(fc["y"]), 653, 653)


_SHARDS_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import dwpa_amd
from dwpa_amd import m22000 as M
rc, st = dwpa_amd.crack_combinator(sys.argv[2], sys.argv[5], sys.argv[6], 0,
                                   nonce_error_corrections=int(sys.argv[4]), out_file=sys.argv[3], batch=64)
print(json.dumps({"rc": rc, "dict": st, "stats": M.crack_stats(), "workers": M.crack_worker_stats()}))
"""


def test_crack_combinator_two_workers(fc, tmp_path):
    """e5. X x Y with DWPA_CRACK_SHARDS_PER_DEVICE=2 (read per call; a child keeps this process's environment as it
    is): every line is cracked, each outfile record is written once, and the two workers' sums are the call's."""
    hf, out = tmp_path / "h.hash", tmp_path / "o.key"
    f = fc["xy"]
    hf.write_bytes(b"\n".join(f["lines"]) + b"\n")
    left = _gzip_file(tmp_path / "x.txt.gz", fc["x"], next(i for i, w in enumerate(fc["x"]) if len(w) == 20))
    right = _plain_file(tmp_path / "y.txt", fc["y"])
    env = dict(os.environ, DWPA_CRACK_SHARDS_PER_DEVICE="2")
    r = subprocess.run([sys.executable, "-c", _SHARDS_CHILD, ROOT, str(hf), str(out), str(NC), str(left), str(right)],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["rc"] == 0 and res["dict"] == [L.DWPA_DICT_OK] * 2
    recs = out.read_bytes().split(b"\n")
    assert recs.pop() == b"" and sorted(recs) == sorted(R._records(f["lines"], _psks(f["recs"])))
    assert len(res["workers"]) == 2 and len({w["device"] for w in res["workers"]}) == 1
    assert sum(w["candidates"] for w in res["workers"]) == res["stats"]["candidates"] <= 653
    assert sum(w["words"] for w in res["workers"]) == res["stats"]["words"] <= len(fc["x"])
    assert res["stats"]["cracked"] == 3 * 653
