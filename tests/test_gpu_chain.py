"""GPU recall of the chain attack: k_prep_chain through the scan API (set_chain / load_chain) and dwpa_crack_chain.

The all-plants method of tests/test_gpu_recall.py and tests/test_gpu_combinator.py: EVERY kept candidate of a load is
the PSK of one line per ESSID, the expected set is restated here in Python (mixed-radix order, join, filter, id), and
the hits must equal it -- none missing, none extra, none twice, ids and PMKs equal -- while loaded() must equal the
kept count.  Batch sizes follow from the device's CU count as in test_gpu_recall, and every scan test asserts which
PBKDF2 kernel ran.

A chain is written here as a list of parts: a list of words, or a mask as bytes.  A load is a window (first, count)
of raw indices; candidate i is element i of itertools.product over the parts (restated in Chain below).
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
from dwpa_amd.device import Dictionary  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import test_gpu_combinator as C  # noqa: E402
from tests import test_gpu_recall as R  # noqa: E402
from tests.test_gpu_recall import sizes  # noqa: E402,F401  (the fixture)
from tests.test_mask import ref_candidate, ref_sets  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC = R.NC
ONE = (b"chain-recall",)
CUSTOM = (b"ab", b"cde")
M6 = b"?1?2"       # K = 6, 2 positions
ML = b"?1-?2"      # a literal and two custom sets: K = 6, 3 positions


# ---------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------
class Chain:
    """The parts of a chain with their radices; candidate(i) = (bytes, kept) by the rules restated here."""

    def __init__(self, parts, custom=CUSTOM):
        self.parts, self.custom = parts, custom
        self.sets = [None if isinstance(p, list) else ref_sets(p, custom) for p in parts]
        self.radix = [len(p) if s is None else s[1] for p, s in zip(parts, self.sets)]
        self.k = 1
        for r in self.radix:
            self.k *= r

    def digits(self, i):
        out = []
        for r in reversed(self.radix):
            i, d = divmod(i, r)
            out.append(d)
        assert i == 0
        return out[::-1]

    def pieces(self, i):
        return [p[d] if s is None else ref_candidate(s[0], d) for p, s, d in zip(self.parts, self.sets, self.digits(i))]

    def candidate(self, i, minlen=8, maxlen=63):
        ps = self.pieces(i)
        psk = b"".join(ps)
        keep = all(len(x) <= 63 for x, s in zip(ps, self.sets) if s is None) and minlen <= len(psk) <= maxlen
        return psk, keep

    def kept(self, first, count):
        """[(id, psk)] of the kept candidates of a window, in slot order: the compaction keeps index order."""
        out = []
        for i in range(first, first + count):
            psk, keep = self.candidate(i)
            if keep:
                out.append((i, psk))
        return out


class Device:
    """The lists of a chain in HBM and the parts as Scan.set_chain takes them."""

    def __init__(self, chain):
        self.dicts = [Dictionary.from_words(p) if isinstance(p, list) else None for p in chain.parts]
        self.parts = [(L.DWPA_CHAIN_MASK, p) if d is None else (L.DWPA_CHAIN_LIST, d.off.ptr, d.data.ptr, len(p))
                      for p, d in zip(chain.parts, self.dicts)]


def plant(kept, essids, seed):
    """One line per (essid, kept candidate).  Returns (lines, expected hits {(line, id, nc, endian, pmk)}, the PSK of
    each line).  C.plant asserts that no two ids give one string or one HMAC key."""
    lines, recs = C.plant([psk for i, psk in kept], essids, seed)
    ids = {psk: i for i, psk in kept}
    exp = {(ln, ids[psk], nc, en, pmk) for ln, (psk, nc, en, pmk) in enumerate(recs)}
    return lines, exp, [r[0] for r in recs]


def recall(lines, exp, chain, loads, batch, how, kernel):
    """set_chain once, then every load: loaded() == the kept count and the hits are exactly the load's plants."""
    dev = Device(chain)
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(lines, nc=NC, batch=batch)
    held = set()
    try:
        assert sc.set_chain(dev.parts, chain.custom) == chain.k
        for first, count in loads:
            ids = [i for i, psk in chain.kept(first, count)]
            slots = set(enumerate(ids))
            assert not slots & held, "a slot would hold a candidate it held before"
            held |= slots
            sc.load_chain(first, count)
            assert sc.loaded() == len(ids), (first, count)
            R._scan_all(sc, how)
            R._assert_same(R._hitset(sc.hits(cap=8192)), {p for p in exp if p[1] in set(ids)}, (how, first, count))
    finally:
        sc.close()
    assert L.pbkdf2_kernels() == {kernel}


# ---------------------------------------------------------------------------------------------------------------
# 1: equal to the merged paths
# ---------------------------------------------------------------------------------------------------------------
def _hits_of(sc, load, count):
    load()
    assert sc.loaded() == count
    R._scan_all(sc, "per_group")
    return R._hitset(sc.hits(cap=8192))


def test_equal_to_the_combinator_path(sizes):
    """1. [X, Y] over the whole key space gives load_combinator's loaded(), ids and hits (amplifier right) over the
    whole rectangle: 1292 raw pairs, 653 kept."""
    xs, ys = C._build_lists()
    ch = Chain([xs, ys])
    kept = ch.kept(0, ch.k)
    assert ch.k == 1292 and len(kept) == 653
    assert [i for i, p in kept] == [b * len(ys) + a for b, a in C.load_pairs(xs, ys, (0, len(xs), 0, len(ys)))]
    lines, exp, _ = plant(kept, ONE, 0x1c)
    dev = Device(ch)
    dx, dy = dev.dicts
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(lines, nc=NC, batch=sizes["one"]["p"])
    try:
        assert sc.set_chain(dev.parts) == ch.k
        by_chain = _hits_of(sc, lambda: sc.load_chain(0, ch.k), len(kept))
        by_combi = _hits_of(sc, lambda: sc.load_combinator(dx.off.ptr, dx.data.ptr, 0, len(xs), dy.off.ptr,
                                                           dy.data.ptr, len(ys), 0, len(ys), C.RIGHT), len(kept))
    finally:
        sc.close()
    R._assert_same(by_chain, exp, "chain")
    assert by_chain == by_combi
    assert L.pbkdf2_kernels() == {R.expected_kernel("one", "p")}


@pytest.mark.parametrize("mode", [6, 7])
def test_equal_to_the_hybrid_path(sizes, mode):
    """1. [X, M] gives load_hybrid mode 6 and [M, X] mode 7, M a 2-position mask of 6 candidates.  In mode 7 the chain's
    id is mask index * N + word index where the hybrid's is word index * K + mask index: the hits are compared after
    that renaming, and the slot order differs with it."""
    xs, _ = C._build_lists()
    ch = Chain([xs, M6] if mode == 6 else [M6, xs])
    kept = ch.kept(0, ch.k)
    assert ch.k == 408 and len(kept) == 6 * 56
    lines, exp, _ = plant(kept, ONE, 0x16 + mode)
    dev = Device(ch)
    dx = dev.dicts[0 if mode == 6 else 1]
    n = len(xs)
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(lines, nc=NC, batch=sizes["one"]["p"])
    try:
        assert sc.set_chain(dev.parts, CUSTOM) == ch.k
        assert sc.set_mask(M6, CUSTOM) == 6  # a scan holds both
        by_chain = _hits_of(sc, lambda: sc.load_chain(0, ch.k), len(kept))
        by_hybrid = _hits_of(sc, lambda: sc.load_hybrid(dx.off.ptr, dx.data.ptr, 0, n, 0, 6, mode), len(kept))
        again = _hits_of(sc, lambda: sc.load_chain(0, ch.k), len(kept))  # set_mask left the chain alone
    finally:
        sc.close()
    R._assert_same(by_chain, exp, "chain")
    if mode == 7:
        by_hybrid = {(ln, (i % 6) * n + i // 6, nc, en, pmk) for ln, i, nc, en, pmk in by_hybrid}
    assert by_chain == by_hybrid == again
    assert L.pbkdf2_kernels() == {R.expected_kernel("one", "p")}


def test_equal_to_the_mask_path(sizes):
    """1. [M] gives load_mask's hits over a window and over the whole key space."""
    mask = b"chain-?d?1?2"
    ch = Chain([mask])
    kept = ch.kept(0, ch.k)
    assert ch.k == 60 == len(kept)
    lines, exp, _ = plant(kept, ONE, 0x13)
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(lines, nc=NC, batch=sizes["one"]["p"])
    try:
        assert sc.set_chain([(L.DWPA_CHAIN_MASK, mask)], CUSTOM) == 60
        assert sc.set_mask(mask, CUSTOM) == 60
        for first, count in ((0, 60), (7, 41), (59, 1)):
            by_chain = _hits_of(sc, lambda: sc.load_chain(first, count), count)
            by_mask = _hits_of(sc, lambda: sc.load_mask(first, count), count)
            R._assert_same(by_chain, {p for p in exp if first <= p[1] < first + count}, (first, count))
            assert by_chain == by_mask
    finally:
        sc.close()
    assert L.pbkdf2_kernels() == {R.expected_kernel("one", "p")}


# ---------------------------------------------------------------------------------------------------------------
# 2 and 3: three and four parts, carries
# ---------------------------------------------------------------------------------------------------------------
A_LENGTHS = (64, 5, 0, 14, 300, 7, 63, 28, 9, 300)  # never-kept words first, inside and last; an empty word; 63 bytes
B_LENGTHS = (300, 3, 10, 64, 32, 0, 4, 33, 64)
C_LENGTHS = (6, 64, 0, 19, 1, 300)
D_LENGTHS = (2, 300, 11, 0, 9)


def _lists():
    rng = random.Random(0x4348)
    seen = set()
    return [[R._word(rng, n, i % 4 == 1, seen) if n else b"" for i, n in enumerate(lens)]
            for lens in (A_LENGTHS, B_LENGTHS, C_LENGTHS, D_LENGTHS)]


SHAPES = ("ABM", "MAB", "AMBC", "ABCD", "A1mB")


def _shape(lists, name):
    a, b, c, d = lists
    part = {"A": a, "B": b, "C": c, "D": d, "M": ML, "1": [b"only"], "m": b"=="}  # 1, m: parts of radix 1
    return Chain([part[ch] for ch in name])


@pytest.fixture(scope="module")
def fx():
    """Every kept candidate of five chains planted under one ESSID, and those of [A, B, M] under the three ESSIDs of
    test_gpu_recall too (one of 52 bytes)."""
    lists = _lists()
    for lens, ws in zip((A_LENGTHS, B_LENGTHS, C_LENGTHS, D_LENGTHS), lists):
        assert [len(w) for w in ws] == list(lens)
        dead = [i for i, w in enumerate(ws) if len(w) > 63]
        assert dead and b"" in ws and not any(b"\n" in w or b"\r" in w for w in ws)
    for ws in lists[:2]:  # never-kept words first, inside and last
        dead = [i for i, w in enumerate(ws) if len(w) > 63]
        assert dead[0] == 0 and dead[-1] == len(ws) - 1 and len(dead) >= 3
    assert {64, 300, 63, 0} <= set(A_LENGTHS) and {64, 300, 0} <= set(B_LENGTHS)
    assert any(any(c >= 0x80 for c in w) for ws in lists for w in ws)
    out = {"lists": lists}
    for k, name in enumerate(SHAPES):
        ch = _shape(lists, name)
        kept = ch.kept(0, ch.k)
        assert ch.k <= 4000 and 30 <= len(kept) <= 800, (name, ch.k, len(kept))
        ids = [i for i, p in kept]
        assert ids != list(range(ids[0], ids[0] + len(ids)))  # slots move: ids[] must carry the id
        if name != "A1mB":
            # among the kept candidates every part after the first stands at every (length % 4, byte offset % 4) that
            # the parts allow: all 16 for a list behind a list (a mask's length is fixed, and so is the offset behind a
            # leading mask), and every list has words of all four lengths % 4
            short = [[len(s[0])] if s is not None else [len(w) for w in part if len(w) <= 63]
                     for part, s in zip(ch.parts, ch.sets)]  # the lengths a kept candidate can hold at each part
            full = 0
            for p in range(1, len(ch.parts)):
                pairs = set()
                for i in ids:
                    ps = ch.pieces(i)
                    pairs.add((len(ps[p]) % 4, sum(len(x) for x in ps[:p]) % 4))
                offs = {0}
                for q in range(p):
                    offs = {(o + n) % 4 for o in offs for n in short[q]}
                assert pairs == {(n % 4, o) for n in short[p] for o in offs}, (name, p, sorted(pairs))
                assert ch.sets[p] is not None or len({n % 4 for n in short[p]}) == 4
                full += len(pairs) == 16
            assert full >= 1
        # total lengths at both ends of the filter, and candidates just outside it
        totals = {len(b"".join(ch.pieces(i))) for i in range(ch.k)}
        assert ({8, 63} <= {len(p) for i, p in kept} and {7, 64} <= totals) or name == "A1mB"
        lines, exp, psks = plant(kept, ONE, 0x20 + k)
        out[name] = {"chain": ch, "kept": kept, "lines": lines, "exp": exp, "psk": psks}
    ch = out["ABM"]["chain"]
    lines, exp, psks = plant(out["ABM"]["kept"], R.ESSIDS, 0x2f)
    out["ABM3"] = {"chain": ch, "kept": out["ABM"]["kept"], "lines": lines, "exp": exp, "psk": psks}
    return out


@pytest.mark.parametrize("name", SHAPES)
def test_whole_key_space(fx, sizes, name):
    """2. Three and four parts (and two parts of radix 1): the whole key space in one load."""
    f = fx[name]
    recall(f["lines"], f["exp"], f["chain"], [(0, f["chain"].k)], sizes["one"]["p"], "per_group",
           R.expected_kernel("one", "p"))


def _carry_loads(ch):
    """3. Windows that start mid-key-space.  With s[p] the stride of part p (the product of the radices behind it), a
    window that crosses a multiple of s[p] wraps every part behind p and carries into p.  Each window is wanted as
    (the multiple it crosses, its count); where it starts is the first choice under which no slot holds a candidate
    that it held in an earlier load, so that a slot left unwritten cannot pass for a found plant."""
    stride = [1] * len(ch.radix)
    for p in range(len(ch.radix) - 2, -1, -1):
        stride[p] = stride[p + 1] * ch.radix[p + 1]
    k, s0 = ch.k, stride[0]
    big = k >= 400  # A1mB has 90 candidates: the same crossings in windows that fit
    want = [(k, 300 if big else k - 1),         # no multiple of 256, ending at K
            (stride[-2], 3),                    # a wrap of the last part
            (2 * stride[-3], 5),                # of the last two
            (3 * s0 if big else 5 * s0, 63),    # of every part up to the first
            (5 * s0 if big else 6 * s0, 65), (k // 2 // s0 * s0, 259 if big else 20),
            (s0, 1), (s0 + 1, 1),               # one candidate: the last before a carry into the first, the first after
            (k, 1)]
    loads, held = [], set()
    for at, count in want:
        for back in ([count] if at == k or count == 1 else range(count // 2 + 1, count)):
            first = at - back
            if first <= 0 or first + count > k:
                continue
            slots = set(enumerate(i for i, psk in ch.kept(first, count)))
            if not slots & held:
                break
        else:
            raise AssertionError("no window of %d across %d keeps its slots apart" % (count, at))
        held |= slots
        loads.append((first, count))
    return loads


@pytest.mark.parametrize("name", SHAPES)
def test_carries(fx, sizes, name):
    """3. ABM: the mask wraps into a list; MAB and AMBC: a list wraps into the mask; A1mB: parts of radix 1 pass the
    carry on."""
    f = fx[name]
    ch = f["chain"]
    loads = _carry_loads(ch)
    assert {c for f_, c in loads} >= ({1, 63, 65, 300, 259} if ch.k >= 400 else {1, 63, 65})
    assert any(f_ + c == ch.k for f_, c in loads)
    crossed = set()  # the parts whose digit changes inside some window
    for first, count in loads:
        a, b = ch.digits(first), ch.digits(first + count - 1)
        crossed |= {p for p in range(len(a)) if a[p] != b[p]}
    assert crossed == {p for p, r in enumerate(ch.radix) if r > 1}
    # the slots of two loads may hold the same candidate only by accident of the windows: none does
    recall(f["lines"], f["exp"], ch, loads, sizes["one"]["p"], "per_group", R.expected_kernel("one", "p"))


def test_run_over_three_essids(fx, sizes):
    """2, 3. [A, B, M] through run() over three ESSIDs, one of them 52 bytes long: the whole key space and a window."""
    f = fx["ABM3"]
    ch = f["chain"]
    recall(f["lines"], f["exp"], ch, [(0, ch.k), (ch.k // 3 + 1, 200)], sizes["mg"]["p"], "run",
           R.expected_kernel("mg", "p"))


# ---------------------------------------------------------------------------------------------------------------
# 4: 64-bit ids
# ---------------------------------------------------------------------------------------------------------------
def test_wide_ids(sizes):
    """4. [3 words, ?d x 10]: K = 3 * 10^10, the mask part's own keyspace is above 2^32.  Windows across 2^32, across
    a word boundary (10^10) and ending at K."""
    words = [b"w0-", b"", b"third-word:"]
    ch = Chain([words, b"?d" * 10])
    assert ch.k == 3 * 10**10 and ch.radix[1] > 2**32
    loads = [(2**32 - 100, 200), (10**10 - 77, 200), (2 * 10**10 - 1, 2), (ch.k - 150, 150)]
    kept = [c for first, count in loads for c in ch.kept(first, count)]
    assert len(kept) == 552 and all(len(p) >= 10 for i, p in kept)
    assert kept[0] == (2**32 - 100, b"w0-%010d" % (2**32 - 100)) and kept[-1] == (ch.k - 1, b"third-word:9999999999")
    assert (10**10 - 1, b"w0-9999999999") in kept and (10**10, b"0000000000") in kept
    lines, exp, _ = plant(kept, ONE, 0x40)
    assert {p[1] for p in exp} == {i for first, count in loads for i in range(first, first + count)}
    recall(lines, exp, ch, loads, sizes["one"]["p"], "per_group", R.expected_kernel("one", "p"))


# ---------------------------------------------------------------------------------------------------------------
# argument errors on a live scan
# ---------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_scan_usable(fx, sizes):
    f = fx["ABM"]
    ch = f["chain"]
    dev = Device(ch)
    la, lb, m = dev.parts
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(f["lines"], nc=NC, batch=sizes["one"]["p"])

    def refused(call):
        with pytest.raises(L.DwpaError) as e:
            call()
        assert e.value.code == L.DWPA_E_ARG

    try:
        refused(lambda: sc.load_chain(0, 1))  # no chain set
        assert sc.set_chain(dev.parts, CUSTOM) == ch.k
        refused(lambda: sc.set_chain([], CUSTOM))
        refused(lambda: sc.set_chain([la, lb, m, la, lb], CUSTOM))
        refused(lambda: sc.set_chain([la, (7,) + lb[1:]], CUSTOM))                    # an unknown kind
        refused(lambda: sc.set_chain([la, (L.DWPA_CHAIN_MASK, b"?x")], CUSTOM))       # a bad mask
        refused(lambda: sc.set_chain([la, m], ()))                                    # ?1 is not defined
        refused(lambda: sc.set_chain([(L.DWPA_CHAIN_LIST, la[1], la[2], 2**32), m], CUSTOM))
        refused(lambda: sc.set_chain([(L.DWPA_CHAIN_MASK, b"?b?b?b?b")] * 2, CUSTOM))  # 2^64
        refused(lambda: sc.set_chain([(L.DWPA_CHAIN_LIST, la[1], la[2], 2**32 - 1)] * 2 + [m], CUSTOM))
        refused(lambda: sc.load_chain(0, sc.batch + 1))
        refused(lambda: sc.load_chain(ch.k, 1))
        refused(lambda: sc.load_chain(ch.k - 1, 2))
        refused(lambda: sc.load_chain(ch.k + 1, 0))
        refused(lambda: sc.load_chain(2**64 - 1, 2))  # the sum wraps
        # the chain set before the refusals is still the scan's
        kept = ch.kept(3, ch.k - 3)
        sc.load_chain(3, ch.k - 3)
        assert sc.loaded() == len(kept) > 100
        R._scan_all(sc, "per_group")
        R._assert_same(R._hitset(sc.hits(cap=8192)), {p for p in f["exp"] if p[1] >= 3}, "after the errors")
        sc.load_chain(ch.k, 0)  # an empty window is a load of nothing
        assert sc.loaded() == 0
        sc.load_chain(5, 0)
        assert sc.loaded() == 0
        # a part of no words: K = 0, which takes no load but the empty one
        empty = Dictionary.from_words([])
        assert sc.set_chain([la, (L.DWPA_CHAIN_LIST, empty.off.ptr, empty.data.ptr, 0), m], CUSTOM) == 0
        sc.load_chain(0, 0)
        assert sc.loaded() == 0
        refused(lambda: sc.load_chain(0, 1))
    finally:
        sc.close()


# ---------------------------------------------------------------------------------------------------------------
# 5: dwpa_crack_chain
# ---------------------------------------------------------------------------------------------------------------
_CRACK_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import dwpa_amd
from dwpa_amd import m22000 as M
job = json.load(open(sys.argv[2]))
res = []
for run in job["runs"]:
    rc, st = dwpa_amd.crack_chain(run["hash"], [tuple(p) for p in job["parts"]] if "parts" not in run else
                                  [tuple(p) for p in run["parts"]], job["custom"], run.get("skip", 0),
                                  run.get("limit", 0), job["nc"], run["out"], batch=64)
    res.append({"rc": rc, "status": st, "stats": M.crack_stats(), "workers": M.crack_worker_stats()})
print(json.dumps(res))
"""


def test_crack_chain(tmp_path):
    """5. A small [A, B, M] at batch 64 with two workers on one device (DWPA_CRACK_SHARDS_PER_DEVICE is read per
    call; a child keeps this process's environment as it is): plants at index 0, at K - 1 and on both sides of a batch
    boundary.  The whole key space: rc 0 and every record once.  A window that leaves out the plant at index 0: rc 1,
    that line stays uncracked, candidates = the kept candidates of the window.  An unreadable list: part_status."""
    a = [b"first", b"L" * 64, b"", b"x" * 300, b"last5"]
    b = [b"-one", b"-twoo", b"", b"-four4"]
    ch = Chain([a, b, b"?d?1"])
    assert ch.k == 400
    kept = dict(ch.kept(0, ch.k))
    planted = sorted({0, 63, 64, 65, min(i for i in kept if i >= 160), max(i for i in kept if i < 256), ch.k - 1})
    assert all(i in kept for i in planted) and len(planted) == 7 and 100 < len(kept) < 400
    lines, exp, psks = plant([(i, kept[i]) for i in planted], ONE, 0x50)
    rng = random.Random(0x51)
    outside = b"no-chain-gives-this"
    extra = R._line(0, 0, "LE", outside, ONE[0], O.c_pbkdf2(outside, ONE[0]), rng)
    pa = tmp_path / "a.txt.gz"
    with gzip.open(pa, "wb") as f:  # CRLF, an empty line inside, the last word as $HEX[]
        f.write(b"".join((w if w != a[-1] else b"$HEX[" + w.hex().encode() + b"]") + b"\r\n" for w in a))
    pb = tmp_path / "b.txt"
    pb.write_bytes(b"\n".join(b))  # an empty line inside, no newline after the last word
    h_all, h_extra = tmp_path / "all.hash", tmp_path / "extra.hash"
    h_all.write_bytes(b"\n".join(lines) + b"\n")
    h_extra.write_bytes(b"\n".join(lines + [extra]) + b"\n")
    outs = [str(tmp_path / ("o%d.key" % i)) for i in range(4)]
    parts = [(L.DWPA_CHAIN_LIST, str(pa)), (L.DWPA_CHAIN_LIST, str(pb)), (L.DWPA_CHAIN_MASK, "?d?1")]
    bad = [(L.DWPA_CHAIN_LIST, str(pa)), (L.DWPA_CHAIN_LIST, str(tmp_path / "missing.txt")), (L.DWPA_CHAIN_MASK, "?d?1")]
    job = {"parts": parts, "custom": ["ab"], "nc": NC,
           "runs": [{"hash": str(h_all), "out": outs[0]},
                    {"hash": str(h_all), "out": outs[1], "skip": 1, "limit": ch.k - 1},
                    {"hash": str(h_extra), "out": outs[2]},
                    {"hash": str(h_all), "out": outs[3], "parts": bad}]}
    jp = tmp_path / "job.json"
    jp.write_text(json.dumps(job))
    env = dict(os.environ, DWPA_CRACK_SHARDS_PER_DEVICE="2")
    r = subprocess.run([sys.executable, "-c", _CRACK_CHILD, ROOT, str(jp)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    whole, window, exhausted, unreadable = json.loads(r.stdout.strip().splitlines()[-1])

    def records(path):
        recs = open(path, "rb").read().split(b"\n")
        assert recs.pop() == b""
        return sorted(recs)

    every = sorted(R._records(lines, psks))
    assert whole["rc"] == 0 and whole["status"] == [L.DWPA_DICT_OK] * 3 and records(outs[0]) == every
    assert len(whole["workers"]) == 2 and len({w["device"] for w in whole["workers"]}) == 1
    assert sum(w["candidates"] for w in whole["workers"]) == whole["stats"]["candidates"] <= len(kept)
    assert whole["stats"]["words"] == len(a) + len(b) and whole["stats"]["cracked"] == len(planted)
    # the plant at index 0 is outside [1, K): its line stays uncracked
    first = R._records(lines, psks)[[p[1] for p in sorted(exp)].index(0)]
    assert window["rc"] == 1 and records(outs[1]) == sorted(set(every) - {first})
    assert window["stats"]["candidates"] == len(kept) - 1 and window["stats"]["cracked"] == len(planted) - 1
    # exhausted: every raw index was loaded once, the kept ones derived
    assert exhausted["rc"] == 1 and records(outs[2]) == every
    assert exhausted["stats"]["candidates"] == len(kept) and exhausted["stats"]["hashes"] == len(planted) + 1
    assert sum(w["items"] for w in exhausted["workers"]) == (ch.k + 63) // 64
    assert unreadable["rc"] == L.DWPA_RC_ERROR and unreadable["status"] == [L.DWPA_DICT_OK, L.DWPA_E_IO, L.DWPA_DICT_OK]
    assert not os.path.exists(outs[3])
