"""Fixtures and a CPU model for the crack loop's load sizing (scan_shard / scan_shard_combi, csrc/crack.cpp).

dwpa_crack_files, dwpa_crack_hybrid and dwpa_crack_combinator size every device load from a running estimate of the
share of candidates that survive the 8..63 filter and the rules.  A load that keeps more than a batch is repeated
with fewer words, one that keeps nothing is skipped, and a hit's id is mapped back to its word after either.  A
mistake there loses candidates in silence, so the fixtures below swing the kept share far enough that the loop must
take those paths, and every kept candidate is the PSK of one PMKID line: a candidate that is dropped, counted twice or
mapped to the wrong word shows in the outfile or in dwpa_crack_stats.candidates.

simulate() restates the sizing loop in plain Python.  The library's item cuts depend on the reader's chunking, so the
model does not predict the library's counters; tests/test_fill_plan.py uses it to prove on the CPU that a fixture
reaches the overflow path for every plausible cut (item_cuts), and tests/test_gpu_fill_recall.py then asserts on the
GPU that the library did.  combi_loads() restates scan_shard_combi, which sizes from the lengths alone and has no
adaptive state: there the model is exact.
"""
import functools
import itertools
import random

from oracle import oracle as O
from oracle import rules as OR
from tests import synth as S

NC = 8
JUNK_LENGTHS = (0, 7, 64, 65, 300)  # outside the 8..63 filter
STRIDE = 16                         # every STRIDE-th line is also checked with the oracle's own derive
_AL = b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz"


# ---------------------------------------------------------------------------------------------------------------
# the sizing loop, restated
# ---------------------------------------------------------------------------------------------------------------
def simulate(kept_per_word, cap, nrules, item_sizes):
    """scan_shard's loop over items of item_sizes words (the last item takes what is left): kept_per_word[i] of word
    i's nrules candidates survive.  Returns (loads, overflowed, empty, candidates), or "E_OVERFLOW" where the loop
    gives up: one word whose candidates overflow the batch."""
    keep = 1.0
    loads = overflowed = empty = cands = 0
    pos = 0
    for size in item_sizes:
        b, e = pos, min(len(kept_per_word), pos + size)
        pos = e
        words, wb = e - b, 0
        while wb < words:
            want = (1.0 if keep >= 1.0 else 0.995) * cap / (nrules * keep)
            most = 16 * cap // nrules
            nw = max(1, min(int(want), most, words - wb))
            raw = sum(kept_per_word[b + wb:b + wb + nw])
            loads += 1
            seen = raw / (nw * nrules)
            if raw > cap:
                if nw == 1:
                    return "E_OVERFLOW"
                keep = max(seen, keep * 1.05)
                overflowed += 1
                continue
            if raw > 0:
                keep = min(1.0, max(0.01, seen))
            else:
                empty += 1
            wb += nw
            cands += raw
    assert pos >= len(kept_per_word), "the items do not cover the words"
    return loads, overflowed, empty, cands


def rule_window_loads(word_lengths, cap, nrules):
    """More rules than the batch: one word at a time over consecutive rule ranges of at most a batch; a word the rule
    engine refuses (0 or more than 256 bytes) costs no launch.  These loads are not sized: the hook does not count
    them."""
    return sum(-(-nrules // cap) for n in word_lengths if 1 <= n <= 256)


def item_cuts(nwords, cap, nr):
    """The plausible cuts of nwords into items at batch cap with nr candidates per word: the queue's doubling
    sequence from first_item to most_item (crack_impl), one whole item, and fixed items of 4 batches."""
    first, most = max(1, cap // nr // 16), max(1, 16 * cap // nr)
    doubling, size, covered = [], first, 0
    while covered < nwords:
        doubling.append(size)
        covered += size
        size = min(most, 2 * size)
    fixed = max(1, 4 * cap // nr)
    return {"doubling": doubling, "whole": [nwords], "fixed": [fixed] * -(-nwords // fixed)}


def combi_loads(base_lengths, amp_lengths, cap, item_sizes):
    """scan_shard_combi's loop for an amplifier of at most a batch, over items of item_sizes base words: [(first
    word, words, kept pairs)] of every load, a load that keeps nothing included.  A load never spans two items."""
    A = len(amp_lengths)
    assert 1 <= A <= cap

    def kept(L):
        return sum(1 for R in amp_lengths if L <= 63 and 8 <= L + R <= 63)

    most = 16 * cap // A
    out, pos = [], 0
    for size in item_sizes:
        wb, end = pos, min(len(base_lengths), pos + size)
        pos = end
        while wb < end:
            nw = k_sum = 0
            while wb + nw < end and nw < most:
                k = kept(base_lengths[wb + nw])
                if k_sum + k > cap:
                    break
                k_sum += k
                nw += 1
            assert nw >= 1
            out.append((wb, nw, k_sum))
            wb += nw
    assert pos >= len(base_lengths), "the items do not cover the words"
    return out


# ---------------------------------------------------------------------------------------------------------------
# plants
# ---------------------------------------------------------------------------------------------------------------
_PMK = {}  # (essid, psk) -> pmk: fixtures that share an ESSID and candidates derive them once


def _pmks(psks, essid):
    need = [p for p in dict.fromkeys(psks) if (essid, p) not in _PMK]
    if need:
        raw = O.c_pbkdf2_many(need, essid, threads=8)
        for i, p in enumerate(need):
            _PMK[(essid, p)] = raw[32 * i:32 * i + 32]
    return [_PMK[(essid, p)] for p in psks]


def plant_lines(psks, essid, seed):
    """One PMKID line per PSK, and a last line whose PSK is no candidate (the run is exhausted and walks every word).
    Every line is confirmed by the oracle with the PMK handed over, every STRIDE-th also with the oracle's derive."""
    assert len(set(psks)) == len(psks) and all(8 <= len(p) <= 63 for p in psks)
    rng = random.Random(seed)
    outside = b"no-candidate-" + essid[:16]
    assert outside not in set(psks)
    lines = []
    for k, (psk, pmk) in enumerate(zip(list(psks) + [outside], _pmks(list(psks) + [outside], essid))):
        line = S.pmkid_line(psk, essid, rng.randbytes(6), rng.randbytes(6), the_pmk=pmk)
        exp = O.c_check_key_m22000(line, [psk], pmk, NC)
        assert exp and exp[0] == psk and exp[3] == pmk, (k, exp)
        if k % STRIDE == 0:
            assert O.c_check_key_m22000(line, [psk], False, NC) == exp, k
        lines.append(line)
    assert len(set(lines)) == len(lines)
    return lines


def _word(rng, n, seen, alphabet=None):
    """A distinct word of n bytes (printable, or of `alphabet`) that the reader takes as it stands."""
    while True:
        w = bytes(rng.choice(alphabet) if alphabet else rng.randint(0x21, 0x7E) for _ in range(n))
        if w not in seen and not w.startswith(b"$HEX["):
            seen.add(w)
            return w


def _junk(rng, i, lengths=JUNK_LENGTHS):
    return bytes(rng.randint(0x21, 0x7E) for _ in range(lengths[i % len(lengths)]))


def _fixture(name, essid, words, kept_per_word, psks, seed, **more):
    f = {"name": name, "essid": essid, "words": words, "kept_per_word": kept_per_word,
         "candidates": sum(kept_per_word), "psk": list(psks), "lines": plant_lines(psks, essid, seed)}
    f.update(more)
    return f


# ---------------------------------------------------------------------------------------------------------------
# the fixtures
# ---------------------------------------------------------------------------------------------------------------
SWING_SEGMENTS = (("sparse", 1032), ("dense", 1000), ("sparse", 136), ("dense", 560), ("junk", 1032))


@functools.lru_cache(maxsize=None)
def swing():
    """The dictionary path: a kept share that swings between 1/8 and 1, and an all-junk tail."""
    rng = random.Random(0xf111)
    words, seen, segs = [], set(), []
    for kind, n in SWING_SEGMENTS:
        segs.append((kind, len(words), n))
        for i in range(n):
            if kind == "dense" or (kind == "sparse" and i % 8 == 3):
                words.append(_word(rng, rng.randint(8, 63), seen))
            else:
                words.append(_junk(rng, len(words)))
    kpw = [int(8 <= len(w) <= 63) for w in words]
    return _fixture("swing", b"fill-swing", words, kpw, [w for w in words if 8 <= len(w) <= 63], 0xa1, segments=segs)


@functools.lru_cache(maxsize=None)
def all_kept():
    """5 x 64 + 1 distinct words, nothing filtered: exactly one batch per load, which cannot overflow."""
    rng = random.Random(0xf112)
    seen = set()
    words = [_word(rng, 8 + i % 56, seen) for i in range(5 * 64 + 1)]
    return _fixture("all_kept", b"fill-all-kept", words, [1] * len(words), words, 0xa2)


RULES_SWING = [":", "l", "$1", "c $1 $2 $3", "d", "[ [ [", "!a $a", "$1 $2 $3 $4 $5 $6 $7 $8"]
RULES_SWING_RUNS = (("sparse", 300), ("dense", 40), ("sparse", 140), ("dense", 40), ("sparse", 140), ("dense", 40),
                    ("none", 140))


@functools.lru_cache(maxsize=None)
def rules_swing():
    """The rules path (DWPA_RULES_FULL): runs of words of which almost every (word, rule) result falls outside 8..63
    (3-, 4-, 66-byte words, and words the rule engine refuses), runs of which almost every result is kept (11..31
    bytes), and a tail that keeps nothing.  The plants are the distinct kept results of the rule oracle."""
    rng = random.Random(0xf113)
    low = b"abcdefghijklmnopqrstuvwxyz"
    words, seen = [], set()
    for kind, n in RULES_SWING_RUNS:
        for i in range(n):
            if kind == "dense":
                w = _word(rng, rng.randint(11, 31), seen, low)
                words.append(w[:1].upper() + w[1:] if i % 3 == 0 else w)  # mixed case: ':' and 'l' differ
            elif kind == "sparse":
                n_ = (0, 66, 300, 3, 0, 300, 4, 0)[i % 8]
                words.append(_word(rng, n_, seen, low) if n_ else b"")
            else:
                n_ = (0, 300, 70)[i % 3]
                words.append(_word(rng, n_, seen, low) if n_ else b"")
    ops = [OR.parse(r) for r in RULES_SWING]
    assert all(o is not None for o in ops)
    by_psk, kpw, outcomes = {}, [], set()
    for wi, w in enumerate(words):
        k = 0
        for ri, o in enumerate(ops):
            c = OR.apply(o, w)
            outcomes.add("reject" if c is None else "short" if len(c) < 8 else "long" if len(c) > 63 else "kept")
            if c is not None and 8 <= len(c) <= 63:
                by_psk.setdefault(c, []).append(wi * len(ops) + ri)
                k += 1
        kpw.append(k)
    psks = sorted(by_psk)
    return _fixture("rules_swing", b"fill-rules-swing", words, kpw, psks, 0xa3, rules=list(RULES_SWING),
                    by_psk=by_psk, outcomes=outcomes)


def join(word, amp, mode):
    return word + amp if mode == 6 else amp + word


HYBRID_NARROW_RUNS = (("sparse", 120), ("dense", 24), ("sparse", 120), ("dense", 16), ("none", 110))
HYBRID_DROPPED = (0, 1, 2, 3, 4, 5, 6, 63, 64, 300)


@functools.lru_cache(maxsize=None)
def hybrid_narrow():
    """Modes 6 and 7 with the mask ?d (K = 10): runs of words whose lengths the one-byte join drops (0..6, 63, 64,
    300; one word in eight of a sparse run is kept, so that the estimate follows the run down) alternate with runs
    whose lengths it keeps (7..62), and a tail that keeps nothing.  The plants are every kept word x every digit."""
    rng = random.Random(0xf114)
    words, seen = [], set()
    for kind, n in HYBRID_NARROW_RUNS:
        for i in range(n):
            if kind == "dense" or (kind == "sparse" and i % 8 == 5):
                words.append(_word(rng, (7, 62, 8, 33, 61, 20)[len(words) % 6], seen))
            else:
                words.append(_junk(rng, len(words), HYBRID_DROPPED))
    kpw = [10 * int(7 <= len(w) <= 62) for w in words]
    f = {"name": "hybrid_narrow", "mask": b"?d", "custom": (), "K": 10, "words": words, "kept_per_word": kpw,
         "candidates": sum(kpw)}
    for mode in (6, 7):
        psks = [join(w, b"%d" % d, mode) for w in words if 7 <= len(w) <= 62 for d in range(10)]
        f[mode] = {"psk": psks, "lines": plant_lines(psks, b"fill-hybrid-narrow", 0xa40 + mode)}
    return f


HYBRID_EDGE_MASKS = {64: (b"?1?1", (b"01234567",)), 65: (b"?1?2", (b"abcde", b"0123456789ABC"))}


def mask_candidates(mask, custom):
    """Every candidate of a mask of custom sets only, in the library's order (itertools.product: last position
    fastest)."""
    sets = [custom[int(mask[i + 1:i + 2]) - 1] for i in range(0, len(mask), 2)]
    assert all(mask[i:i + 1] == b"?" for i in range(0, len(mask), 2))
    return [bytes(t) for t in itertools.product(*sets)]


@functools.lru_cache(maxsize=None)
def hybrid_edge(K):
    """A mask of exactly a batch (K = 64: the sizing loop, one word per load) and of one more (K = 65: one word x mask
    ranges) at batch 64: three kept words among dropped ones, plants at mask indices 0, 63 and K - 1."""
    mask, custom = HYBRID_EDGE_MASKS[K]
    cands = mask_candidates(mask, custom)
    assert len(cands) == K and len(set(cands)) == K
    rng = random.Random(0xf115 + K)
    seen = set()
    words = [_word(rng, n, seen) if n else b"" for n in (3, 62, 6, 0, 300, 30, 5, 64, 61, 63, 2)]
    kept = [i for i, w in enumerate(words) if 6 <= len(w) <= 61]
    assert [len(words[i]) for i in kept] == [6, 30, 61]
    kpw = [K * int(6 <= len(w) <= 61) for w in words]
    f = {"name": "hybrid_edge", "mask": mask, "custom": custom, "K": K, "words": words, "kept_per_word": kpw,
         "candidates": sum(kpw)}
    for mode in (6, 7):
        psks = [join(words[i], cands[j], mode) for i in kept for j in sorted({0, 63, K - 1})]
        f[mode] = {"psk": psks, "lines": plant_lines(psks, b"fill-hybrid-edge", 0xa50 + mode)}
    return f


# base words by item of the queue's doubling cut (1, 2, 4, 8, 16, 16 words: a load never spans two items)
COMBI_BASE_LENGTHS = ((70,) + (2, 56) + (62, 2, 56, 62) + (4, 62, 62, 62, 2, 56, 62, 4) + (70,) * 16 +
                      (2, 56, 2, 4, 60, 62, 56))


@functools.lru_cache(maxsize=None)
def combi_edge(A, side):
    """The combinator loop at batch 64 with an amplifier of exactly a batch (A = 64) and of one less (A = 63): the
    amplifier holds one word of 1 byte, 31 of 4 bytes and the rest of 8 bytes, so a base word of 2, 56, 62, 4 bytes
    keeps A - 32, 32, 1, A pairs and one of 60 or 70 bytes none.  side 0: the right list is the amplifier (PSK =
    base + amplifier word); side 1: the left list is (PSK = amplifier word + base).  Plants: every kept pair."""
    assert A in (63, 64) and side in (0, 1)
    rng = random.Random(0xf116)  # the 63-word amplifier is the 64-word one without its last word
    low, up = b"abcdefghijklmnopqrstuvwxyz", b"ABCDEFGHIJKLMNOPQRSTUVWXYZ"
    seen = set()
    amp = [_word(rng, n, seen, low) for n in (1,) + (4,) * 31 + (8,) * 32][:A]
    base = [_word(rng, n, seen, up) for n in COMBI_BASE_LENGTHS]
    kpw = [sum(1 for a in amp if len(b) <= 63 and 8 <= len(b) + len(a) <= 63) for b in base]
    psks = [(a + b if side else b + a) for b in base for a in amp if len(b) <= 63 and 8 <= len(a) + len(b) <= 63]
    assert len(psks) == sum(kpw)
    return _fixture("combi_edge", b"fill-combi-edge", base, kpw, psks, 0xa60 + side, amp=amp, side=side,
                    loads=combi_loads([len(b) for b in base], [len(a) for a in amp], 64,
                                      item_cuts(len(base), 64, A)["doubling"]))


def wide_rule(r):
    """Rule r of the wide rule files: 62 one-character appends, 62 inserts at position 1, then two-character appends:
    all parse, and all give distinct results for one word."""
    if r < 62:
        return "$%c" % _AL[r]
    if r < 124:
        return "i1%c" % _AL[r - 62]
    r -= 124
    return "$%c $%c" % (_AL[r // 62], _AL[r % 62])


RULES_WIDE_WORDS = (b"widerule", b"wide-rule-1", b"Wide.Rule.Two", b"wide_rule_three_", b"WIDE rule 4 of 20bytes"[:20],
                    b"the-last-wide-word")


@functools.lru_cache(maxsize=None)
def rules_wide(nrules):
    """Rule files of exactly a batch of rules, one more, and 16 batches + 1 at batch 64, over six words of 8..20
    bytes: every result is kept.  Plants: every (word, rule) of the first and the last word, and rules 0, 63, 64 and
    nrules - 1 of the others."""
    rules = [wide_rule(r) for r in range(nrules)]
    ops = [OR.parse(r) for r in rules]
    assert all(o is not None for o in ops) and len(set(rules)) == nrules
    words = list(RULES_WIDE_WORDS)
    assert len(words) == 6 and all(8 <= len(w) <= 20 for w in words)
    plants = {}
    for wi, w in enumerate(words):
        every = wi in (0, len(words) - 1)
        res = [OR.apply(o, w) for o in ops]
        assert all(c is not None and 8 <= len(c) <= 63 for c in res) and len(set(res)) == nrules
        for ri in range(nrules) if every else sorted({0, 63, 64, nrules - 1} & set(range(nrules))):
            assert res[ri] not in plants
            plants[res[ri]] = wi * nrules + ri
    return _fixture("rules_wide", b"fill-rules-wide", words, [nrules] * len(words), list(plants), 0xa7, rules=rules,
                    plants=plants)
