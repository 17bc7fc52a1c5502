"""The prepared-candidate differential's model (CPU, needs no GPU): what every candidate generator of the scan path
must leave in the batch -- the kept ids and, per id, the HMAC-SHA1 key midstates of the candidate's bytes.

  * midstates(keys): SHA-1's compression function from FIPS 180-4 in numpy, over a whole list of keys at once; the ten
    words per key in the device's order (ipad h0..h4, opad h0..h4).
  * One Attack per generator: ids(spec, window), cand(spec, id) -> the candidate's bytes or None when it is dropped,
    keyspace(spec) and radices(spec, id), all on the references the suite already has (tests/test_mask.py,
    tests/test_markov.py, tests/join_plan.py, tests/test_gpu_chain.Chain, tests/chain_rules_plan.py,
    tests/table_plan.py, tests/assoc_plan.py, oracle/rules.py); none calls the library.
  * specs(attack): a fixed, seeded list of random specifications, each with its windows.
  * compare(model, prepared, ...): the comparison tests/test_gpu_prepared.py makes per window; SLIPS are deliberately
    wrong models it must catch (tests/test_prepared_plan.py).

What the limits in include/dwpa22000.h rule out, and the lists therefore do not hold: a keyspace above 2^63 for the
table attack (a word owns fewer than 2^32 candidates and a list fewer than 2^32 words, so it would take 2^31 words), the
association attack (the same, per net), dictionaries, rules and the combinator (their ids are products of list sizes
that have to exist in memory); ids at or above 2^32 for the association without rules (its keyspace is its word
count, which the call takes as 32 bits); two equal candidates in one window of a mask, Markov or numeric load (a
position's set holds no byte twice); and a load that keeps more
than the batch: every dwpa_scan_load_* refuses a count above the batch, so the kept counter never passes it through the
scan API.  compare() states the overflow rule all the same and the CPU tests hold it to it; the GPU tests load windows
of exactly the batch.  One thing is left out for its cost, not for a limit: a dictionary load's id is its word index,
so ids across 2^32 take a list of 2^32 words, 32 GiB of offsets alone.  Rules and the association with rules do cross
2^32, as the combinator does: a list of 2^20 words under 4,095 rules, a net of 65,530 words under 65,535 rules.
"""
import functools
import math
import random

import numpy as np

from oracle import rules as OR
from tests import assoc_plan as A
from tests import chain_rules_plan as CR
from tests import rule_corpus as RC
from tests import table_plan as T
from tests import test_gpu_chain as G
from tests import test_markov as MK
from tests.join_plan import COMBI_AMP_LEFT, COMBI_AMP_RIGHT, combi_join, hybrid_join, hybrid_keeps, keeps
from tests.test_mask import BUILTIN, ref_candidate, ref_sets

U32, U64 = 2**32, 2**64
BATCH = 4096  # the scans' batch: the largest window
COUNTS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3000, BATCH)  # lane, wave and 256-thread block edges


# ---------------------------------------------------------------------------------------------------------------
# SHA-1 (FIPS 180-4, 6.1.2) over columns: state [5][n], block [16][n], uint32
# ---------------------------------------------------------------------------------------------------------------
IV = (0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476, 0xC3D2E1F0)


def _rotl(x, n):
    return (x << np.uint32(n)) | (x >> np.uint32(32 - n))


def sha1_compress(state, block):
    """One compression: the five chaining words after `block`, for every column."""
    w = [np.array(x, dtype=np.uint32) for x in block]
    a, b, c, d, e = (np.array(x, dtype=np.uint32) for x in state)
    with np.errstate(over="ignore"):
        for t in range(80):
            if t >= 16:
                w[t % 16] = _rotl(w[(t - 3) % 16] ^ w[(t - 8) % 16] ^ w[(t - 14) % 16] ^ w[t % 16], 1)
            if t < 20:
                f, k = (b & c) | (~b & d), 0x5A827999
            elif t < 40:
                f, k = b ^ c ^ d, 0x6ED9EBA1
            elif t < 60:
                f, k = (b & c) | (b & d) | (c & d), 0x8F1BBCDC
            else:
                f, k = b ^ c ^ d, 0xCA62C1D6
            tmp = _rotl(a, 5) + f + e + np.uint32(k) + w[t % 16]
            e, d, c, b, a = d, c, _rotl(b, 30), a, tmp
        return np.stack([np.array(s, dtype=np.uint32) + x for s, x in zip(state, (a, b, c, d, e))])


def _blocks(data):
    """Bytes of n x 64 -> [n][16] big-endian words."""
    assert len(data) % 64 == 0
    return np.frombuffer(data, dtype=">u4").astype(np.uint32).reshape(-1, 16)


def _iv(n):
    return np.tile(np.array(IV, dtype=np.uint32).reshape(5, 1), (1, n))


def sha1_from(state, done, data):
    """The digest of a message whose first `done` bytes (a multiple of 64) led to `state` ([5] words) and whose rest is
    `data`: the padding of FIPS 180-4 5.1.1, then one compression per block."""
    assert done % 64 == 0
    pad = data + b"\x80" + bytes((55 - len(data)) % 64) + (8 * (done + len(data))).to_bytes(8, "big")
    st = np.array(state, dtype=np.uint32).reshape(5, 1)
    for blk in _blocks(pad):
        st = sha1_compress(st, blk.reshape(16, 1))
    return b"".join(int(x).to_bytes(4, "big") for x in st[:, 0])


def sha1(data):
    return sha1_from(IV, 0, data)


def midstates(keys):
    """uint32 [10][n]: for every key (at most 64 bytes; HMAC pads it with zeros to the block) the chaining words after
    key ^ 0x36.. (rows 0..4) and after key ^ 0x5c.. (rows 5..9), one compression from the IV each."""
    keys = list(keys)
    n = len(keys)
    if not n:
        return np.zeros((10, 0), dtype=np.uint32)
    assert all(len(k) <= 64 for k in keys)
    kb = _blocks(b"".join(k + bytes(64 - len(k)) for k in keys)).T  # [16][n]
    return np.concatenate([sha1_compress(_iv(n), kb ^ np.uint32(0x36363636)),
                           sha1_compress(_iv(n), kb ^ np.uint32(0x5C5C5C5C))])


def hmac_sha1_from_mid(mid, msg):
    """HMAC-SHA1 finished from one key's ten midstate words."""
    mid = [int(x) for x in mid]
    return sha1_from(mid[5:], 64, sha1_from(mid[:5], 64, msg))


# ---------------------------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------------------------
def simulate(model, batch=BATCH):
    """What scan_prepared returns for a generator that computes `model` ({id: bytes}) and compacts in index order."""
    ids = sorted(model)[:batch]
    return {"count": len(model), "ids": np.array(ids, dtype=np.uint64), "mid": midstates(model[i] for i in ids),
            "sref": None}


def compare(model, prep, batch=BATCH, loaded=None, sref=None):
    """AssertionError unless `prep` (dwpa_amd._lib.scan_prepared) is the batch `model` ({id: candidate bytes}, the
    kept candidates of the load) prescribes: the raw counter is the model's size; loaded() that size clamped to the
    batch; the ids are the model's keys, none twice (under overflow: `batch` distinct keys of it, whichever); every
    id's ten midstate words are midstates(model[id]) bit for bit; sref (the expected salt reference per id), when
    given, holds per slot."""
    want = len(model)
    assert prep["count"] == want, "the kept counter is %d, the model keeps %d" % (prep["count"], want)
    n = min(want, batch)
    if loaded is not None:
        assert loaded == n, "loaded() is %d, not %d" % (loaded, n)
    ids = [int(i) for i in prep["ids"]]
    assert len(ids) == n and prep["mid"].shape == (10, n), (len(ids), prep["mid"].shape, n)
    assert len(set(ids)) == n, "an id twice"
    extra = sorted(set(ids) - set(model))
    assert not extra, "ids the model does not keep: %r" % extra[:5]
    if want <= batch:
        missing = sorted(set(model) - set(ids))
        assert not missing, "ids missing: %r" % missing[:5]
    bad = np.nonzero((midstates(model[i] for i in ids) != prep["mid"]).any(axis=0))[0]
    assert not len(bad), "midstates differ for ids %r (the model's candidates: %r)" % (
        [ids[j] for j in bad[:5]], [model[ids[j]] for j in bad[:5]])
    if sref is not None:
        got = [int(x) for x in prep["sref"]]
        assert got == [sref[i] for i in ids], "a slot's salt reference is not its net's"


# ---------------------------------------------------------------------------------------------------------------
# the slips: deliberately wrong models.  Each maps the index the reference is asked for (or its answer) the way a
# slip in a generator would; compare() must catch each on the committed lists wherever it can change anything.
# ---------------------------------------------------------------------------------------------------------------
SLIPS = ("first32", "reversed", "radix", "maxlen64", "lastbyte")


def _split(i, radices):
    """Digits of i over the radices, last fastest; what is left above the first radix wraps."""
    out = []
    for r in reversed(radices):
        i, d = divmod(i, r)
        out.append(d)
    return out[::-1]


def _join(digits, radices):
    i = 0
    for d, r in zip(digits, radices):
        i = i * r + d
    return i


def slip_index(attack, spec, i, slip):
    """The index a generator with the slip would take its candidate for id i from (None: the slip cannot apply)."""
    if slip == "first32":
        return i % U32
    rad = attack.radices(spec, i)
    if rad is None:
        return None
    base, rs = rad
    sub = i - base
    if slip == "reversed":  # the FIRST position fastest
        return base + _join(_split(sub, rs[::-1])[::-1], rs)
    if slip == "radix":  # the last radix above 1 carries one early
        at = max((p for p, r in enumerate(rs) if r > 1), default=None)
        if at is None:
            return None
        wrong = rs[:at] + [rs[at] - 1] + rs[at + 1:]
        return base + _join(_split(sub, wrong), rs)
    raise ValueError(slip)


def model(attack, spec, window, slip=None):
    """{id: candidate bytes} of the kept candidates of a window; with a slip, the model of a generator that has it
    (still keyed by the right ids: a slip changes what a slot holds, not what it is called)."""
    out = {}
    for i in attack.ids(spec, window):
        if slip in (None, "lastbyte"):
            c = attack.cand(spec, i)
            if slip and c:
                c = c[:-1] + bytes([c[-1] ^ 0x01])
        elif slip == "maxlen64":
            c = attack.cand(spec, i, maxlen=64)
        else:
            j = slip_index(attack, spec, i, slip)
            c = attack.cand(spec, i if j is None or j >= attack.keyspace(spec) else j)
        if c is not None:
            out[i] = c
    return out


# ---------------------------------------------------------------------------------------------------------------
# the attacks
# ---------------------------------------------------------------------------------------------------------------
class Attack:
    """name, the kernel it exercises, whether the kernel filters and compacts, and the reference."""
    name = kernel = None
    compacts = True

    def ids(self, spec, win):
        first, count = win
        return range(first, first + count)

    def raw(self, win):
        """Raw candidates (lanes) of a window."""
        return win[1]


def _ref(spec, build):
    if "_ref" not in spec:
        spec["_ref"] = build()
    return spec["_ref"]


class MaskAttack(Attack):
    name, kernel, compacts = "mask", "k_prep_mask", False

    def sets(self, spec):
        return _ref(spec, lambda: ref_sets(spec["mask"], spec["custom"]))[0]

    def keyspace(self, spec):
        return _ref(spec, lambda: ref_sets(spec["mask"], spec["custom"]))[1]

    def cand(self, spec, i, minlen=8, maxlen=63):
        return ref_candidate(self.sets(spec), i)  # a mask load filters nothing

    def radices(self, spec, i):
        return 0, [len(s) for s in self.sets(spec)]


@functools.lru_cache(maxsize=None)
def markov_model():
    """The trained model of tests/test_markov.py: its counts and the image the library takes."""
    n = MK.ref_counts(MK._train_words())
    return n, MK.ref_image(n)


class MarkovAttack(Attack):
    name, kernel, compacts = "markov", "k_prep_markov", False

    def _r(self, spec):
        def build():
            sets = MK.mk_sets(spec["mask"], spec["custom"])
            return {"sets": sets, "rad": MK.ref_radices(sets, spec["threshold"]), "rows": {},
                    "k": MK.ref_keyspace(sets, spec["threshold"])}
        return _ref(spec, build)

    def keyspace(self, spec):
        return self._r(spec)["k"]

    def cand(self, spec, i, minlen=8, maxlen=63):
        """tests/test_markov.ref_markov with its rows remembered: digit d of position p picks the d-th byte of the
        ranking after the byte before it (ref_order), filtered to the position's set and cut at the radix."""
        r, n = self._r(spec), markov_model()[0]
        digits = _split(i, r["rad"])
        out, prev = bytearray(), 0
        for p, s in enumerate(r["sets"]):
            row = r["rows"].get((p, prev))
            if row is None:
                row = r["rows"][(p, prev)] = [b for b in MK.ref_order(n, p, prev) if b in s][:r["rad"][p]]
            prev = row[digits[p]]
            out.append(prev)
        return bytes(out)

    def radices(self, spec, i):
        return 0, list(self._r(spec)["rad"])


class NumericAttack(Attack):
    name, kernel, compacts = "numeric", "k_prep_numeric", False

    def keyspace(self, spec):
        return min(10**spec["digits"], U64)

    def cand(self, spec, i, minlen=8, maxlen=63):
        return b"%0*d" % (spec["digits"], i)

    def radices(self, spec, i):
        return 0, [10] * spec["digits"]


class DictAttack(Attack):
    name, kernel = "dict", "k_prep_dict"

    def keyspace(self, spec):
        return len(spec["words"])

    def cand(self, spec, i, minlen=8, maxlen=63):
        w = spec["words"][i]
        return w if minlen <= len(w) <= maxlen else None

    def radices(self, spec, i):
        return None


class RulesAttack(Attack):
    """Window (first word, words): every rule over them; id = word * nrules + rule."""
    name, kernel = "rules", "k_rules_prep"

    def ops(self, spec):
        return _ref(spec, lambda: [OR.parse(r) for r in spec["rules"]])

    def keyspace(self, spec):
        return len(spec["words"]) * len(spec["rules"])

    def ids(self, spec, win):
        nr = len(spec["rules"])
        return range(win[0] * nr, (win[0] + win[1]) * nr)

    def raw(self, win, spec=None):
        return win[1] * len(spec["rules"])

    def cand(self, spec, i, minlen=8, maxlen=63):
        w, r = divmod(i, len(spec["rules"]))
        c = OR.apply(self.ops(spec)[r], spec["words"][w])
        return c if c is not None and minlen <= len(c) <= maxlen else None

    def radices(self, spec, i):
        return 0, [len(spec["words"]), len(spec["rules"])]


class HybridAttack(Attack):
    """Window (first word, words, mask first, mask count); id = word * K + mask index."""
    name, kernel = "hybrid", "k_prep_hybrid"

    def _r(self, spec):
        return _ref(spec, lambda: ref_sets(spec["mask"], spec["custom"]))

    def keyspace(self, spec):
        return len(spec["words"]) * self._r(spec)[1]

    def ids(self, spec, win):
        fw, nw, mf, mc = win
        k = self._r(spec)[1]
        return [w * k + j for w in range(fw, fw + nw) for j in range(mf, mf + mc)]

    def raw(self, win):
        return win[1] * win[3]

    def cand(self, spec, i, minlen=8, maxlen=63):
        sets, k = self._r(spec)
        w, j = divmod(i, k)
        word = spec["words"][w]
        if not hybrid_keeps(word, len(sets), minlen, maxlen):
            return None
        return hybrid_join(word, ref_candidate(sets, j), spec["mode"])

    def radices(self, spec, i):
        return 0, [len(spec["words"])] + [len(s) for s in self._r(spec)[0]]


class CombinatorAttack(Attack):
    """Window (first base, bases, amplifier first, amplifier count); id = base * A + amplifier index."""
    name, kernel = "combinator", "k_prep_combinator"

    def keyspace(self, spec):
        return len(spec["base"]) * len(spec["amp"])

    def ids(self, spec, win):
        fb, nb, af, ac = win
        a = len(spec["amp"])
        return [b * a + j for b in range(fb, fb + nb) for j in range(af, af + ac)]

    def raw(self, win):
        return win[1] * win[3]

    def cand(self, spec, i, minlen=8, maxlen=63):
        b, a = divmod(i, len(spec["amp"]))
        x, y = spec["base"][b], spec["amp"][a]
        return combi_join(x, y, spec["side"]) if keeps(x, y, minlen, maxlen) else None

    def radices(self, spec, i):
        return 0, [len(spec["base"]), len(spec["amp"])]


class ChainAttack(Attack):
    name, kernel = "chain", "k_prep_chain"

    def chain(self, spec):
        return _ref(spec, lambda: G.Chain(spec["parts"], spec["custom"]))

    def keyspace(self, spec):
        return self.chain(spec).k

    def cand(self, spec, i, minlen=8, maxlen=63):
        psk, keep = self.chain(spec).candidate(i, minlen, maxlen)
        return psk if keep else None

    def radices(self, spec, i):
        return 0, list(self.chain(spec).radix)


class ChainRulesAttack(ChainAttack):
    """parts: a list, a mask, or (list, rule lines) for a ruled list part."""
    name, kernel = "chain_rules", "k_prep_chain_rules"

    def chain(self, spec):
        return _ref(spec, lambda: CR.RuledChain(spec["parts"], spec["custom"]))


class TableAttack(Attack):
    name, kernel, compacts = "table", "k_prep_table", False

    def plan(self, spec):
        return _ref(spec, lambda: T.Plan(spec["table"], spec["words"], 8, 63, spec["word_max"]))

    def keyspace(self, spec):
        return self.plan(spec).k

    def cand(self, spec, i, minlen=8, maxlen=63):
        return self.plan(spec).candidate(i)  # the words are filtered when the table is set: a load keeps everything

    def radices(self, spec, i):
        p = self.plan(spec)
        j = p.word_of(i)
        return p.start[j], [len(p.alt[c]) for c in p.words[p.kword[j]]]


class AssocAttack(Attack):
    """nets [(essid, mac_ap)], words per net, rule lines or None."""
    name = "assoc"

    def __init__(self, rules):
        self.with_rules = rules
        self.kernel = "k_prep_assoc<%s>" % ("true" if rules else "false")

    def plan(self, spec):
        return _ref(spec, lambda: A.Plan([], nets=spec["nets"], words=spec["words"], rules=spec["rules"]))

    def keyspace(self, spec):
        return self.plan(spec).k

    def cand(self, spec, i, minlen=8, maxlen=63):
        return self.plan(spec).candidate(i, minlen, maxlen)

    def radices(self, spec, i):
        p = self.plan(spec)
        n = p.net_of(i)
        return p.start[n], [p.r, len(p.words[n])]


def salt_refs(essids):
    """ESSID -> the word offset of its entry in an association's salt table: one entry {nsalt, [2][nsalt][16]} per
    ESSID in byte order, nsalt the SHA-1 blocks of ESSID || INT(i) behind the 64-byte key block."""
    out, at = {}, 0
    for e in sorted(set(essids)):
        out[e] = at
        at += 1 + 2 * 16 * ((len(e) + 4 + 9 + 63) // 64)
    return out


def assoc_srefs(spec, plan, ids):
    ref = salt_refs(e for e, m in spec["nets"])
    return {i: ref[spec["nets"][plan.net_of(i)][0]] for i in ids}


ATTACKS = {a.name if a.name != "assoc" else ("assoc_rules" if a.with_rules else "assoc_plain"): a for a in (
    MaskAttack(), MarkovAttack(), NumericAttack(), DictAttack(), RulesAttack(), HybridAttack(), CombinatorAttack(),
    ChainAttack(), ChainRulesAttack(), TableAttack(), AssocAttack(False), AssocAttack(True))}


def raw_count(name, spec, win):
    a = ATTACKS[name]
    return a.raw(win, spec) if name == "rules" else a.raw(win)


# ---------------------------------------------------------------------------------------------------------------
# seeded random specifications
# ---------------------------------------------------------------------------------------------------------------
EDGE_BYTES = bytes([0x00, 0x0a, 0x80, 0xff])
SET_SIZES = (1, 2, 3, 5, 7, 10, 16, 17, 26, 64, 95, 100, 200, 255, 256)


def _esc(bs):
    """Raw bytes as mask-language text: '?' doubled."""
    return b"".join(b"??" if c == 0x3f else bytes([c]) for c in bs)


def _rand_set(rng, size):
    """`size` distinct bytes in a random order, the edge bytes 0x00 0x0a 0x80 0xff first in line to be among them."""
    rest = [c for c in range(256) if c not in EDGE_BYTES]
    rng.shuffle(rest)
    pick = (list(EDGE_BYTES) + rest)[:size] if rng.random() < 0.7 else rest[:size]
    rng.shuffle(pick)
    return bytes(pick)


def _rand_word(rng, n, binary=False):
    if binary:
        return bytes(rng.choice(EDGE_BYTES + b"aZ9") for _ in range(n))
    return bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789-_ .") for _ in range(n))


def rand_mask(rng, npos, bits, threshold=0, nsets=None):
    """(mask, custom): npos positions -- literals (any byte, '?' and the edge bytes among them), built-in sets and up
    to four custom sets of 1..256 raw bytes -- whose keyspace (every set cut at `threshold` if given) stays below
    2^bits.  About nsets positions (default: up to 12) carry a set, the others a literal."""
    customs = [_rand_set(rng, rng.choice(SET_SIZES)) for _ in range(rng.randint(1, 4))]
    options = [(b"?" + c.encode(), len(BUILTIN[c])) for c in "ludhHsab"]
    options += [(b"?%d" % (k + 1), len(c)) for k, c in enumerate(customs)]
    want = min(npos, nsets if nsets is not None else rng.randint(1, 12))
    at = set(rng.sample(range(npos), want))
    toks, used = [], 0.0
    for p in range(npos):
        tok = None
        if p in at:
            t, size = rng.choice(options)
            cost = math.log2(min(size, threshold) if threshold else size)
            if used + cost < bits - 0.01:
                tok, used = t, used + cost
        toks.append(tok if tok else _esc(bytes([rng.choice(EDGE_BYTES + b"?aZ0- ~")])))
    return b"".join(toks), tuple(_esc(c) for c in customs)


def _across(rng, c):
    """A first index with first < 2^32 <= first + c - 1."""
    return U32 - 1 - rng.randrange(c - 1)


def index_windows(rng, k, n, inside=()):
    """Windows (first, count) of a keyspace k for the n-th spec of a list: four counts of COUNTS (the lists walk
    through all of them), started at 0, ending at k, across 2^32 where k allows, and at random 64-bit offsets; then
    one window around each index of `inside`."""
    out = []
    for j in range(4):
        c = COUNTS[(4 * n + j) % len(COUNTS)]
        if c > k:
            c = k
        if not c:
            continue
        kinds = [0, k - c, rng.randrange(k - c + 1)]
        if c > 1 and k >= U32 + c:
            kinds.append(_across(rng, c))
        out.append((kinds[(n + j) % len(kinds)], c))
    if k >= U32 + 257:
        out.append((_across(rng, 257), 257))
    for at in inside:
        c = min(k, 130)
        out.append((max(0, min(at - c // 2, k - c)), c))
    return out


def _rect(rng, c, n0, n1):
    """(a, b) with a * b == c, a <= n0, b <= n1, preferring neither to be 1; None when there is no such pair."""
    pairs = [(a, c // a) for a in range(1, min(c, n0) + 1) if c % a == 0 and c // a <= n1]
    if not pairs:
        return None
    inner = [p for p in pairs if p[0] > 1 and p[1] > 1]
    return rng.choice(inner or pairs)


def _lengths_list(rng, lengths, binary_every=5):
    return [_rand_word(rng, n, binary=(i % binary_every == 3)) for i, n in enumerate(lengths)]


def _mask_specs():
    rng = random.Random(0x3a51)
    out = [{"name": "top", "mask": b"\x00?b?bA?b?b?b\xff?b?b?1z", "custom": (_esc(_rand_set(rng, 200)),)},  # 200 * 2^56
           {"name": "literals63", "mask": _esc(_rand_word(rng, 63, True)), "custom": ()},                   # K = 1
           {"name": "nested", "mask": b"?2x?1?3", "custom": (b"?d\x00\xff", b"?1\n\x80", b"?2?l")},
           {"name": "ones", "mask": b"?1?2?1?2?1?2?1?d?d?d?d", "custom": (b"\x00", b"\xff")}]          # radix 1 sets
    for n, npos in enumerate((1, 8, 63, 7, 9, 10, 11, 62, 33, 17, 63, 40)):
        bits = (20, 40, 63.9)[n % 3]
        m, c = rand_mask(rng, npos, bits, nsets=None if bits < 40 else min(npos, 14))  # enough sets to get near it
        out.append({"name": "rand%d" % n, "mask": m, "custom": c})
    a = ATTACKS["mask"]
    for n, s in enumerate(out):
        s["windows"] = index_windows(rng, a.keyspace(s), n)
    return out


def _markov_specs():
    rng = random.Random(0x3a52)
    out = [{"name": "top", "mask": b"?b" * 8, "custom": (), "threshold": 255},          # 255^8: above 2^63
           {"name": "cut1", "mask": b"?a?1?b?dpre", "custom": (EDGE_BYTES + b"ab",), "threshold": 1},
           {"name": "wide", "mask": b"?a" * 12, "custom": (), "threshold": 10},      # 95^12 is above 2^64
           {"name": "model", "mask": b"pre??x?1?2?l", "custom": (b"ab", b"?dXY"), "threshold": 0}]
    for n, (npos, t) in enumerate(((1, 256), (8, 3), (63, 2), (9, 27), (10, 200), (11, 16), (33, 95), (63, 256))):
        bits = (20, 40, 63.9)[n % 3]
        m, c = rand_mask(rng, npos, bits, threshold=t, nsets=None if bits < 40 else min(npos, 14))
        out.append({"name": "rand%d" % n, "mask": m, "custom": c, "threshold": t})
    a = ATTACKS["markov"]
    for n, s in enumerate(out):
        s["windows"] = index_windows(rng, a.keyspace(s), n)
    return out


def _numeric_specs():
    rng = random.Random(0x3a53)
    out = [{"name": "d%d" % d, "digits": d} for d in range(8, 21)]
    a = ATTACKS["numeric"]
    for n, s in enumerate(out):
        s["windows"] = index_windows(rng, a.keyspace(s), n)
    return out


def _offset_lists(rng, lengths):
    """Word lists whose words of 1..63 bytes start at every offset mod 4 with every length mod 4."""
    for _ in range(1000):
        ls = list(lengths)
        rng.shuffle(ls)
        off, pairs = 0, set()
        for n in ls:
            if 1 <= n <= 63:
                pairs.add((n % 4, off % 4))
            off += n
        if len(pairs) == 16:
            return ls
    raise AssertionError("no order covers every (length % 4, offset % 4) pair")


def _dict_specs():
    rng = random.Random(0x3a54)
    out = []
    for n in range(3):
        ls = _offset_lists(rng, list(range(71)) * 2 + [rng.randint(0, 70) for _ in range(4400)])
        words = _lengths_list(rng, ls)
        words += [words[7], words[7], b"twice-in-a-row", b"twice-in-a-row"]
        out.append({"name": "list%d" % n, "words": words})
    out.append({"name": "all-kept", "words": [b"%08d" % i for i in range(BATCH + 100)]})
    for n, s in enumerate(out):
        s["windows"] = index_windows(rng, len(s["words"]), n)
    out[-1]["windows"].append((50, BATCH))  # every slot of the batch taken
    return out


def _rule_pool(rng, n):
    """n rules of tests/rule_corpus.py, rejecting and memory functions among them."""
    pool = [r for r in RC.single_function_rules() + RC.memory_rules() + RC.combo_rules(120, 0x3a) if OR.parse(r)]
    must = [":", "l", ">8", "<9", "_9", "M [ 4", "$1 $2 $3", "d", "Q", "!a"]
    return must[:n] + rng.sample([r for r in pool if r not in must], max(0, n - len(must)))


def _rules_specs():
    rng = random.Random(0x3a55)
    lens = (0, 1, 4, 7, 8, 9, 12, 20, 31, 32, 33, 60, 62, 63, 64, 65, 128, 255, 256, 257)
    out = []
    for n, nrules in enumerate((1, 1, 1, 5, 64, 16)):
        nwords = (BATCH + 64) if nrules == 1 else 300
        ls = _offset_lists(rng, [rng.choice(lens) if i % 3 else rng.randint(5, 12) for i in range(nwords)])
        words = [_rand_word(rng, ln, binary=(i % 7 == 3)) for i, ln in enumerate(ls)]
        rules = ["$1 c", "d", "[ $x $y"][n:n + 1] if nrules == 1 else _rule_pool(rng, nrules)
        out.append({"name": "r%d_%d" % (nrules, n), "words": words, "rules": rules})
    for n, s in enumerate(out):
        nr, nw = len(s["rules"]), len(s["words"])
        wins = []
        for j in range(4 if nr == 1 else 3):
            c = COUNTS[(4 * n + j) % len(COUNTS)] if nr == 1 else max(1, min(BATCH // nr, (13, 64, 47)[j] * 16 // nr))
            wins.append(((0, nw - c, rng.randrange(nw - c + 1))[(n + j) % 3], c))
        s["windows"] = wins
    # ids across 2^32: 4,095 rules (a word's results fill the batch but for one slot) over 2^20 + 264 words; word
    # 1,048,832 owns the ids 2^32 - 256 .. 2^32 + 3,838
    rules = wide_rules(4095)
    words = [b"%07d" % i for i in range(U32 // len(rules) + 8)]
    out.append({"name": "wide", "words": words, "rules": rules,
                "windows": [(0, 1), (U32 // len(rules), 1), (len(words) - 1, 1)]})
    return out


def wide_rules(n):
    """n distinct rules, for ids across 2^32: appends of two or three characters behind a few rejecting ones."""
    chars = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNO"
    if n <= len(chars) ** 2:
        out = ["$%s $%s" % (x, y) for x in chars for y in chars][:n]
    else:
        out = ["$%s $%s $%s" % (x, y, z) for x in chars for y in chars for z in chars][:n]
    assert len(out) == n == len(set(out))
    return [":", "l", ">8", "<9", "_9", "Q"] + out[6:]


def _hybrid_specs():
    rng = random.Random(0x3a56)
    out = []
    # ids above 2^63 (one word under a keyspace of 200 * 2^56) and mask indices across 2^32, both modes
    for mode in (6, 7):
        out.append({"name": "top%d" % mode, "mask": b"?b?b?b?b?b?b?b?1", "custom": (_esc(_rand_set(rng, 200)),),
                    "mode": mode, "words": [b"w", b"", b"x" * 55, b"y" * 56][:1 if mode == 6 else 4]})
    out[-1]["mask"], out[-1]["custom"] = b"?d?d?d?d?d?d?d?d?d?d", ()  # 10^10: words x indices across 2^32
    for n, (npos, mode) in enumerate(((1, 6), (1, 7), (3, 6), (3, 7), (8, 6), (8, 7), (20, 6), (62, 7), (63, 6),
                                       (5, 7))):
        m, c = rand_mask(rng, npos, 12, nsets=min(npos, 3))
        ls = _offset_lists(rng, list(range(71)) + [max(0, 8 - npos), max(0, 7 - npos), 63 - npos, 64 - npos] * 3)
        words = _lengths_list(rng, ls)
        words += [w for w in words if len(w) + npos == 9][:1] * 2  # a word three times: equal candidates, other ids
        out.append({"name": "rand%d" % n, "mask": m, "custom": c, "mode": mode, "words": words})
    a = ATTACKS["hybrid"]
    for n, s in enumerate(out):
        k, nw = a._r(s)[1], len(s["words"])
        wins = []
        for j in range(4):
            c = COUNTS[(4 * n + j) % len(COUNTS)]
            shape = _rect(rng, c, nw, min(k, U32 - 1))
            if shape is None:
                continue  # another spec of the list takes this count
            words, mc = shape
            fw = (0, nw - words, rng.randrange(nw - words + 1))[(n + j) % 3]
            mf = (0, k - mc, rng.randrange(k - mc + 1))[(n + j + 1) % 3]
            if mc > 1 and k >= U32 + mc and j == 3:
                mf = _across(rng, mc)
            wins.append((fw, words, mf, mc))
        cw, cm = min(nw, 3), min(k, 43)  # the first and the last corner of the words x indices rectangle
        s["windows"] = wins + [(0, cw, 0, cm), (nw - cw, cw, k - cm, cm)]
    return out


def _combinator_specs():
    rng = random.Random(0x3a57)
    out = []
    for n, side in enumerate((COMBI_AMP_RIGHT, COMBI_AMP_LEFT, COMBI_AMP_RIGHT, COMBI_AMP_LEFT)):
        base = _lengths_list(rng, _offset_lists(rng, list(range(67)) + [300, 4, 4, 5, 3, 60, 59, 58]))
        amp = _lengths_list(rng, _offset_lists(rng, list(range(67)) + [300, 4, 4, 3, 5, 1, 2, 6]))
        # joins that meet: ab + c = a + bc, twice over
        base += [b"meet-ab", b"meet-a", b"meet-a"]
        amp += [b"c", b"bc"]
        out.append({"name": "rand%d" % n, "base": base, "amp": amp, "side": side})
    # 66,000 x 66,000 words: ids across 2^32
    big = [b"%07d" % i for i in range(66000)]
    out.append({"name": "wide-right", "base": big, "amp": [b"-" + w for w in big], "side": COMBI_AMP_RIGHT})
    out.append({"name": "wide-left", "base": big, "amp": [b"-" + w for w in big], "side": COMBI_AMP_LEFT})
    for n, s in enumerate(out):
        nb, na = len(s["base"]), len(s["amp"])
        wins = []
        for j in range(4):
            c = COUNTS[(4 * n + j) % len(COUNTS)]
            shape = _rect(rng, c, min(nb, 70), min(na, 4096))
            if shape is None:
                continue  # another spec of the list takes this count
            b, a = shape
            wins.append(((0, nb - b, rng.randrange(nb - b + 1))[(n + j) % 3], b,
                         (0, na - a, rng.randrange(na - a + 1))[(n + j + 1) % 3], a))
        if nb == 66000:  # base 65075 ends below 2^32, base 65076 begins above it
            wins.append((U32 // na - 1, 3, na - 100, 100))
            wins.append((U32 // na, 1, U32 % na - 128, 257))
        s["windows"] = wins + [(0, 3, 0, 43), (nb - 3, 3, na - 43, 43)]  # the rectangle's first and last corner
    return out


def _chain_parts(rng, arity, bits):
    """Parts of a random chain: lists (one of them a single word now and then) and small masks mixed."""
    parts, kinds = [], [rng.choice("LM") for _ in range(arity)]
    if "L" not in kinds:
        kinds[rng.randrange(arity)] = "L"
    if "M" not in kinds:
        kinds[rng.randrange(arity)] = "M"
    share = 40 // arity
    for kind in kinds:
        if kind == "M":
            npos = rng.randint(1, 5)
            parts.append(rand_mask(rng, npos, bits / arity, nsets=rng.randint(0, min(npos, 2))))
        else:
            n = rng.choice((1, 2, 3, 17, 64, 65, 100))
            lens = [rng.choice((0, 1, 2, 3, 5, 8, share, share + 1, 63 - share, 62, 63, 64, 70)) for _ in range(n)]
            parts.append(_lengths_list(rng, lens))
    return parts


def _chain_specs():
    rng = random.Random(0x3a58)
    top = _esc(_rand_set(rng, 100))
    out = [{"name": "top", "parts": [[b"", b"W" * 55], b"?b?b?b?b?b?b?b?1"], "custom": (top,)},  # 200 * 2^56
           {"name": "meet", "parts": [[b"prefix-ab", b"prefix-a"], [b"c", b"bc"]], "custom": ()},
           {"name": "ones", "parts": [[b"only-one"], b"-x-", [b"", b"a"], b"?1"], "custom": (b"\x00",)},
           {"name": "wide", "parts": [b"?d?d?d?d?d", [b"-", b"+-", b"x" * 64], b"?d?d?d?d?d?d"], "custom": ()},
           # totals of 6, 7, 7, 8 and 62, 63, 63, 64 bytes
           {"name": "lengths", "parts": [[b"ab", b"abc", b"x" * 58, b"x" * 59], b"-?d-", [b"y", b"yy"]], "custom": ()}]
    for n, arity in enumerate((2, 3, 4, 2, 3, 4, 2, 3, 4)):
        while True:
            parts = _chain_parts(rng, arity, 30)
            # the custom sets of a chain are shared by its mask parts: give every mask part built-in sets and ?1 only
            custom = (_esc(_rand_set(rng, rng.choice(SET_SIZES[:8]))),)
            parts = [p if isinstance(p, list) else _only_first_custom(p[0]) for p in parts]
            spec = {"name": "rand%d" % n, "parts": parts, "custom": custom}
            ch = ATTACKS["chain"].chain(spec)
            if 5000 <= ch.k < U64 and any(ch.candidate(i)[1] for i in range(min(ch.k, 300))):
                break
        out.append(spec)
    a = ATTACKS["chain"]
    for n, s in enumerate(out):
        s["windows"] = index_windows(rng, a.keyspace(s), n)
    return out


def _only_first_custom(mask):
    """A mask text whose custom-set tokens all name ?1."""
    out, i = [], 0
    while i < len(mask):
        if mask[i:i + 1] == b"?":
            t = mask[i:i + 2]
            out.append(b"?1" if t in (b"?2", b"?3", b"?4") else t)
            i += 2
        else:
            out.append(mask[i:i + 1])
            i += 1
    return b"".join(out)


def _chain_rules_specs():
    rng = random.Random(0x3a59)
    top = _esc(_rand_set(rng, 50))
    low = [b"lower-%02d" % i for i in range(6)]
    out = [{"name": "top", "parts": [([b"Ab", b"cD"], [":", "c"]), b"?b?b?b?b?b?b?b?1"], "custom": (top,)},
           {"name": "collide", "parts": [(low, [":", "l", "$1", "$1 ]"]), [b"", b"1"]], "custom": ()},
           {"name": "wide", "parts": [b"?d?d?d?d?d", ([b"-", b"+-", b"x" * 64], [":", "d", ">2"]), b"?d?d?d?d?d"],
            "custom": ()},
           # totals of 6, 7, 7, 8 and 62, 63, 63, 64 bytes, and one more each under '$!'
           {"name": "lengths", "parts": [([b"ab", b"abc", b"x" * 58, b"x" * 59], [":", "$!"]), b"-?d-", [b"y", b"yy"]],
            "custom": ()}]
    for n, arity in enumerate((2, 3, 4, 2, 3, 4)):
        while True:
            custom = (_esc(_rand_set(rng, rng.choice(SET_SIZES[:8]))),)
            parts = [p if isinstance(p, list) else _only_first_custom(p[0]) for p in _chain_parts(rng, arity, 24)]
            lists = [p for p, x in enumerate(parts) if isinstance(x, list)]
            for p in rng.sample(lists, rng.randint(1, len(lists))):
                parts[p] = (parts[p] + [_rand_word(rng, 257), _rand_word(rng, 256)],
                            _rule_pool(rng, rng.choice((1, 3, 12))))
            spec = {"name": "rand%d" % n, "parts": parts, "custom": custom}
            ch = ATTACKS["chain_rules"].chain(spec)
            if 5000 <= ch.k < U64 and any(ch.candidate(i)[1] for i in range(min(ch.k, 300))):
                break
        out.append(spec)
    a = ATTACKS["chain_rules"]
    for n, s in enumerate(out):
        s["windows"] = index_windows(rng, a.keyspace(s), n)
    return out


def _table_specs():
    rng = random.Random(0x3a5a)
    out = []
    for n in range(5):
        keys = rng.sample(range(256), 24)
        mapping = {}
        for j, k in enumerate(keys + list(EDGE_BYTES[:2])):
            alts = _rand_set(rng, (1, 2, 3, 5, 8, 16, 2, 4)[j % 8])
            if j % 3 == 0:  # an alternative equal to its key
                alts = bytes([k]) + bytes(c for c in alts if c != k)[:len(alts) - 1]
            mapping[k] = alts
        # two keys with one alternative list: words that differ only there give equal candidates
        mapping[keys[1]] = mapping[keys[0]] if n % 2 == 0 else mapping[keys[1]]
        neutral = bytes(c for c in range(0x30, 0x7b) if c not in mapping)
        words = []
        for i in range(500):
            ln = rng.choice((0, 5, 7, 8, 8, 9, 10, 11, 12, 16, 33, 62, 63, 63, 64, 70))
            nk = rng.choice((0, 0, 1, 1, 2, 3, 5, 8))
            w = bytearray(rng.choice(neutral) for _ in range(ln))
            for p in rng.sample(range(ln), min(nk, ln)):
                w[p] = rng.choice(list(mapping))
            words.append(bytes(w))
        twin = bytearray(b"twin-word-")
        words[50:50] = [bytes(twin + bytes([keys[0]])), bytes(twin + bytes([keys[1]]))]
        out.append({"name": "rand%d" % n, "table": T.table_text(mapping), "words": words,
                    "word_max": (0, 4096, 100, 16, 0)[n]})
    out.append({"name": "big", "table": T.TABLE, "words": list(T.PLAN_BIG.words), "word_max": 0})  # K = 3 * 2^31
    a = ATTACKS["table"]
    for n, s in enumerate(out):
        p = a.plan(s)
        wide = max(range(p.kept()), key=lambda j: p.count[p.kword[j]])
        inside = [p.start[wide] + p.count[p.kword[wide]] // 2, p.start[wide + 1]]
        s["windows"] = index_windows(rng, p.k, n, inside=[i for i in inside if i < p.k])
    return out


def _assoc_specs(with_rules):
    rng = random.Random(0x3a5c if with_rules else 0x3a5b)
    out = []
    for n in range(4):
        nnets = (3, 9, 20, 40)[n]
        essids = [b"net-%d-%s" % (j, b"e" * rng.choice((0, 3, 17))) for j in range(nnets)]
        essids[1] = essids[0]  # two nets (two MACs) under one ESSID
        nets = [(e[:32], A.mac(0x100 * n + j)) for j, e in enumerate(essids)]
        words = []
        for j in range(nnets):
            nw = (0, 1, 4200, 2, 65, 0, 130)[j % 7] if n else (1500, 0, 2600)[j]
            ws = [_rand_word(rng, rng.choice((1, 7, 8, 9, 20, 62, 63, 64, 100, 256)), binary=(i % 9 == 4))
                  for i in range(nw)]
            # nets of several words share two, the first of their list; the nets of no word and of one stay as they are
            words.append(list(dict.fromkeys(([b"Shared-Word", b"lower-word"] if nw > 1 else []) + ws)))
        rules = None
        if with_rules:
            rules = [":", "l", "u"] + _rule_pool(rng, (2, 5, 9, 17)[n])[1:]
        out.append({"name": "nets%d" % nnets, "nets": nets, "words": words, "rules": rules})
    a = ATTACKS["assoc_rules" if with_rules else "assoc_plain"]
    for n, s in enumerate(out):
        p = a.plan(s)
        big = max(range(len(p.words)), key=lambda j: len(p.words[j]))
        s["windows"] = index_windows(rng, p.k, n, inside=[(p.start[big] + p.start[big + 1]) // 2])
    if with_rules:
        # ids across 2^32: a net may own up to 2^32 - 1 indices, so 65,530 words under 65,535 rules end just below
        # 2^32 and the next net's indices cross it (inside its rule 4,587)
        nets = [(b"wide-net", A.mac(0x900)), (b"wide-next", A.mac(0x901)), (b"wide-net", A.mac(0x902))]
        words = [[b"w%07d" % i for i in range(65530)], [_rand_word(rng, rng.choice((5, 6, 9, 60, 61, 62))) + b"%02d" % i
                                                      for i in range(100)], [b"last-net-1", b"last-net-2"]]
        s = {"name": "wide", "nets": nets, "words": words, "rules": wide_rules(65535)}
        k = a.plan(s).k
        s["windows"] = [(0, 64), (U32 - 100, 257), (a.plan(s).start[1] - 60, 130), (k - 65, 65)]
        out.append(s)
    return out


@functools.lru_cache(maxsize=None)
def specs(name):
    """The committed list of an attack: [{"name", its parameters, "windows"}]."""
    return {"mask": _mask_specs, "markov": _markov_specs, "numeric": _numeric_specs, "dict": _dict_specs,
            "rules": _rules_specs, "hybrid": _hybrid_specs, "combinator": _combinator_specs, "chain": _chain_specs,
            "chain_rules": _chain_rules_specs, "table": _table_specs,
            "assoc_plain": lambda: _assoc_specs(False), "assoc_rules": lambda: _assoc_specs(True)}[name]()


def rules_bytes(rules):
    """Rule lines as the text the library takes (the corpus holds bytes above 0x7f as latin-1 characters)."""
    return ("\n".join(rules) + "\n").encode("latin-1")
