"""The PMK differential's plan (CPU): which candidates under which ESSIDs tests/test_gpu_pmk.py derives, the oracle's
PMK of each, where the large launches are sampled, the comparison, and five deliberately wrong PBKDF2 models that
tests/test_pmk_plan.py shows the comparison catches.

The reference is oracle.c_pbkdf2_many (OpenSSL).  Its PMKs are computed once per session, keyed by (ESSID, PSK), and
pickled for the forced-kernel child processes (FIXTURE_ENV).  Everything that depends on the device is a function of
its CU count, so the same tables can be built, counted and checked without one.

A PMK is compared as the device holds it: eight 32-bit words, the big-endian reading of its 32 bytes; output block 1 is
words 0..4, block 2 words 5..7.
"""
import hashlib
import os
import pickle
import random
import time

import numpy as np

from oracle import oracle as O
from tests import assoc_plan as A
from tests import synth as S

FIXTURE_ENV = "DWPA_PMK_FIXTURE"   # set for the forced-build children: the parent's pickled tables
REACHED_ENV = "DWPA_PMK_REACHED"   # set for them too: where a child leaves the kernel names it reached
DIGITS = 9
PLANT_PSK = b"no-candidate-is-this"   # the PSK of every scan line: nothing hits
MAX_PMKS = 16384                   # the file's oracle budget


def psk(v):
    return b"%0*d" % (DIGITS, v)


def nsalt(essid):
    """SHA-1 blocks of the salt message behind the 64-byte HMAC key block: ESSID, INT(i), 0x80, the 8-byte length."""
    return (len(essid) + 4 + 1 + 8 + 63) // 64


# ---------------------------------------------------------------------------------------------------------------
# ESSIDs
# ---------------------------------------------------------------------------------------------------------------
ESSID_LENGTHS = tuple(range(0, 33)) + (33, 51, 52, 115, 116)
ESSID_1 = b"q"
ESSID_32 = bytes(0x41 + i % 26 for i in range(32))


def make_essid(n):
    """One ESSID per length.  1 and 32 bytes: those of tests/test_gpu_pbkdf2_queue_lds.py.  Short ones carry the bytes a
    text handler would trip over (NUL first and last, LF, 0xff); the others are seeded binary."""
    fixed = {1: ESSID_1, 2: b"\x00\x0a", 3: b"\xff\x00\x0a", 4: b"\x0a\xff\xff\x00", 32: ESSID_32}
    return fixed[n] if n in fixed else random.Random(0xe551d + n).randbytes(n)


def oracle_takes(essid):
    """Whether the oracle can use a line with this ESSID at all (an empty hex field is no valid hex to it)."""
    pmk = bytes(range(32))
    line = S.pmkid_line(PLANT_PSK, essid, bytes(6), b"\x01" * 6, the_pmk=pmk)
    return O.c_check_key_m22000(line, [PLANT_PSK], pmk, 8) is not False


# Which ESSIDs are usable is the oracle's decision, oracle_takes().  The length filter below is that verdict cached, not
# the rule: importing the plan should not call the oracle, and tests/test_pmk_plan.py fails if the two ever disagree.
ALL_ESSIDS = tuple(make_essid(n) for n in ESSID_LENGTHS)
ESSIDS = tuple(e for e in ALL_ESSIDS if len(e) > 0)
REFUSED = tuple(e for e in ALL_ESSIDS if len(e) == 0)


def by_len(n):
    return next(e for e in ESSIDS if len(e) == n)


def group_order(essids):
    """A scan numbers its ESSID groups in byte order of the ESSIDs (engine.cpp scan_create: a std::map of strings)."""
    out = sorted(set(essids))
    assert len(out) == len(essids)
    return out


def scan_line(essid, k=0):
    """A PMKID line of PLANT_PSK: usable, and hit by no candidate."""
    return S.pmkid_line(PLANT_PSK, essid, A.mac(0x900000 + k), b"\x02\x5a" + k.to_bytes(4, "big"))


# ---------------------------------------------------------------------------------------------------------------
# the tables' contents
# ---------------------------------------------------------------------------------------------------------------
SLOTS = 1088                                   # four workgroups of 256 plus one wave
COUNTS = (1087, 1023, 257, 256, 255, 65, 64, 63, 1)   # the partial loads; load k starts at SLOTS_FIRST + 1 + k
SLOTS_FIRST = 200_000_011
SLOTS_POISON = 900_000_000                     # loaded and never derived: what a lane past the count would derive
SLOT_ESSIDS = (ESSID_1, ESSID_32)
SWEEP = 64
SWEEP_FIRST = 310_000_007                      # pbkdf2(g) derives [first, first + 64), run() [first + 1, first + 65)
QUEUE_FIRST = 420_000_013
QUEUE_SHIFT = 7                                # the second queue load starts this much later
QUEUE_POISON = 910_000_000
GROUP_FIRST = 530_000_017
GROUP_POISON = (920_000_000, 930_000_000)      # derived by a first run(); then loaded and never derived
GROUP_ESSID_LENGTHS = (1, 52, 116)
GROUP_TAIL = 37
PRIO_FIRST = 640_000_019
CHECK_JOBS = 192
CHECK_LENGTHS = (1, 51, 52, 116)
ASSOC_LENGTHS = (1, 51, 52, 115, 116, 32)
ASSOC_NETS = 40
ASSOC_RULE = "$!"


def slot_values():
    """The values case a and b derive: load k (k = 0: all SLOTS slots) starts at SLOTS_FIRST + k, so no slot holds the
    candidate it held in the load before and one run of consecutive values serves every load."""
    return range(SLOTS_FIRST, SLOTS_FIRST + SLOTS + len(COUNTS))


def sweep_values():
    return range(SWEEP_FIRST, SWEEP_FIRST + SWEEP + 1)


def level_lanes(cus):
    return cus * 4 * 64


def queue_threshold(cus):
    """The largest PMK count that is not a work queue (pbkdf2_module.cpp use_prio): 2 * pmks <= 8 * level_lanes.  One
    resident round of the queue kernels holds as many slots."""
    return 4 * level_lanes(cus)


def _up64(x):
    return (x // 64 + 1) * 64


def sizes(cus):
    """tests/test_gpu_recall.py's sizes, as a plain function of the CU count."""
    ll = level_lanes(cus)
    return {"level_lanes": ll,
            "one": {"plain": ll // 2 // 64 * 64, "p": _up64(ll // 2), "q": _up64(4 * ll)},
            "mg": {"plain": ll // 6 // 64 * 64, "p": _up64(ll // 6), "q": _up64(8 * ll // 6)}}


def sample(n, q, total, base=0, seed=0):
    """Sorted slots of [0, n) of a large launch whose resident round holds q lanes and whose slot 0 is lane `base` of
    the launch's lane space.  Structural: the slots tests/test_gpu_pbkdf2_queue_lds.py samples (first and last slot,
    lanes 0, 63, 64, both sides of a workgroup's end, the last slot of the resident round and the first of a wave's
    second item, the last full wave's ends) and both sides of every multiple of q / 8 -- an XCD's share of the round.
    Seeded filler brings the set to `total`."""
    assert q % 8 == 0 and n >= 1
    pos = set(structural(n, q, base))
    assert len(pos) <= total <= n
    rng = random.Random((seed << 32) ^ n)
    while len(pos) < total:
        pos.add(rng.randrange(n))
    return sorted(pos)


def structural(n, q, base=0):
    last_full = (n // 64) * 64
    pos = {0, 1, 63, 64, 65, 127, 128, 255, 256, last_full - 64, last_full - 1, last_full, n - 1}
    lanes = {q - 64, q - 1, q, q + 1, q + 63, q + 64}
    for m in range(0, base + n + q // 8, q // 8):
        lanes |= {m - 1, m}
    pos |= {x - base for x in lanes}
    return sorted(p for p in pos if 0 <= p < n)


def queue_case(cus):
    q = queue_threshold(cus)
    n = q + 193
    return {"q": q, "n": n, "essid": ESSID_32, "first": QUEUE_FIRST, "sample": sample(n, q, 1024)}


def group_case(cus):
    q = queue_threshold(cus)
    batch = sizes(cus)["mg"]["q"]
    assert batch % 64 == 0 and 3 * batch > q >= 3 * (batch - 64)
    essids = group_order([by_len(x) for x in GROUP_ESSID_LENGTHS])
    n = batch - GROUP_TAIL
    return {"q": q, "batch": batch, "n": n, "essids": essids, "first": GROUP_FIRST,
            "sample": [sample(n, q, 512, base=c * batch, seed=c + 1) for c in range(3)]}


def prio_cases(cus):
    """The smallest _p and _mg_p batches, fully loaded; the oracle sample is the structural positions alone (q: the
    resident round of the queue kernels means nothing here, so its multiples of q / 8 are plain spread-out slots)."""
    s, q = sizes(cus), queue_threshold(cus)
    one, mg = s["one"]["p"], s["mg"]["p"]
    essids = group_order([by_len(x) for x in GROUP_ESSID_LENGTHS])
    return {"one": {"batch": one, "essid": ESSID_32, "first": PRIO_FIRST, "sample": structural(one, q)},
            "mg": {"batch": mg, "essids": essids, "first": PRIO_FIRST + 1_000_003,
                   "sample": [structural(mg, q, base=c * mg) for c in range(3)]}}


def assoc_case(rules):
    """ASSOC_NETS nets whose ESSIDs cycle through ASSOC_LENGTHS (one, two and three salt blocks), 1..3 words each: a
    net's slots are at most three, so neighbouring lanes of a wave differ in their salt's block count."""
    essids = [by_len(x) for x in ASSOC_LENGTHS]
    nets = [(essids[n % len(essids)], A.mac(0x910000 + n)) for n in range(ASSOC_NETS)]
    words = [A.counter_words(b"pmk-net%02d" % n, 1 + n % 3) for n in range(ASSOC_NETS)]
    plan = A.Plan(None, rules=[ASSOC_RULE] if rules else None, nets=nets, words=words)
    assert plan.dropped == 0 and plan.k == sum(len(w) for w in words)
    cands = [plan.candidate(i) for i in range(plan.k)]
    assert all(cands) and len(set(cands)) == plan.k
    lines = [S.pmkid_line(PLANT_PSK, e, m, b"\x02\x5b" + n.to_bytes(4, "big")) for n, (e, m) in enumerate(nets)]
    return {"plan": plan, "nets": nets, "lines": lines, "cands": cands,
            "essid_of": [nets[plan.net_of(i)][0] for i in range(plan.k)]}


def check_case():
    """CHECK_JOBS PMKID jobs of one key each, every key its own, ESSID lengths cycling through CHECK_LENGTHS."""
    essids = [by_len(x) for x in CHECK_LENGTHS]
    return [(essids[j % len(essids)], b"check-path-key-%04d" % j) for j in range(CHECK_JOBS)]


def requests(cus):
    """{table name: [(essid, [psk])]}: every PMK the file asks the oracle for."""
    qc, gc, pc = queue_case(cus), group_case(cus), prio_cases(cus)
    req = {"slots": [(e, [psk(v) for v in slot_values()]) for e in SLOT_ESSIDS],
           "sweep": [(e, [psk(v) for v in sweep_values()]) for e in ESSIDS],
           "queue": [(qc["essid"], [psk(qc["first"] + s) for s in qc["sample"]])],
           "groups": [(e, [psk(gc["first"] + s) for s in pos]) for e, pos in zip(gc["essids"], gc["sample"])],
           "prio_one": [(pc["one"]["essid"], [psk(pc["one"]["first"] + s) for s in pc["one"]["sample"]])],
           "prio_mg": [(e, [psk(pc["mg"]["first"] + s) for s in pos])
                       for e, pos in zip(pc["mg"]["essids"], pc["mg"]["sample"])],
           "check": [(e, [k for ee, k in check_case() if ee == e]) for e in sorted({e for e, _ in check_case()})]}
    for rules in (False, True):
        ac = assoc_case(rules)
        by = {}
        for e, c in zip(ac["essid_of"], ac["cands"]):
            by.setdefault(e, []).append(c)
        req["assoc_rules" if rules else "assoc_plain"] = sorted(by.items())
    return req


# ---------------------------------------------------------------------------------------------------------------
# the reference tables
# ---------------------------------------------------------------------------------------------------------------
def words_of(pmks):
    """32-byte PMKs -> uint32[8][n]."""
    raw = np.frombuffer(b"".join(pmks), dtype=">u4").astype(np.uint32)
    return raw.reshape(len(pmks), 8).T.copy()


class Tables:
    """The oracle's PMKs, keyed (essid, psk); `names` maps a table to its keys."""

    def __init__(self, cus, threads=8):
        self.cus, self.pmk, self.names = cus, {}, {}
        t = time.perf_counter()
        for name, rows in requests(cus).items():
            self.names[name] = [(e, k) for e, keys in rows for k in keys]
            for e, keys in rows:
                new = [k for k in dict.fromkeys(keys) if (e, k) not in self.pmk]
                raw = O.c_pbkdf2_many(new, e, threads=threads)
                for i, k in enumerate(new):
                    self.pmk[(e, k)] = raw[32 * i:32 * i + 32]
        self.seconds = time.perf_counter() - t
        assert len(self.pmk) <= MAX_PMKS, len(self.pmk)

    def words(self, essid, psks):
        return words_of([self.pmk[(essid, k)] for k in psks])

    def numeric(self, essid, values):
        return self.words(essid, [psk(v) for v in values])


def tables(cus):
    """The session's tables: read from the parent's pickle in a forced-build child, else computed."""
    path = os.environ.get(FIXTURE_ENV)
    if path:
        with open(path, "rb") as f:
            t = pickle.load(f)
        assert t.cus == cus
        return t
    return Tables(cus, threads=min(16, os.cpu_count() or 8))


# ---------------------------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------------------------
def compare(got, want, ids, prev=None, shown=4):
    """got, want: uint32[8][n]; ids[j]: what names column j in a message (a slot number, or (slot, candidate)).
    Returns '' when every word of every column agrees, else a message that counts the differing columns and names the
    first `shown`: their ids, the words that differ, what was read and what was expected, and -- given prev, the
    buffer as it was read before the derive -- whether the column still holds those words (a lane that never wrote)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.ndim != 2 or got.shape[0] != 8 or got.shape[1] != len(ids):
        return "shapes differ: got %s, want %s, %d ids" % (got.shape, want.shape, len(ids))
    bad = np.flatnonzero((got != want).any(axis=0))
    if not len(bad):
        return ""
    stale = [] if prev is None else [int(j) for j in bad if (got[:, j] == np.asarray(prev)[:, j]).all()]
    out = ["%d of %d PMKs differ" % (len(bad), got.shape[1])]
    if prev is not None:
        out.append("%d of them stale (the words the buffer held before the derive)" % len(stale))
    for j in bad[:shown]:
        w = np.flatnonzero(got[:, j] != want[:, j])
        out.append("%s%s: words %s got %s want %s" % (
            ids[j], " stale" if j in stale else "", [int(k) for k in w],
            " ".join("%08x" % x for x in got[w, j]), " ".join("%08x" % x for x in want[w, j])))
    return "; ".join(out)


# ---------------------------------------------------------------------------------------------------------------
# deliberately wrong models
# ---------------------------------------------------------------------------------------------------------------
def _f(key, first_msg, iters=4096):
    """PBKDF2's F with the first HMAC message spelled out: U_1 = HMAC(key, first_msg), T = U_1 ^ ... ^ U_iters."""
    key = key + bytes(64 - len(key)) if len(key) <= 64 else hashlib.sha1(key).digest() + bytes(44)
    inner, outer = hashlib.sha1(bytes(c ^ 0x36 for c in key)), hashlib.sha1(bytes(c ^ 0x5c for c in key))

    def mac(msg):
        i = inner.copy()
        i.update(msg)
        o = outer.copy()
        o.update(i.digest())
        return o.digest()
    u = mac(first_msg)
    t = int.from_bytes(u, "big")
    for _ in range(iters - 1):
        u = mac(u)
        t ^= int.from_bytes(u, "big")
    return t.to_bytes(20, "big")


def model_right(key, essid, neighbour):
    return (_f(key, essid + b"\0\0\0\1") + _f(key, essid + b"\0\0\0\2"))[:32]


def model_block2_salt1(key, essid, neighbour):
    """Output block 2 derived from block 1's salt blocks: both lanes of a slot read blk 0."""
    t1 = hashlib.pbkdf2_hmac("sha1", key, essid, 4096, 20)
    return (t1 + t1)[:32]


def model_word7_dropped(key, essid, neighbour):
    """store_block writes words 5 and 6 of block 2 only; word 7 stays zero."""
    return hashlib.pbkdf2_hmac("sha1", key, essid, 4096, 32)[:28] + bytes(4)


def model_int_le(key, essid, neighbour):
    """INT(i) written little-endian into the salt block."""
    return (_f(key, essid + b"\1\0\0\0") + _f(key, essid + b"\2\0\0\0"))[:32]


def model_4095(key, essid, neighbour):
    """One iteration short."""
    return hashlib.pbkdf2_hmac("sha1", key, essid, 4095, 32)


def model_neighbour_salt(key, essid, neighbour):
    """The salt entry of the group next door (gsalt[2 * (c + 1)], or a neighbouring lane's sref)."""
    return hashlib.pbkdf2_hmac("sha1", key, neighbour, 4096, 32)


WRONG = {"block2_salt1": model_block2_salt1, "word7_dropped": model_word7_dropped, "int_le": model_int_le,
         "4095": model_4095, "neighbour_salt": model_neighbour_salt}
