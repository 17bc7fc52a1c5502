"""Plans for the check-path recall tests (CPU only; imports no GPU code).

The server check path (dwpa_check_m22000 / dwpa_check_batch) fails silently in one direction: a (key, attempt) item the
verifier drops is reported as "wrong password".  Which lane verifies an item follows from its key position in the job
and its index in the line's attempt list, so a plan here plants a hit at EVERY attempt index of a nonce window, at
chosen key positions of one shared key list, for keyver 1, 2 and 3 and both nonce orders (the order decides which
words of the PRF message the attempt patches).  A job is "the PSK is key number `pos`, the MIC verifies at attempt
(off, endian)"; its expected result comes from the C oracle, called with the one PSK and its PMK, and must be the
planted attempt -- an assert, so an unlucky seed fails loudly and no case is ever left out.

Every plan shares one ESSID and one list of K distinct keys among its jobs: the library derives K PMKs per call and
gathers them into K x jobs slots.

  plan(name) -> {"name", "essid", "keys", "pmks", "jobs": [(line, keys, pmk, nc)], "exp": [result or False],
                 "key_index": [pos or None], "meta": [(keyver, pos, attempt index or tag, swap)]}
"""
import functools
import os
import random
from concurrent.futures import ThreadPoolExecutor

from oracle import oracle as O
from tests import synth as S

THREADS = min(16, os.cpu_count() or 8)
STRIDE = 16  # every STRIDE-th job also gets the oracle's whole check: full key list, derive included
ATTEMPTS = {28: 61, 30: 65, 128: 261, 258: 521}  # nc -> attempts; 64 is the verifiers' switch (ATT_PARALLEL_MIN)
KEYVERS = (1, 2, 3)

# plan -> (nc, K, key positions).  40 keys: attempt-parallel segments of 16 + 16 + 8 keys with the early exit on, one
# segment of 40 with it off.  The reduced *_host plans run through the host backend on the CPU.
ITEMS = {"items_261": (128, 40, (0, 1, 15, 16, 17, 39)),
         "items_65": (30, 40, tuple(range(40))),
         "items_61": (28, 40, tuple(range(40))),
         "items_521": (258, 20, (0, 15, 16, 19)),
         "items_261_host": (128, 6, (0, 5)),
         "items_65_host": (30, 6, (0, 5)),
         "items_61_host": (28, 6, (0, 5))}
CALLER_PMK_ATTEMPTS = (0, 137, 520)  # items_521: jobs at position 0 that hand over the PMK (x keyver)

# stored ANONCE tail, planted offset, planted endian: the attempt the oracle must report
TAILS = (("ffffffff", 1, "LE"),   # LE and BE +1 both write 00000000: two attempts match, PHP's first (LE) is reported
         ("00000000", -1, "LE"),  # the same downwards: both write ffffffff
         ("000000ff", 1, "BE"),   # the carry leaves the low byte
         ("ff000000", 1, "LE"),
         ("feffffff", 2, "LE"),   # wraps 32 bits
         ("fffffffe", 2, "BE"))
TAIL_POSITIONS = (0, 15, 16, 39)


def attempts(nc):
    """The attempt list of a window in PHP's order (common.php:250-300): the stored nonce, then +k, -k little endian
    and +k, -k big endian for k = 1 .. halfnc."""
    halfnc = (nc >> 1) + 1
    out = [(0, None)]
    for k in range(1, halfnc + 1):
        out += [(k, "LE"), (-k, "LE"), (k, "BE"), (-k, "BE")]
    assert len(out) == 1 + 4 * halfnc and len(set(out)) == len(out)
    return out


for _nc, _n in ATTEMPTS.items():
    assert len(attempts(_nc)) == _n


def line_swap(line):
    """PHP's `swap` of an EAPOL line: ANONCE goes first in the PRF message (the attempt patches message bytes 28..31
    of the nonce pair) unless SNONCE sorts before it by its first 6 bytes (then bytes 60..63)."""
    f = line.split(b"*")
    anonce, eapol = bytes.fromhex(f[6].decode()), bytes.fromhex(f[7].decode())
    return not O.php_strncmp(eapol[17:49], anonce, 6) < 0


def _nonces(rng, swap, tail=None):
    an, sn = rng.randbytes(32), rng.randbytes(32)
    if tail is not None:
        an = an[:28] + tail
    c = S._cmp6(sn, an)
    assert c != 0
    if (c > 0) != swap:
        an, sn = sn[:28] + an[28:], an[:28] + sn[28:]
    return an, sn


def _keys(rng, n):
    keys = []
    while len(keys) < n:
        k = S.fast_psk(rng)
        if k not in keys and not k.startswith(b"$HEX["):
            keys.append(k)
    return keys


def _line(rng, essid, psk, pmk, kv, off, endian, swap, tail=None):
    an, sn = _nonces(rng, swap, tail)
    line = S.eapol_line(psk, essid, rng.randbytes(6), rng.randbytes(6), an, sn, kv, off, endian or "LE",
                        mp=rng.choice((0x00, 0x80, 0x02)), eapol_len=rng.choice((121, 123, 151)), the_pmk=pmk, rng=rng)
    assert line_swap(line) == swap
    return line


class _Builder:
    def __init__(self, name, seed, nkeys):
        self.name = name
        self.rng = random.Random(seed)
        self.essid = b"check-recall-" + name.encode()
        assert len(self.essid) <= 32
        self.keys = _keys(self.rng, nkeys)
        raw = O.c_pbkdf2_many(self.keys, self.essid, threads=THREADS)
        self.pmks = [raw[32 * i:32 * i + 32] for i in range(nkeys)]
        self.rows = []  # (line, pos, nc, want, caller_pmk, meta, psk, pmk)

    def add(self, kv, pos, nc, off, endian, swap, want, tag, tail=None, caller_pmk=False, outsider=False):
        """want: the (off, endian) the oracle must report for the PSK alone, None for a miss."""
        if outsider:  # a PSK that is not in the list: the line verifies, the job must miss
            psk = b"not-in-the-list-" + bytes([0x41 + kv])
            assert psk not in self.keys
            pmk = O.c_pbkdf2(psk, self.essid)
        else:
            psk, pmk = self.keys[pos], self.pmks[pos]
        line = _line(self.rng, self.essid, psk, pmk, kv, off, endian, swap, tail)
        self.rows.append((line, pos, nc, want, caller_pmk, (kv, pos, tag, swap), psk, pmk, outsider))

    def finish(self):
        rows, keys = self.rows, self.keys
        assert len(set(keys)) == len(keys) and len({r[0] for r in rows}) == len(rows)

        def alone(r):  # the PSK and its PMK handed over: no derive
            return O.c_check_key_m22000(r[0], [r[6]], r[7], r[2])

        def whole(r):
            return O.c_check_key_m22000(r[0], keys, self.pmks[0] if r[4] else False, r[2])

        with ThreadPoolExecutor(THREADS) as ex:
            one = list(ex.map(alone, rows))
            sel = [i for i, r in enumerate(rows) if i % STRIDE == 0 or r[4] or r[8]]
            full = dict(zip(sel, ex.map(lambda i: whole(rows[i]), sel)))
        jobs, exp, key_index, meta = [], [], [], []
        for i, (line, pos, nc, want, caller, m, psk, pmk, outsider) in enumerate(rows):
            if outsider:  # the line is sound (it verifies with its own PSK); no key of the list is that PSK
                assert want is not None and one[i] == [psk, want[0], want[1], pmk], (self.name, m, one[i])
                e = False
            elif want is None:
                assert one[i] is False, (self.name, m, one[i])
                e = False
            else:
                e = [psk, want[0], want[1], pmk]
                assert one[i] == e, (self.name, m, one[i][:3] if one[i] else one[i])
            if i in full:
                assert full[i] == e, (self.name, m, "whole oracle call")
            jobs.append((line, keys, self.pmks[0] if caller else False, nc))
            exp.append(e)
            key_index.append(pos if e else None)
            meta.append(m)
        return {"name": self.name, "essid": self.essid, "keys": keys, "pmks": self.pmks, "jobs": jobs, "exp": exp,
                "key_index": key_index, "meta": meta}


def _items(name):
    nc, nkeys, positions = ITEMS[name]
    b = _Builder(name, 0xC4EC0 + nc, nkeys)
    att = attempts(nc)
    for kv in KEYVERS:
        for pos in positions:
            for ai, (off, endian) in enumerate(att):
                b.add(kv, pos, nc, off, endian, bool(b.rng.getrandbits(1)), (off, endian), ai)
    if name == "items_521":  # the caller's PMK belongs to key 0 (PHP uses $pmk for the first key only)
        for kv in KEYVERS:
            for ai in CALLER_PMK_ATTEMPTS:
                b.add(kv, 0, nc, att[ai][0], att[ai][1], ai % 2 == 0, att[ai], ai, caller_pmk=True)
    p = b.finish()
    n = len(att) * len(positions) * 3 + (9 if name == "items_521" else 0)
    assert len(p["jobs"]) == n
    if name != "items_521":  # both nonce orders among the jobs of every (keyver, position), read from the lines
        seen = {(kv, pos, line_swap(j[0])) for j, (kv, pos, _, _) in zip(p["jobs"], p["meta"])}
        assert seen == {(kv, pos, sw) for kv in KEYVERS for pos in positions for sw in (False, True)}
    return p


def _misses():
    """One window past each list (+-(halfnc + 1), both endians) per keyver and verifier: nc = 28 is key-parallel,
    nc = 128 attempt-parallel; and per verifier one job whose line verifies with a PSK the list does not hold."""
    b = _Builder("misses", 0xC4EC1, 40)
    for nc in (28, 128):
        past = (nc >> 1) + 2
        for kv in KEYVERS:
            for n, (off, endian) in enumerate(((past, "LE"), (-past, "LE"), (past, "BE"), (-past, "BE"))):
                b.add(kv, (0, 15, 16, 39)[n], nc, off, endian, bool(n & 1) ^ (kv == 2), None, "past%+d%s" % (off, endian))
        b.add(2 if nc == 28 else 3, 0, nc, 3, "BE", True, (3, "BE"), "outsider", outsider=True)
    p = b.finish()
    assert len(p["jobs"]) == 26 and not any(p["exp"])
    return p


def _tails():
    b = _Builder("tails", 0xC4EC2, 40)
    n = 0
    for tail, off, endian in TAILS:
        for kv in KEYVERS:
            for swap in (False, True):
                b.add(kv, TAIL_POSITIONS[n % 4], 128, off, endian, swap, (off, endian), tail, tail=bytes.fromhex(tail))
                n += 1
    p = b.finish()
    assert len(p["jobs"]) == 36 and all(p["exp"])
    return p


def _double_full(name, copies):
    """`copies` copies of the PSK as keys (separate slots, one PMK), stored tail ffffffff, +1 planted: the LE and the
    BE attempt of every slot match.  The first key and PHP's first attempt (LE) win."""
    b = _Builder(name, 0xC4EC3, 1)
    b.add(2, 0, 128, 1, "LE", False, (1, "LE"), "ffffffff", tail=b"\xff" * 4)
    p = b.finish()
    line, keys, pmk, nc = p["jobs"][0]
    p["jobs"][0] = (line, keys * copies, pmk, nc)
    both = O.c_check_key_m22000(S.eapol_line(keys[0], p["essid"], b"\1" * 6, b"\2" * 6, b"\3" * 28 + b"\xff" * 4,
                                             b"\4" * 32, 2, 1, "BE", the_pmk=p["pmks"][0]), keys, p["pmks"][0], 128)
    assert both and both[1:3] == [1, "LE"]  # planted big endian, found little endian: the two attempts are one value
    return p


@functools.lru_cache(maxsize=None)
def plan(name):
    if name in ITEMS:
        return _items(name)
    if name == "misses":
        return _misses()
    if name == "tails":
        return _tails()
    if name == "double_full":
        return _double_full(name, 300)
    if name == "double_full_host":
        return _double_full(name, 20)
    raise KeyError(name)


def subset(p, keyvers):
    """The plan cut down to the jobs of these keyvers (same key list, so the same PMKs)."""
    idx = [i for i, m in enumerate(p["meta"]) if m[0] in keyvers]
    q = dict(p)
    for f in ("jobs", "exp", "key_index", "meta"):
        q[f] = [p[f][i] for i in idx]
    return q


def mismatches(p, got, key_index):
    """Jobs whose result or key_index differs from the plan: [(job, (keyver, position, attempt, swap), got, exp)]."""
    assert len(got) == len(key_index) == len(p["jobs"])
    return [(i, p["meta"][i], got[i], key_index[i], p["exp"][i], p["key_index"][i]) for i in range(len(got))
            if got[i] != p["exp"][i] or key_index[i] != p["key_index"][i]]


def describe(p, bad):
    """What an assert shows of a mismatch list: counts per keyver and the first few (keyver, position, attempt, swap)
    with what came back (PMKs cut short)."""
    def short(r):
        return r if r is False else [r[0][:12], r[1], r[2], r[3][:4].hex()]
    per_kv = {kv: sum(1 for b in bad if b[1][0] == kv) for kv in KEYVERS}
    return (p["name"], "%d of %d jobs differ" % (len(bad), len(p["jobs"])), per_kv,
            [(b[1], "got", short(b[2]), b[3], "exp", short(b[4]), b[5]) for b in bad[:5]])


def run_batch(p):
    """One dwpa_check_batch call over the plan's jobs: (results, key_index per job)."""
    import dwpa_amd
    from dwpa_amd import _lib as L
    b = dwpa_amd.BatchJobs(p["jobs"])
    b.run()
    return b.results(), [int(b.out[i].key_index) if b.rcs[i] == L.DWPA_HIT else None for i in range(b.n)]
