"""Plans for the hashcat-nonce-window recall tests (CPU only; imports no GPU code).

A scan in DWPA_NC_HASHCAT mode tries the stored ANONCE, then +-1..+-nec in little and big endian, cut down by the
line's message-pair bits, and verifies every attempt key-parallel from per-attempt KW blocks.  An attempt that is
dropped, patched into the wrong word, read from the wrong KW block or mapped to the wrong (nc, endian) fails silently:
"PSK not in the dictionary".  A plan here is the line list of ONE Scan(lines, nc=nec, nc_mode=DWPA_NC_HASHCAT): a hit
planted at chosen attempt indices of the window, for keyver 1, 2 and 3 and both nonce orders (the first corrected byte
is PRF-message byte 63 / 95 for keyver 1 and 2 -- two words, for 63 two blocks -- and 64 / 96 for keyver 3, one
aligned word), under chosen message pairs, and lines planted just outside the window or in an endian the message pair
forbids, which must miss.

The model is restated here, not read from the library: hashcat_attempts(nec, mp) is the ordered attempt list, and
expected(line, nec, true_tail) the first attempt of it whose 4 written bytes equal bytes 28..31 of the ANONCE the MIC
was made with.  The reference is the C oracle, called with the row's one PSK and its PMK, as an assert (no row is
ever skipped): where the message pair allows both endians and the plant lies inside +-nec it must report exactly the
model's (offset, endian) -- PHP's window +-(nec + 1) at nc = 2 * nec has the same order, see attempts equality in
tests/test_nonce_plan.py -- and for every other row it must still find the PSK, at an attempt that writes the true
bytes: the line is genuine, and the miss (or the other attempt index) is the window's doing.

All plans share two ESSIDs (rows alternate, so run() is a multi-group launch), one PMKID control line per ESSID, and
one dictionary of 130 distinct kept words (two waves + 2 lanes) with filtered-out words between them (ids != slots).
"No PSK twice within an ESSID" holds for the dictionary: a line is hit by exactly one candidate.  A row's PSK is the
kept word at POS[n % 6], n counting the rows of its (keyver, nonce order, hit or miss).

  plan(name) -> {"name", "nec", "lines", "words", "kept", "rows" [dict], "controls" [(line index, position)],
                 "hits" {(line, cand, nc, endian, pmk)}, "classes" {keyver}}
"""
import functools
import hashlib
import hmac
import os
import random
import struct
from concurrent.futures import ThreadPoolExecutor

from oracle import oracle as O
from tests import check_recall as C
from tests import synth as S

THREADS = min(16, os.cpu_count() or 8)
STRIDE = C.STRIDE  # every STRIDE-th row also gets the oracle's whole call, derive included
KEYVERS = (1, 2, 3)
ESSIDS = (b"nonce", b"nonce-recall-the-longest-ssid-32")
NKEPT = 130
POS = (0, 63, 64, 127, 128, 129)  # kept-word positions: both ends of the two full waves, and the 2 lanes after them
CONTROL_POS = (63, 64)  # the PMKID control of ESSID 0 lies inside the first 64-slot wave, that of ESSID 1 outside
JUNK = (b"", b"short-7", b"j" * 64, b"k" * 65, b"l" * 300)  # outside the 8..63 filter
EAPOL_LENS = (121, 123, 151)
EAPOL_LENS_KV3 = (121, 123, 151, 112, 128)  # 112, 128: the CMAC's last block is complete
MPS = (0x00, 0x80, 0x02)
PLANS = ("every_8", "every_16", "wide_64", "small_0", "small_1", "edges_8", "edges_16", "message_pair", "tails",
         "short_anonce")
WIDE_INDICES = (0, 1, 63, 64, 65, 255, 256)
MP_MASKS = (0x10, 0x20, 0x40, 0x60, 0x30, 0x90, 0xa0)
MP_PLANTS = ((0, None), (3, "LE"), (-3, "BE"), (8, "LE"), (-8, "BE"))
SHORT_LENS = (20, 31)
SHORT_TWIN = {4: 2}  # short ANONCE, nec 2: planted attempt index -> the earlier attempt with the same message
assert len(ESSIDS[1]) == 32 and all(0x20 <= c <= 0x7e and c != 0x3a for e in ESSIDS for c in e)


# ---------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------
def hashcat_attempts(nec, mp):
    """[(off, endian)] in the order a DWPA_NC_HASHCAT scan tries them: the stored nonce; then, unless message-pair
    bit 0x10 is set, for k = 1..nec the LE pair (unless of bits 0x20 / 0x40 only 0x40 is set) and the BE pair (unless
    only 0x20 is set)."""
    out = [(0, None)]
    le = not (mp & 0x40 and not mp & 0x20)
    be = not (mp & 0x20 and not mp & 0x40)
    if not mp & 0x10:
        for k in range(1, nec + 1):
            if le:
                out += [(k, "LE"), (-k, "LE")]
            if be:
                out += [(k, "BE"), (-k, "BE")]
    assert len(out) == (1 if mp & 0x10 else 1 + 2 * nec * (le + be)) and len(set(out)) == len(out)
    return out


def both_endians(mp):
    """The message pair cuts nothing from the window."""
    return not mp & 0x10 and bool(mp & 0x20) == bool(mp & 0x40)


def written(stored, off, endian):
    """The 4 bytes attempt (off, endian) writes over a stored ANONCE tail."""
    if endian is None:
        assert off == 0
        return stored
    fmt = "<I" if endian == "LE" else ">I"
    return struct.pack(fmt, (struct.unpack(fmt, stored)[0] + off) & 0xFFFFFFFF)


def line_fields(line):
    """(keyver, stored ANONCE, EAPOL frame, message pair) of an EAPOL line."""
    f = line.split(b"*")
    eapol = bytes.fromhex(f[7].decode())
    return struct.unpack(">H", eapol[5:7])[0] & 3, bytes.fromhex(f[6].decode()), eapol, int(f[8], 16)


def expected(line, nec, true_tail):
    """(index, off, endian) of the first attempt that writes `true_tail`, bytes 28..31 of the ANONCE the MIC was made
    with; None: no attempt of the window does."""
    _, anonce, _, mp = line_fields(line)
    assert len(anonce) == 32
    for i, (off, endian) in enumerate(hashcat_attempts(nec, mp)):
        if written(anonce[28:], off, endian) == true_tail:
            return i, off, endian
    return None


def short_messages(line, nec):
    """A line with an ANONCE under 32 bytes: the nonce part of every attempt's PRF message, the library's own
    reading in hashcat mode (parity unpinned).  The correction base is 0 (PHP's unpack fails), attempt a writes
    pack(endian, off) with PHP's substr_replace clamping at byte 28 (ANONCE first) or 60 of the ORIGINAL nonce pair:
    nothing is carried from attempt to attempt."""
    _, anonce, eapol, mp = line_fields(line)
    assert len(anonce) < 32
    snonce = eapol[17:49]
    if O.php_strncmp(snonce, anonce, 6) < 0:
        n0, patch = snonce + anonce, 60
    else:
        n0, patch = anonce + snonce, 28
    return [O.substr_replace(n0, written(b"\0" * 4, off, endian), patch, 4)
            for off, endian in hashcat_attempts(nec, mp)]


def mic_of(line, pmk, n):
    """The MIC of an EAPOL line for the nonce part `n` of the PRF message, from oracle/oracle.py's primitives."""
    f = line.split(b"*")
    ap, sta = bytes.fromhex(f[3].decode()), bytes.fromhex(f[4].decode())
    keyver, _, eapol, _ = line_fields(line)
    m = ap + sta if O.php_strncmp(ap, sta, 6) < 0 else sta + ap
    if keyver == 3:
        ptk = hmac.new(pmk, b"\1\0Pairwise key expansion" + m + n + b"\x80\1", hashlib.sha256).digest()
        return O.omac1_aes_128(eapol, ptk[:16])
    ptk = hmac.new(pmk, b"Pairwise key expansion\0" + m + n + b"\0", hashlib.sha1).digest()
    return hmac.new(ptk[:16], eapol, hashlib.md5 if keyver == 1 else hashlib.sha1).digest()[:16]


def expected_short(line, nec, pmk):
    """(index, off, endian) of the first attempt of a short-ANONCE line whose message gives the stored MIC."""
    mic = bytes.fromhex(line.split(b"*")[2].decode())
    att = hashcat_attempts(nec, line_fields(line)[3])
    for i, n in enumerate(short_messages(line, nec)):
        if mic_of(line, pmk, n) == mic:
            return (i,) + att[i]
    return None


def _plain(b):
    return b if all(0x20 <= c <= 0x7E and c != 0x3A for c in b) and not b.startswith(b"$HEX[") \
        else b"$HEX[" + b.hex().encode() + b"]"


def record(line, psk):
    """The outfile record of a cracked line: MIC or PMKID : AP : STA : ESSID : PSK."""
    f = line.split(b"*")
    return b":".join([f[2], f[3], f[4], _plain(bytes.fromhex(f[5].decode())), _plain(psk)])


# ---------------------------------------------------------------------------------------------------------------
# the shared dictionary and its PMKs
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dictionary():
    """{"words", "kept" (dictionary index of every kept word), "psk" {position: word}, "pmk" {(essid index,
    position): PMK}}: PMKs are derived once per (ESSID, word), by the C oracle."""
    rng = random.Random(0x40CE)
    words, kept, seen = [JUNK[1]], [], set()
    while len(kept) < NKEPT:  # the first kept word has 8 bytes, the last 63
        n = {0: 8, NKEPT - 1: 63}.get(len(kept)) or rng.randint(8, 63)
        w = bytes(rng.randint(0x21, 0x7E) for _ in range(n))
        if w in seen or w.startswith(b"$HEX["):
            continue
        seen.add(w)
        kept.append(len(words))
        words.append(w)
        if len(kept) % 9 == 0 and len(kept) < NKEPT:
            words.append(JUNK[len(kept) // 9 % len(JUNK)])
    assert len(kept) == NKEPT and [i for i, w in enumerate(words) if 8 <= len(w) <= 63] == kept
    assert kept[0] != 0 and kept[-1] == len(words) - 1 and {words[i] for i in range(len(words))
                                                            if i not in kept} == set(JUNK)
    assert len({words[i] for i in kept}) == NKEPT  # no PSK twice: a line is hit by one candidate only
    used = sorted(set(POS) | set(CONTROL_POS))
    psk = {pos: words[kept[pos]] for pos in used}
    pmk = {}
    for e, essid in enumerate(ESSIDS):
        raw = O.c_pbkdf2_many([psk[pos] for pos in used], essid, threads=THREADS)
        for k, pos in enumerate(used):
            pmk[e, pos] = raw[32 * k:32 * k + 32]
    return {"words": words, "kept": kept, "psk": psk, "pmk": pmk}


# ---------------------------------------------------------------------------------------------------------------
# building a plan
# ---------------------------------------------------------------------------------------------------------------
def _short_line(rng, essid, psk, pmk, kv, alen, swap, eapol_len, nec, index):
    """As tests/golden/make_golden.py short_anonce_line, for every keyver: an ANONCE of `alen` bytes, the MIC made
    for attempt `index` of short_messages."""
    an, sn = C._nonces(rng, swap)
    an = an[:alen]
    ap, sta = rng.randbytes(6), rng.randbytes(6)
    frame = S.eapol_line(psk, essid, ap, sta, b"\0" * 32, sn, kv, eapol_len=eapol_len, the_pmk=pmk, rng=rng)
    f = frame.split(b"*")
    f[6], f[8] = an.hex().encode(), b"00"
    assert (not O.php_strncmp(sn, an, 6) < 0) == swap
    line = b"*".join(f)
    f[2] = mic_of(line, pmk, short_messages(line, nec)[index]).hex().encode()
    return b"*".join(f)


class _Builder:
    def __init__(self, name, nec, seed):
        self.name, self.nec = name, nec
        self.rng = random.Random(seed)
        self.d = dictionary()
        self.rows = []
        self.count = {}

    def add(self, kv, swap, plant, hit, tag, mp=None, tail=None, short=None):
        """plant: (off, endian) of the attempt the MIC is made for, or for short=ANONCE length its attempt index.
        hit: whether the plan means this row to be found (the model decides; finish() asserts they agree)."""
        i = len(self.rows)
        e = i % 2  # rows alternate between the ESSIDs
        n = self.count[kv, swap, hit] = self.count.get((kv, swap, hit), -1) + 1
        pos = POS[n % 6]
        psk, pmk = self.d["psk"][pos], self.d["pmk"][e, pos]
        lens = EAPOL_LENS_KV3 if kv == 3 else EAPOL_LENS
        eapol_len = lens[n % len(lens)]
        if short:
            line = _short_line(self.rng, ESSIDS[e], psk, pmk, kv, short, swap, eapol_len, self.nec, plant)
            want, true_tail = expected_short(line, self.nec, pmk), None
        else:
            off, endian = plant
            an, sn = C._nonces(self.rng, swap, tail)
            mp = MPS[i % 3] if mp is None else mp
            line = S.eapol_line(psk, ESSIDS[e], self.rng.randbytes(6), self.rng.randbytes(6), an, sn, kv, off,
                                endian or "LE", mp=mp, eapol_len=eapol_len, the_pmk=pmk, rng=self.rng)
            assert C.line_swap(line) == swap
            true_tail = written(an[28:], off, endian)
            want = expected(line, self.nec, true_tail)
        assert (want is not None) == hit, (self.name, tag, want)
        self.rows.append({"line": line, "kv": kv, "swap": swap, "essid": e, "pos": pos, "psk": psk, "pmk": pmk,
                          "mp": line_fields(line)[3], "eapol_len": eapol_len, "plant": plant, "want": want,
                          "true_tail": true_tail, "short": short, "tag": tag})

    def finish(self):
        rows, d, nec = self.rows, self.d, self.nec
        lines = [r["line"] for r in rows]
        controls = []
        for e, pos in enumerate(CONTROL_POS):
            controls.append((len(lines), pos))
            lines.append(S.pmkid_line(d["psk"][pos], ESSIDS[e], self.rng.randbytes(6), self.rng.randbytes(6),
                                      the_pmk=d["pmk"][e, pos]))
        assert len(set(lines)) == len(lines)

        def alone(r):  # the PSK and its PMK handed over: no derive
            return O.c_check_key_m22000(r["line"], [r["psk"]], r["pmk"], 2 * nec)

        def whole(r):
            return O.c_check_key_m22000(r["line"], [r["psk"]], False, 2 * nec)

        with ThreadPoolExecutor(THREADS) as ex:
            one = list(ex.map(alone, rows))
            sel = range(0, len(rows), STRIDE)
            full = dict(zip(sel, ex.map(lambda i: whole(rows[i]), sel)))
            ctl = list(ex.map(lambda c: O.c_check_key_m22000(lines[c[0]], [d["psk"][c[1]]], False, 2 * nec), controls))
        for i, (r, o) in enumerate(zip(rows, one)):
            what = (self.name, i, r["tag"], o[:3] if o else o)
            if r["short"]:  # PHP carries $n from the first attempt on: the oracle can confirm index 0 only
                if r["plant"] == 0:
                    assert o == [r["psk"], 0, None, r["pmk"]], what
            else:
                # the line is genuine: the oracle finds the PSK, at an attempt that writes the true bytes
                assert o and o[0] == r["psk"] and o[3] == r["pmk"], what
                assert written(line_fields(r["line"])[1][28:], o[1], o[2]) == r["true_tail"], what
                if both_endians(r["mp"]) and r["want"] is not None:  # the same ordered window: the same attempt
                    assert (o[1], o[2]) == r["want"][1:], what
            if i in full:
                assert full[i] == o, what + ("whole oracle call",)
        for (k, pos), o in zip(controls, ctl):
            assert o == [d["psk"][pos], None, None, d["pmk"][k - len(rows), pos]], (self.name, "control", k)
        hits = {(i, d["kept"][r["pos"]], r["want"][1], r["want"][2], r["pmk"]) for i, r in enumerate(rows) if r["want"]}
        hits |= {(k, d["kept"][pos], None, None, d["pmk"][k - len(rows), pos]) for k, pos in controls}
        return {"name": self.name, "nec": nec, "lines": lines, "words": d["words"], "kept": d["kept"], "rows": rows,
                "controls": controls, "hits": hits, "classes": {r["kv"] for r in rows}}


def _orders(k):
    """Both nonce orders, the first one alternating, so that neither ESSID goes with one order only."""
    return (False, True) if k % 2 == 0 else (True, False)


def _every(name, nec, indices):
    b = _Builder(name, nec, 0x40CE0 + nec)
    att = hashcat_attempts(nec, 0)
    assert len(att) == 1 + 4 * nec
    for ai in indices:
        for kv in KEYVERS:
            for swap in _orders(ai):
                b.add(kv, swap, att[ai], True, ai)
    p = b.finish()
    for r in p["rows"]:  # the reported attempt index is the planted one
        assert r["want"][0] == r["tag"] and r["mp"] in MPS, (name, r["tag"], r["want"])
    assert len(p["rows"]) == 6 * len(indices)
    return p


def _small(nec):
    """Every index of the 1- and the 5-attempt window, and one past it in both endians and directions."""
    b = _Builder("small_%d" % nec, nec, 0x40CE5 + nec)
    att = hashcat_attempts(nec, 0)
    assert len(att) == (1, 5)[nec]
    for ai in range(len(att)):
        for kv in KEYVERS:
            for swap in _orders(ai):
                b.add(kv, swap, att[ai], True, ai)
    for k, (off, endian) in enumerate(((nec + 1, "LE"), (-nec - 1, "LE"), (nec + 1, "BE"), (-nec - 1, "BE"))):
        for kv in KEYVERS:
            for swap in _orders(k):
                b.add(kv, swap, (off, endian), False, "past%+d%s" % (off, endian))
    p = b.finish()
    assert len(p["rows"]) == 6 * len(att) + 24
    return p


def _edges(nec):
    """+-nec found, +-(nec + 1) missed, in both endians."""
    b = _Builder("edges_%d" % nec, nec, 0x40CEE + nec)
    k = 0
    for mag, hit in ((nec, True), (nec + 1, False)):
        for endian in ("LE", "BE"):
            for off in (mag, -mag):
                for kv in KEYVERS:
                    for swap in _orders(k):
                        b.add(kv, swap, (off, endian), hit, "%+d%s" % (off, endian))
                k += 1
    p = b.finish()
    assert len(p["rows"]) == 48 and len(p["hits"]) == 24 + 2
    for r in p["rows"]:  # the last four indices of the window, by magnitude: LE+, LE-, BE+, BE-
        if r["want"]:
            assert r["want"][0] == 4 * nec - 3 + ("LE", "BE").index(r["plant"][1]) * 2 + (r["plant"][0] < 0)
    return p


def _message_pair():
    nec = 8
    b = _Builder("message_pair", nec, 0x40CEA)
    k = 0
    for mp in MP_MASKS:
        allowed = {e for _, e in hashcat_attempts(nec, mp)}
        for off, endian in MP_PLANTS:
            for kv in KEYVERS:
                for swap in _orders(k):
                    b.add(kv, swap, (off, endian), endian in allowed, "mp%02x%+d%s" % (mp, off, endian or ""), mp=mp)
            k += 1
    p = b.finish()
    assert len(p["rows"]) == len(MP_MASKS) * len(MP_PLANTS) * 6
    index = {(r["mp"], r["plant"]): r["want"] and r["want"][0] for r in p["rows"]}
    for mp in (0x10, 0x30, 0x90):  # only the stored nonce
        assert [index[mp, pl] for pl in MP_PLANTS] == [0, None, None, None, None]
    for mp in (0x20, 0xa0):  # LE only: index 1 + 2 (k - 1) + (0 for +k, 1 for -k)
        assert [index[mp, pl] for pl in MP_PLANTS] == [0, 5, None, 15, None]
    assert [index[0x40, pl] for pl in MP_PLANTS] == [0, None, 6, None, 16]  # BE only
    assert [index[0x60, pl] for pl in MP_PLANTS] == [0, 9, 12, 29, 32]  # both: 1 + 4 (k - 1) + ...
    return p


def _tails():
    nec = 8
    b = _Builder("tails", nec, 0x40CE7)
    k = 0
    for t, (tail, off, endian) in enumerate(C.TAILS):
        for mp in (0x00, 0x20, 0x40) if t < 2 else (0x00,):
            for kv in KEYVERS:
                for swap in _orders(k):
                    b.add(kv, swap, (off, endian), True, "%s-mp%02x" % (tail, mp), mp=mp, tail=bytes.fromhex(tail))
            k += 1
    p = b.finish()
    assert len(p["rows"]) == 36 + 24 and len(p["hits"]) == 60 + 2
    for r in p["rows"]:  # the LE and the BE attempt write one value: the first ALLOWED one is reported
        twin = r["tag"].startswith(("ffffffff", "00000000"))
        assert r["want"][1:] == (r["plant"][0], "BE" if twin and r["mp"] == 0x40 else r["plant"][1]), r["tag"]
        if twin:
            assert r["want"][0] == (1 if r["plant"][0] > 0 else 2)
    return p


def _short_anonce():
    nec = 2
    b = _Builder("short_anonce", nec, 0x40CE2)
    att = hashcat_attempts(nec, 0)
    assert len(att) == 9
    k = 0
    for alen in SHORT_LENS:
        for ai in range(len(att)):
            for kv in KEYVERS:
                for swap in _orders(k):
                    b.add(kv, swap, ai, True, "%d-%d" % (alen, ai), short=alen)
            k += 1
    p = b.finish()
    for r in p["rows"]:  # over a base of 0, -1 LE and -1 BE both write ffffffff: index 4 is reported as index 2
        at = SHORT_TWIN.get(r["plant"], r["plant"])
        assert r["want"] == (at,) + att[at], r["tag"]
    assert len(p["rows"]) == 2 * 9 * 6
    return p


@functools.lru_cache(maxsize=None)
def plan(name):
    if name in ("every_8", "every_16"):
        nec = int(name[6:])
        return _every(name, nec, range(1 + 4 * nec))
    if name == "wide_64":
        return _every(name, 64, WIDE_INDICES)
    if name in ("small_0", "small_1"):
        return _small(int(name[6:]))
    if name in ("edges_8", "edges_16"):
        return _edges(int(name[6:]))
    if name == "message_pair":
        return _message_pair()
    if name == "tails":
        return _tails()
    if name == "short_anonce":
        return _short_anonce()
    raise KeyError(name)


def hits_within(p, nkept):
    """The plan's hits when only the first `nkept` kept words are loaded."""
    return {h for h in p["hits"] if h[1] <= p["kept"][nkept - 1]}


def model_hits(rows, nec):
    """Row numbers the model finds in a window of +-nec (rows of any plan but short_anonce)."""
    return [i for i, r in enumerate(rows) if expected(r["line"], nec, r["true_tail"]) is not None]


def describe(p, got):
    """What an assert shows of a hit set that differs from the plan's: per missing / extra hit the row's keyver,
    nonce order, position and tag (PMKs cut short)."""
    def row(h):
        if h[0] >= len(p["rows"]):
            return ("control",) + h[:4]
        r = p["rows"][h[0]]
        return ("kv%d" % r["kv"], "swap" if r["swap"] else "noswap", "pos%d" % r["pos"], r["tag"]) + h[1:4] + \
            (h[4][:4].hex(),)
    missing, extra = sorted(p["hits"] - got), sorted(got - p["hits"])
    return (p["name"], "missing %d" % len(missing), [row(h) for h in missing[:6]], "extra %d" % len(extra),
            [row(h) for h in extra[:6]])
