"""Fixtures and a CPU model for the precision tests: a target that is almost right must never be reported (CPU only;
imports no GPU code and not the library).

The recall plans (check_recall.py, nonce_plan.py, fill_plan.py) pin "every true PSK is found".  Their lines are all
genuine, so a verifier that compared three of the four target words, 15 of the 16 bytes, or one word in the wrong byte
order would pass them: random decoys never land within a word of a target.  A fixture here is built over ONE PSK and
holds, per line kind (PMKID, EAPOL keyver 1, 2, 3):

  control      the true line; EAPOL: one per (frame length, planted correction)
  bit0..127    its control with bit b of the 16-byte PMKID / MIC flipped (bit 0 = 0x80 of byte 0, bit 127 = 0x01 of
               byte 15): the hex field is rewritten, nothing else differs from that control
  swap0..3     the control with target word w byte-swapped.  No one-bit flip can satisfy a comparer that reads a word
               in the wrong byte order (bswap(t ^ e) == t needs t ^ bswap(t) == bswap(e), and the left side is its own
               byte swap where a single bit is not), so the fixture carries these four lines for it
  long_*       an over-long target, on MACs of its own: the true 16 bytes + 4 more (a hit), the same with bit 127
               flipped (a miss), and the first with a bit of byte 17 flipped (a hit): exactly 16 bytes are compared.
               The oracle (PHP's strncmp(.., 16)) accepts the longer field for the PMKID and for the MIC of every key
               version, so the triple is built for all four kinds (tests/test_precision_plan.py asserts the acceptance)
  zero         a line whose target was made from the all-zero PMK (common.php:592 checks such lines with the PMK
               handed over): idle lanes of the key-parallel verifier compute exactly this value, and only their
               `active` / `mine` guards keep them quiet.  No candidate derives the zero PMK: always a miss

An EAPOL kind has two frames, one from each side of a MIC block boundary (keyver 1/2: 119 and 120 bytes, one HMAC
inner block or two; keyver 3: 112 and 121 bytes, a complete and an incomplete last CMAC block), and per frame one TRUE
ANONCE: the eight planted corrections move the STORED tail (true - off, in the attempt's endian), so every line of a
frame has the same MACs, frame and true MIC, and the attempt that would verify it lies at every residue mod 4 of the
attempt list in both endians (the host backend verifies keyver 1/2 attempts four at a time).  The attempt order is
nonce_plan.hashcat_attempts: PHP's window at nc is that list for nec = (nc >> 1) + 1.

Fixtures: "single" (one ESSID, corrections within +-5: nc = 8 in PHP's order and nec = 8 in hashcat's), "wide" (the same
with the corrections at +-30 and +-65, nc = 128: the attempt-parallel verifier), "multi" (the families spread over the
1-, 13- and 52-byte ESSIDs of the scan recall tests) and "digits" (an eight-digit PSK, for a mask window).

The model: expected() -- a control or long hit is found at its planted (nc, endian), everything else is missed -- and
weak_match(ignored_bits) / swapped_match(word), comparers with a defect, which tests/test_precision_plan.py shows the
fixture detects: each accepts a line the plan says must be missed.
"""
import functools
import random

from oracle import oracle as O
from tests import check_recall as C
from tests import nonce_plan as N
from tests import synth as S

KINDS = ("pmkid", 1, 2, 3)
PSK = b"Precision: near-miss PSK #1"
PSK_DIGITS = b"48151623"
MASK_DIGITS = b"?d?d?d?d?d?d?d?d"
ZERO_PMK = b"\0" * 32
ESSID_ONE = b"precision-one"
ESSID_DIGITS = b"precision-mask"
ESSIDS_MULTI = (b"R", b"recall-mid-13", bytes(0x41 + i % 26 for i in range(52)))  # test_gpu_recall.ESSIDS
FRAME_LENS = {1: (119, 120), 2: (119, 120), 3: (112, 121)}
# planted corrections: attempt indices 1, 2, 7, 8, 17, 18, 15, 20 of the 21-attempt list, 117..120 and 257..260 of the
# 261-attempt one: every residue mod 4, both endians, the window's last attempt included
PLANTS = {"narrow": ((1, "LE"), (-1, "LE"), (2, "BE"), (-2, "BE"), (5, "LE"), (-5, "LE"), (4, "BE"), (-5, "BE")),
          "wide": ((30, "LE"), (-30, "LE"), (30, "BE"), (-30, "BE"), (65, "LE"), (-65, "LE"), (65, "BE"), (-65, "BE"))}
NC = {"narrow": 8, "wide": 128}
FIXTURES = {"single": (PSK, (ESSID_ONE,), "narrow"), "wide": (PSK, (ESSID_ONE,), "wide"),
            "multi": (PSK, ESSIDS_MULTI, "narrow"), "digits": (PSK_DIGITS, (ESSID_DIGITS,), "narrow")}
NWORDS = 130
P_AT = (0, 63, 64, 129)  # first and last lane of a full wave, lanes 0 and 1 of the partial third wave
LONG_TAIL = bytes.fromhex("a5c3e1f0")
MISS = False  # the oracle's miss value (PHP's false)


def halfnc(nc):
    return (nc >> 1) + 1


# ---------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------
def expected(line_kind, is_control, plant=None):
    """What a correct checker reports for a fixture line whose PSK is among the keys: a control (or long-target hit)
    of an EAPOL kind its planted (nc, endian), a PMKID one (None, None); None (a miss) for everything else."""
    if not is_control:
        return None
    return (None, None) if line_kind == "pmkid" else tuple(plant)


def weak_match(ignored_bits):
    """A comparer of (target field, computed 16 bytes) that does not look at the target bits in ignored_bits (bit
    b = 0x80 >> b % 8 of byte b // 8): weak_match(()) is the sound one, strncmp over 16 bytes."""
    mask = bytearray(b"\xff" * 16)
    for b in ignored_bits:
        mask[b // 8] &= ~(0x80 >> b % 8) & 0xFF
    mask = bytes(mask)

    def match(target, computed):
        return len(target) >= 16 and all((t ^ c) & m == 0 for t, c, m in zip(target[:16], computed, mask))
    return match


def swapped_match(word):
    """A comparer that reads target word `word` in the wrong byte order."""
    def match(target, computed):
        t = bytearray(target[:16])
        t[4 * word:4 * word + 4] = t[4 * word:4 * word + 4][::-1]
        return len(target) >= 16 and bytes(t) == computed
    return match


def weak_comparers():
    """{name: comparer}: 128 one-bit-blind, 16 one-byte-blind, 4 one-word-blind, 4 one-word-swapped."""
    out = {"bit%d" % b: weak_match((b,)) for b in range(128)}
    out.update({"byte%d" % k: weak_match(range(8 * k, 8 * k + 8)) for k in range(16)})
    out.update({"word%d" % w: weak_match(range(32 * w, 32 * w + 32)) for w in range(4)})
    out.update({"swapped%d" % w: swapped_match(w) for w in range(4)})
    return out


def target_of(line):
    return bytes.fromhex(line.split(b"*")[2].decode())


def with_target(line, target):
    f = line.split(b"*")
    f[2] = target.hex().encode()
    return b"*".join(f)


def flip(target, bit):
    t = bytearray(target)
    t[bit // 8] ^= 0x80 >> bit % 8
    return bytes(t)


# ---------------------------------------------------------------------------------------------------------------
# building a fixture
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dictionary(psk=PSK):
    """130 words of 8..63 bytes: `psk` at P_AT, 126 distinct decoys elsewhere."""
    rng = random.Random(0x9ec15)
    seen, words = {PSK, PSK_DIGITS}, []
    while len(words) < NWORDS:
        if len(words) in P_AT:
            words.append(psk)
            continue
        w = bytes(rng.randint(0x21, 0x7E) for _ in range(rng.randint(8, 63)))
        if w not in seen and not w.startswith(b"$HEX["):
            seen.add(w)
            words.append(w)
    assert [i for i, w in enumerate(words) if w == psk] == list(P_AT) and len(set(words)) == NWORDS - 3
    return tuple(words)


class _Builder:
    def __init__(self, psk, essids, variant, seed):
        self.psk, self.essids, self.variant = psk, essids, variant
        self.plants = PLANTS[variant]
        self.nec = halfnc(NC[variant])
        self.att = N.hashcat_attempts(self.nec, 0)
        self.seed = seed
        self.pmk = {e: O.c_pbkdf2(psk, e) for e in essids}
        self.rows = []
        self.nfam = 0

    def row(self, line, kind, tag, hit, plant, essid, true, control, frame=None):
        self.rows.append({"line": line, "kind": kind, "tag": tag, "hit": hit, "plant": plant,
                          "essid": essid, "true": true, "control": control, "frame": frame,
                          "found": expected(kind, hit, plant)})
        return len(self.rows) - 1

    def family(self, kind, frame, e, the_pmk=None):
        """plant -> true line of one (kind, frame) on ESSID e: one set of MACs, one frame, one true ANONCE."""
        essid = self.essids[e % len(self.essids)]
        self.nfam += 1
        rng = random.Random("%d/%s/%s/%d/%s" % (self.seed, kind, frame, self.nfam, the_pmk is not None))
        ap, sta = rng.randbytes(6), rng.randbytes(6)
        pmk = the_pmk or self.pmk[essid]
        if kind == "pmkid":
            return essid, {None: S.pmkid_line(self.psk, essid, ap, sta, the_pmk=pmk)}
        an, sn = C._nonces(rng, bool(self.nfam & 1))
        fseed = rng.getrandbits(64)
        out = {}
        for off, endian in self.plants:
            stored = an[:28] + N.written(an[28:], -off, endian)
            line = S.eapol_line(self.psk, essid, ap, sta, stored, sn, kind, off, endian, mp=0x00, eapol_len=frame,
                                the_pmk=pmk, rng=random.Random(fseed))
            want = N.expected(line, self.nec, an[28:])  # the model's first attempt that writes the true tail
            assert want is not None and want[1:] == (off, endian) and self.att[want[0]] == (off, endian), (kind, want)
            assert len(bytes.fromhex(line.split(b"*")[7].decode())) == frame
            out[(off, endian)] = line
        assert len({target_of(ln) for ln in out.values()}) == 1 and len(set(out.values())) == len(out)
        assert {self.att.index(p) % 4 for p in self.plants} == {0, 1, 2, 3}
        assert {(self.att.index(p) % 4, p[1]) for p in self.plants} == {(1, "LE"), (2, "LE"), (3, "BE"), (0, "BE")}
        return essid, out

    def kind(self, kind):
        frames = FRAME_LENS.get(kind, (None,))
        ki = KINDS.index(kind)  # over three ESSIDs every ESSID gets controls of two kinds or more
        fams = [self.family(kind, fr, ki + f) for f, fr in enumerate(frames)]
        ctl = {}
        for f, (essid, lines) in enumerate(fams):
            for plant, line in lines.items():
                ctl[f, plant] = self.row(line, kind, "control", True, plant, essid, target_of(line), None, frames[f])
        plants = list(fams[0][1])

        def near(tag, f, plant, change):
            c = self.rows[ctl[f, plant]]
            t = change(c["true"])
            assert t != c["true"] and len(t) == 16
            self.row(with_target(c["line"], t), kind, tag, False, plant, c["essid"], c["true"], ctl[f, plant],
                     c["frame"])

        for b in range(128):
            near("bit%d" % b, b % len(fams), plants[b // 2 % len(plants)], lambda t: flip(t, b))
        for w in range(4):
            near("swap%d" % w, w % len(fams), plants[w % len(plants)],
                 lambda t: t[:4 * w] + t[4 * w:4 * w + 4][::-1] + t[4 * w + 4:])
        # the over-long target, on MACs of its own (an outfile record holds the first 16 bytes and the MACs)
        essid, lines = self.family(kind, frames[-1], ki + 2)
        plant = plants[3 % len(plants)]
        line = lines[plant]
        true = target_of(line)
        tail17 = bytes([LONG_TAIL[0] ^ 0x10]) + LONG_TAIL[1:]
        k = self.row(with_target(line, true + LONG_TAIL), kind, "long_hit", True, plant, essid, true, None, frames[-1])
        self.row(with_target(line, flip(true, 127) + LONG_TAIL), kind, "long_miss", False, plant, essid, true, k,
                 frames[-1])
        self.row(with_target(line, true + tail17), kind, "long_hit17", True, plant, essid, true, None, frames[-1])
        # the zero PMK: one line per ESSID
        for e in range(len(self.essids)):
            essid, lines = self.family(kind, frames[0], e, the_pmk=ZERO_PMK)
            plant = plants[2 % len(plants)]
            self.row(lines[plant], kind, "zero", False, plant, essid, None, None, frames[0])


@functools.lru_cache(maxsize=None)
def fixture(name):
    """{"name", "psk", "essids", "variant", "nc", "pmk" {essid: PMK of psk}, "rows" [dict], "lines", "words"}; a row:
    line, kind, tag, hit, plant (off, endian) of a hit, essid, true (the 16 bytes a correct verifier computes for the
    PSK; None for a zero line), control (row index of the line it was made from), frame, found ((nc, endian) a hit
    reports, else None)."""
    psk, essids, variant = FIXTURES[name]
    b = _Builder(psk, essids, variant, 0x9ec1)
    for kind in KINDS:
        b.kind(kind)
    rows = b.rows
    lines = [r["line"] for r in rows]
    assert len(set(lines)) == len(lines)
    ntrue = {r["line"].split(b"*")[2] for r in rows if r["hit"]}
    assert not any(r["line"].split(b"*")[2] in ntrue for r in rows if not r["hit"])
    return {"name": name, "psk": psk, "essids": essids, "variant": variant, "nc": NC[variant], "pmk": b.pmk,
            "rows": rows, "lines": lines, "words": dictionary(psk)}


def decoys(fx):
    w = fx["words"]
    return w[1], w[2]


def jobs(fx, nc=None):
    """One check job per row: keys [decoy, PSK, decoy] and a derive, or -- every row whose number among its kind's
    hits or misses has an odd bit count, half of them -- the key [PSK] with its PMK handed over, which takes the
    caller-PMK route.  Both routes meet both frames and every planted correction."""
    d0, d1 = decoys(fx)
    nc = fx["nc"] if nc is None else nc
    out, count = [], {}
    for r in fx["rows"]:
        n = count[r["kind"], r["hit"]] = count.get((r["kind"], r["hit"]), -1) + 1
        if bin(n).count("1") & 1:
            out.append((r["line"], [fx["psk"]], fx["pmk"][r["essid"]], nc))
        else:
            out.append((r["line"], [d0, fx["psk"], d1], False, nc))
    return out


def job_results(fx, js):
    """(expected result, expected key_index) of every job of jobs(fx), from the model."""
    exp, key_index = [], []
    for r, j in zip(fx["rows"], js):
        if r["found"] is None:
            exp.append(MISS)
            key_index.append(None)
        else:
            exp.append([fx["psk"], r["found"][0], r["found"][1], fx["pmk"][r["essid"]]])
            key_index.append(j[1].index(fx["psk"]))
    return exp, key_index


def check_plan(fx, kinds=KINDS):
    """The fixture's jobs as a plan of tests/check_recall.py's shape (run_batch, mismatches, describe and
    check_recall_child.py take it), cut down to `kinds`."""
    js = jobs(fx)
    exp, key_index = job_results(fx, js)
    idx = [i for i, r in enumerate(fx["rows"]) if r["kind"] in kinds]
    return {"name": "precision_" + fx["name"], "essid": fx["essids"][0], "keys": [decoys(fx)[0], fx["psk"], decoys(fx)[1]],
            "jobs": [js[i] for i in idx], "exp": [exp[i] for i in idx], "key_index": [key_index[i] for i in idx],
            "meta": [(0 if fx["rows"][i]["kind"] == "pmkid" else fx["rows"][i]["kind"], key_index[i],
                      fx["rows"][i]["tag"], fx["rows"][i]["plant"]) for i in idx]}


def zero_jobs(fx):
    """The positive control of the zero lines, the goldens' zero-pmk shape: key [""] with the zero PMK handed over.
    Returns (jobs, expected results)."""
    js, exp = [], []
    for r in fx["rows"]:
        if r["tag"] == "zero":
            js.append((r["line"], [b""], ZERO_PMK, fx["nc"]))
            found = (None, None) if r["kind"] == "pmkid" else PLANTS[fx["variant"]][2]
            exp.append([b"", found[0], found[1], ZERO_PMK])
    return js, exp


def scan_hits(fx, rows=None, nwords=NWORDS):
    """{(line, cand, nc, endian, pmk)} of a scan of the lines of `rows` (row indices; all by default) over the first
    nwords words of the dictionary: every hit row, once per copy of the PSK."""
    rows = range(len(fx["rows"])) if rows is None else rows
    cands = [i for i in P_AT if i < nwords]
    return {(k, c, fx["rows"][i]["found"][0], fx["rows"][i]["found"][1], fx["pmk"][fx["rows"][i]["essid"]])
            for k, i in enumerate(rows) if fx["rows"][i]["hit"] for c in cands}


def records(fx):
    """The outfile records of a crack call over the fixture's lines, sorted: one per hit row."""
    return sorted(N.record(with_target(r["line"], r["true"]), fx["psk"]) for r in fx["rows"] if r["hit"])


def describe(fx, idx):
    return [(fx["rows"][i]["kind"], fx["rows"][i]["tag"], fx["rows"][i]["plant"], fx["rows"][i]["frame"]) for i in idx]
