"""The association attack's reference and fixtures (CPU): nets from hashlines, the single generator, entries, start[]
and candidate(id), restated in plain Python from the contract in include/dwpa22000.h ("association attack") with
oracle/rules.py as the rule engine.  tests/test_assoc_plan.py holds the library to it; tests/test_gpu_assoc.py takes its
expectations from it.

Fixture words end in a counter, so no two candidates of a fixture are one string and none ends in NUL (a trailing NUL
is HMAC key padding: two such PSKs are one key).
"""
import bisect
import gzip
import random

from oracle import oracle as O
from oracle import rules as RU
from tests import synth as S

NC = 8
OFFSETS = (0, 1, -1, 2, -2, -3, 4, -4)  # planted nonce offsets, as tests/test_gpu_recall.py
SUFFIXES = (b"", b"1", b"123", b"!")


# ---------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------
def line_net(line):
    """(essid, mac_ap) of a hashline the fixtures build, None for anything else (the fixtures' unusable lines are far
    from the format: what exactly the parser accepts is tests/test_abi.py's and the parity tests' business)."""
    f = line.split(b"*")
    if len(f) != 9 or f[0] != b"WPA" or f[1] not in (b"01", b"02"):
        return None
    try:
        return bytes.fromhex(f[5].decode()), bytes.fromhex(f[3].decode())
    except ValueError:
        return None


def nets_of(lines):
    """[(essid, mac_ap, [input lines])] in order of first appearance, and the net of every line (None: unusable)."""
    nets, index, of_line = [], {}, []
    for i, ln in enumerate(lines):
        key = line_net(ln)
        if key is None:
            of_line.append(None)
            continue
        if key not in index:
            index[key] = len(nets)
            nets.append((key[0], key[1], []))
        nets[index[key]][2].append(i)
        of_line.append(index[key])
    return nets, of_line


def _upper(b):
    return bytes(c - 32 if 0x61 <= c <= 0x7A else c for c in b)


def _lower(b):
    return bytes(c + 32 if 0x41 <= c <= 0x5A else c for c in b)


def single(mac_ap, essid, minlen):
    """The single generator, duplicates included."""
    out = []
    if len(mac_ap) == 6:
        b = int.from_bytes(mac_ap, "big")
        for i in (-1, 0, 1):
            h = b"%012x" % ((b + i) % 2**48)
            for j in (12, 10, 8):
                out += [h[12 - j:], _upper(h[12 - j:])]
    for suffix in SUFFIXES:
        c = essid + suffix
        if len(c) < minlen:
            continue
        out.append(c)
        if _upper(c) != c:
            out.append(_upper(c))
        if _lower(c) != c:
            out.append(_lower(c))
    return out


def unhex(w):
    """$HEX[...] as the library's hc_unhex takes it: an even number of hex digits between the brackets."""
    if len(w) > 6 and w.startswith(b"$HEX[") and w.endswith(b"]") and len(w) % 2 == 0:
        try:
            return bytes.fromhex(w[5:-1].decode("ascii"))
        except ValueError:
            return w
    return w


def parse_assoc_line(ln):
    """(mac, word) of one association line (no line end), None for a line of another shape."""
    if len(ln) < 13 or ln[12:13] != b":" or any(c not in b"0123456789abcdefABCDEF" for c in ln[:12]):
        return None
    w = ln[13:]
    return bytes.fromhex(ln[:12].decode()), unhex(w) if w.startswith(b"$HEX[") else w


class Plan:
    """lines: the hash file's lines; assoc: the association file's lines (raw, no line ends) or None; single: the flag;
    rules: rule lines (str) or None.  nets=[(essid, mac_ap)] stands in for the lines where a fixture needs its
    candidates before it can build them, and words=[[...] per net] for the sources, as Scan.set_assoc takes entries.
    Everything the library reports is an attribute computed here in plain ints."""

    def __init__(self, lines, assoc=None, single_gen=False, rules=None, nets=None, words=None, single_minlen=None):
        self.lines, self.assoc, self.single, self.rules = list(lines or []), assoc, single_gen, rules
        if nets is None:
            self.nets, self.net_of_line = nets_of(self.lines)
        else:
            self.nets, self.net_of_line = [(e, m, []) for e, m in nets], []
        self.ops = [RU.parse(r) for r in rules] if rules is not None else None
        assert self.ops is None or all(o is not None for o in self.ops)
        self.r = len(self.ops) if self.ops is not None else 1
        words = [list(ws) for ws in words] if words is not None else [[] for _ in self.nets]
        assert len(words) == len(self.nets)
        self.file_lines = self.unmatched = self.malformed = 0
        for ln in assoc or []:
            self.file_lines += 1
            p = parse_assoc_line(ln)
            if p is None:
                self.malformed += 1
                continue
            hit = [n for n, (e, m, _) in enumerate(self.nets) if m == p[0]]
            if not hit:
                self.unmatched += 1
            for n in hit:
                words[n].append(p[1])
        if single_gen:
            for n, (e, m, _) in enumerate(self.nets):
                words[n] += single(m, e, single_minlen or (8 if rules is None else 1))
        self.words, self.dropped = [], 0
        for ws in words:
            seen, kept = set(), []
            for w in ws:
                if not 1 <= len(w) <= 256 or w in seen:
                    self.dropped += 1
                    continue
                seen.add(w)
                kept.append(w)
            self.words.append(kept)
        self.start = [0]
        for ws in self.words:
            assert len(ws) * self.r < 2**32
            self.start.append(self.start[-1] + len(ws) * self.r)
        self.k = self.start[-1]
        self.entries = sum(len(ws) for ws in self.words)

    def info(self):
        return {"keyspace": self.k, "nets": len(self.nets), "entries": self.entries, "file_lines": self.file_lines,
                "unmatched": self.unmatched, "malformed": self.malformed, "dropped": self.dropped, "rules": self.r}

    def split(self, i):
        """Index -> (net, rule, word index)."""
        assert 0 <= i < self.k
        n = bisect.bisect_right(self.start, i) - 1  # the last net that starts at or below i: it is not empty
        assert self.words[n] and self.start[n] <= i < self.start[n + 1]
        sub = i - self.start[n]
        return n, sub // len(self.words[n]), sub % len(self.words[n])

    def net_of(self, i):
        return self.split(i)[0]

    def candidate(self, i, minlen=8, maxlen=63):
        """The candidate of index i, or None."""
        n, rule, w = self.split(i)
        c = self.words[n][w] if self.ops is None else RU.apply(self.ops[rule], self.words[n][w])
        return c if c is not None and minlen <= len(c) <= maxlen else None

    def flat(self):
        """(words, net per word) as Scan.set_assoc takes them."""
        return ([w for ws in self.words for w in ws], [n for n, ws in enumerate(self.words) for _ in ws])

    def first_line(self, i):
        return self.nets[self.net_of(i)][2][0]


# ---------------------------------------------------------------------------------------------------------------
# fixture building: nets first, lines from their candidates
# ---------------------------------------------------------------------------------------------------------------
def mac(k):
    """A MAC_AP no other fixture net has: 02:a5 then a counter."""
    return b"\x02\xa5" + k.to_bytes(4, "big")


def make_line(kind, nc, endian, psk, essid, ap, pmk, rng):
    sta = rng.randbytes(6)
    if kind == 0:
        return S.pmkid_line(psk, essid, ap, sta, the_pmk=pmk)
    return S.eapol_line(psk, essid, ap, sta, rng.randbytes(32), rng.randbytes(32), kind, nc, endian,
                        mp=(0x00, 0x80, 0x02)[nc % 3], the_pmk=pmk, rng=rng)


def plant(nets, psks_of_net, rng, kinds=(0, 1, 2, 3)):
    """nets: [(essid, mac_ap)]; psks_of_net[n]: the PSKs net n's lines carry, one line each (a net with none gets one
    line of a PSK nobody tries, so that it exists).  Lines are net-major, so net numbers are list positions.  Returns
    (lines, [(net, psk)] per line, [pmk] per line, [(nc, endian)] per line as the oracle reports them)."""
    lines, owner, pmks, found = [], [], [], []
    for n, (essid, ap) in enumerate(nets):
        psks = list(psks_of_net[n]) or [b"nobody-tries-%06d" % n]
        raw = O.c_pbkdf2_many(psks, essid, threads=8)
        for i, psk in enumerate(psks):
            k = len(lines)
            pmk = raw[32 * i:32 * i + 32]
            line = make_line(kinds[k % len(kinds)], OFFSETS[k // 4 % 8], ("LE", "BE")[k // 32 % 2], psk, essid, ap, pmk, rng)
            exp = O.c_check_key_m22000(line, [psk], pmk, NC)
            assert exp and exp[0] == psk and exp[3] == pmk, (k, exp)
            lines.append(line)
            owner.append((n, psk))
            pmks.append(pmk)
            found.append((exp[1], exp[2]))
    assert len(set(lines)) == len(lines)
    return lines, owner, pmks, found


def counter_words(tag, n, length=0):
    """n words that end in a counter: tag-000000, tag-000001, ...; length pads the tag with 'x' to that many bytes."""
    out = []
    for i in range(n):
        w = b"%s-%06d" % (tag, i)
        if length:
            assert length >= len(w)
            w = tag + b"x" * (length - len(w)) + b"-%06d" % i
        out.append(w)
    return out


def write_assoc(path, lines, gz=False, crlf=False):
    data = b"".join(ln + (b"\r\n" if crlf else b"\n") for ln in lines)
    with open(path, "wb") as f:
        f.write(gzip.compress(data) if gz else data)


# rule lines a rules *file* loads under hashcat's loader (no reject or memory function), with length-changing ones
FILE_RULES = [":", "l", "u", "c", "$1", "$1 $2 $3", "^e ^h ^t", "d", "[ [ [", "r", "$!"]


def cpu_fixture(seed=0xa550c):
    """One hash file for the CPU tests: ESSIDs of 4, 7, 8 and 32 bytes; BSSIDs 000000000000, ffffffffffff and an
    all-digit one; one MAC under two ESSIDs; a net with two lines; an unusable line in the middle.  Returns (lines,
    association lines with unmatched, malformed, duplicate, empty, over-long and $HEX[] entries)."""
    rng = random.Random(seed)
    nets = [(b"four", bytes(6)), (b"Seven77", b"\xff" * 6), (b"Eight888", bytes.fromhex("123456789012")),
            (bytes(0x41 + i % 26 for i in range(32)), mac(1)), (b"twin-essid-A", mac(2)), (b"twin-essid-B", mac(2)),
            (b"linksys", mac(3))]
    psks = [[b"psk-of-net-%d-a" % n] for n in range(len(nets))]
    psks[3].append(b"psk-of-net-3-b")  # a second line in one net
    lines, _, _, _ = plant(nets, psks, rng, kinds=(0, 2))
    lines.insert(4, b"this is no hashline")
    assoc = []
    for n, (e, m) in enumerate(nets):
        if n == 5:
            continue  # the twin MAC is listed once and feeds both nets
        assoc += [m.hex().encode() + b":" + w for w in counter_words(b"assoc%d" % n, 3)]
    assoc += [nets[1][1].hex().upper().encode() + b":UPPER-MAC-000001",          # hex digits in upper case
              nets[2][1].hex().encode() + b":assoc2-000000",                      # a duplicate within its net
              nets[2][1].hex().encode() + b":",                                   # an empty word
              nets[2][1].hex().encode() + b":" + b"L" * 257,                      # above 256 bytes
              nets[2][1].hex().encode() + b":" + b"M" * 256,                      # exactly 256: kept
              nets[3][1].hex().encode() + b":$HEX[" + b"colon:\xff-000001".hex().encode() + b"]",
              nets[3][1].hex().encode() + b":$HEX[zz]",                           # not hex: stays as written
              b"0a0b0c0d0e0f:nobody-has-this-mac",                                # unmatched
              b"0a0b0c0d0e:short-mac", b"0a0b0c0d0e0g:not-hex-000", b"0a0b0c0d0e0f;semicolon", b"",  # malformed
              nets[6][1].hex().encode() + b":with:colons:inside-1"]
    return lines, assoc
