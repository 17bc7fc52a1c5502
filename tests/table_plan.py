"""The table attack's fixtures and its reference, shared by tests/test_table_plan.py (CPU), tests/test_table.py (CPU)
and tests/test_gpu_table.py (GPU).

The reference is independent of the library: a table text is parsed here by the rules of include/dwpa22000.h ("table
attack"), a word's candidates are itertools.product over the per-byte alternative lists, and the keyspace is a prefix
sum in plain ints, so a product of 2^64 or 16^63 is simply a large number here.

A Plan is a table, a word list and a filter.  Every word of a fixture ends in a decimal counter of neutral bytes
(digits are neither keys nor values of TABLE), so no two words -- and no two candidates -- are one string, and no
candidate ends in a NUL byte (two PSKs that differ in trailing NULs are one HMAC key).
"""
import itertools

U32 = 2**32 - 1


def hx(b):
    return b"\\x%02x" % b


def table_text(mapping, hexed=True):
    """{key byte: bytes of alternatives} as table text, one K=V line per alternative."""
    lines = []
    for k, vs in mapping.items():
        for v in vs:
            lines.append((hx(k) if hexed else bytes([k])) + b"=" + (hx(v) if hexed else bytes([v])))
    return b"\n".join(lines) + b"\n"


def _side(line, i):
    """One byte of a K=V line at i: (byte, next i) or None at the end of the line."""
    if i >= len(line):
        return None
    h = line[i + 2:i + 4]
    if line[i:i + 2] == b"\\x" and len(h) == 2 and all(c in b"0123456789abcdefABCDEF" for c in h):
        return int(h, 16), i + 4
    return line[i], i + 1


def ref_parse(text):
    """alt[c] for the 256 byte values, or ValueError(line number)."""
    alt = [None] * 256
    mappings = 0
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    for n, line in enumerate(lines, 1):
        if line.endswith(b"\r"):
            line = line[:-1]
        if not line:
            continue
        k = _side(line, 0)
        if k is None or k[1] >= len(line) or line[k[1]] != 0x3d:
            raise ValueError(n)
        v = _side(line, k[1] + 1)
        if v is None or v[1] != len(line):
            raise ValueError(n)
        if alt[k[0]] is None:
            alt[k[0]] = []
        if v[0] in alt[k[0]]:
            continue
        if len(alt[k[0]]) == 16:
            raise ValueError(n)
        alt[k[0]].append(v[0])
        mappings += 1
    if not mappings:
        raise ValueError(len(lines) + 1)
    return [bytes([c]) if a is None else bytes(a) for c, a in enumerate(alt)]


def ref_count(alt, word):
    k = 1
    for c in word:
        k *= len(alt[c])
    return k


KEPT, DROP_LEN, DROP_MAX = "kept", "length", "word_max"


class Plan:
    """A table (text), a list and a filter: which words are kept and why not, start[], K, and candidate(id)."""

    def __init__(self, table, words, minlen=8, maxlen=63, word_max=0):
        self.table, self.words = table, list(words)
        self.minlen, self.maxlen, self.word_max = minlen, maxlen, word_max
        self.alt = ref_parse(table)
        wm = word_max if word_max else U32
        self.count = [ref_count(self.alt, w) for w in self.words]
        self.why = [DROP_LEN if not minlen <= len(w) <= min(maxlen, 63) else DROP_MAX if k > wm else KEPT
                    for w, k in zip(self.words, self.count)]
        self.kword = [i for i, y in enumerate(self.why) if y == KEPT]
        self.start = [0]
        for i in self.kword:
            self.start.append(self.start[-1] + self.count[i])
        self.k = self.start[-1]

    def kept(self):
        return len(self.kword)

    def word_of(self, i):
        """The kept-word ordinal j with start[j] <= i < start[j + 1]."""
        assert 0 <= i < self.k
        lo, hi = 0, len(self.kword)
        while hi - lo > 1:
            m = (lo + hi) // 2
            lo, hi = (m, hi) if self.start[m] <= i else (lo, m)
        return lo

    def candidate(self, i):
        j = self.word_of(i)
        w = self.words[self.kword[j]]
        sub = i - self.start[j]
        out = bytearray(len(w))
        for p in range(len(w) - 1, -1, -1):  # last position fastest
            a = self.alt[w[p]]
            sub, d = divmod(sub, len(a))
            out[p] = a[d]
        assert sub == 0
        return bytes(out)

    def all_of_word(self, j):
        """Every candidate of kept word j by itertools.product: what candidate() must agree with."""
        w = self.words[self.kword[j]]
        return [bytes(t) for t in itertools.product(*[self.alt[c] for c in w])]

    def window(self, first, count):
        return [(i, self.candidate(i)) for i in range(first, first + count)]


# ---------------------------------------------------------------------------------------------------------------
# the table of the GPU fixtures: alternative counts 1, 2, 3, 5, 7, 8, 11 and 16; a key without identity; keys and
# values 0x00, 0x80 and 0xff.  Digits, '-' and the letters k..p are neutral: neither key nor value.
# ---------------------------------------------------------------------------------------------------------------
TABLE_MAP = {
    ord("a"): b"a@A",                       # 3
    ord("b"): b"bB&%!",                     # 5
    ord("c"): b"cC(<{[^",                   # 7
    ord("d"): b"dD)>}]~_+=;",               # 11
    ord("h"): b"hH#*?/:.",                  # 8
    ord("s"): b"s$",                        # 2
    ord("x"): b"xXyYzZwWvVuUtTrR",          # 16
    ord("q"): b"Q",                         # 1: replaced, the original is gone
    0x00: b"\x00\x80",                      # 2
    0x80: b"\x80\x00\xff",                  # 3
    0xff: b"\x00\xff",                      # 2
}
TABLE = table_text(TABLE_MAP)


def tail(n, width=4):
    return b"%0*d" % (width, n)


def ones(n, base=0):
    """n words of count 1 and 8..12 bytes (so the packed offsets take every value mod 4), some with the replaced q."""
    body = (b"klmn", b"qkl-m", b"opq-kl", b"mnopklq", b"-q-q-q-q")
    return [body[(base + i) % 5] + tail(base + i) for i in range(n)]


WIDE = b"abcd" + tail(7777)            # 3 * 5 * 7 * 11 = 1155
assert len(WIDE) == 8

PLAN_ONES = Plan(TABLE, ones(200))                                        # 64 words per wave
PLAN_WIDE = Plan(TABLE, [WIDE])                                           # one word over several waves and blocks
PLAN_MIXED = Plan(TABLE, ones(70) + [WIDE] + ones(70, 100))               # loads that begin and end inside WIDE
PLAN_RUN = Plan(TABLE, ones(30) + [b"abc-" + tail(1)] + ones(30, 100))    # 3 * 5 * 7 = 105, for run() over 3 ESSIDs
PLAN_ONE_KEPT = Plan(TABLE, [b"short", b"a" + b"klmnop-" + tail(5), b"x" * 16])   # nkept = 1, count 3
PLAN_65 = Plan(TABLE, ones(65, 300))                                      # nkept = 65
# bytes 0x00 / 0x80 / 0xff as keys and values, counts 1, 2, 3 and 16 in one word, 8 and 63 bytes, odd offsets
BYTES_WORDS = [b"\x80\x00\xffqx" + tail(1, 3),                            # 8 bytes: 3 * 2 * 2 * 1 * 16 = 192
               b"a" + b"qk-" * 19 + b"s" + tail(2),                       # 63 bytes: 3 * 2 = 6
               b"\xff-\x80-\x00" + tail(3, 5),                            # 10 bytes: 2 * 3 * 2 = 12
               b"s" + b"lmnopq-" * 8 + b"\x80" + tail(44, 5)]             # 63 bytes at an odd offset: 2 * 3 = 6
PLAN_BYTES = Plan(TABLE, BYTES_WORDS)
# three words of 2^31 candidates: K = 3 * 2^31 > 2^32
PLAN_BIG = Plan(TABLE, [b"xxxxxxxh" + tail(n, 1) for n in range(3)])
BIG_WINDOWS = [(2**31 - 64, 128), (2**32 - 64, 128), (3 * 2**31 - 128, 128)]

# every drop reason with a kept neighbour on each side, the first, the last and every second word dropped
WORD_MAX = 14
DROPS = [
    (b"", DROP_LEN),                             # 0 bytes, the first word
    (b"klmn" + tail(2), KEPT),                   # 1
    (b"a" + tail(1, 6), DROP_LEN),               # 7 bytes
    (b"sc" + b"-" * 3 + tail(4), KEPT),          # 2 * 7 = 14: exactly word_max
    (b"a" + b"k" * 59 + tail(3), DROP_LEN),      # 64 bytes
    (b"sa" + b"-" * 57 + tail(6), KEPT),         # 63 bytes, 6
    (b"ab" + b"-" * 3 + tail(5), DROP_MAX),      # 3 * 5 = 15: word_max + 1
    (b"ass" + b"-" + tail(8), KEPT),             # 8 bytes, 12
    (b"x" * 8 + tail(7), DROP_MAX),              # 16^8 = 2^32
    (b"d" + b"q" * 7 + tail(10), KEPT),          # 11
    (b"x" * 16 + tail(9), DROP_MAX),             # 16^16 = 2^64
    (b"\x00" + b"k" * 7 + tail(11), KEPT),       # 2
    (b"x" * 63, DROP_MAX),                       # 16^63
    (b"c" + b"-" * 8 + tail(13), KEPT),          # 7
    (b"h" * 2 + b"-" * 3 + tail(12), DROP_MAX),  # 64
    (b"a" + b"-" * 8 + tail(14), KEPT),          # 3
    (b"s" * 66 + tail(15), DROP_LEN),            # 70 bytes, the last word
]
PLAN_DROPS = Plan(TABLE, [w for w, y in DROPS], word_max=WORD_MAX)
# the same list under word_max = 0 (2^32 - 1): 2^32 is still dropped; 15 * 16^7 (above 2^31, below 2^32) is kept
NEAR = b"x" * 7 + b"=" + tail(99)
TABLE15 = TABLE + b"\n".join(b"==" + bytes([v]) for v in b"=ABCDEFGHIJKLMN") + b"\n"   # '=' with 15 alternatives
PLAN_DROPS_WIDE = Plan(TABLE15, [w for w, y in DROPS] + [NEAR], word_max=0)

PLANS = {"ones": PLAN_ONES, "wide": PLAN_WIDE, "mixed": PLAN_MIXED, "run": PLAN_RUN, "one_kept": PLAN_ONE_KEPT,
         "65": PLAN_65, "bytes": PLAN_BYTES, "big": PLAN_BIG, "drops": PLAN_DROPS, "drops_wide": PLAN_DROPS_WIDE}
# the indices the GPU tests plant: everything, except for the plans whose keyspace is too large to enumerate
PLANTED = {name: [(0, p.k)] for name, p in PLANS.items() if p.k <= 4096}
PLANTED["big"] = BIG_WINDOWS
