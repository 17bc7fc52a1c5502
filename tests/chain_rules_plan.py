"""Fixtures and reference for rules on chain list parts (k_prep_chain_rules, dwpa_scan_set_chain_rules,
dwpa_crack_chain_rules, python -m dwpa_amd.chain with rules: / rule: modifiers).  Nothing here needs a GPU.

A chain is written as in tests/test_gpu_chain.py -- a list of words, or a mask as bytes -- and a RULED list part as a
tuple (words, rule lines).  The reference is RuledChain, tests/test_gpu_chain.Chain with this restated on top:

  * a ruled part has len(words) * len(rules) choices, RULE-MAJOR: choice = rule * len(words) + word;
  * its piece is oracle/rules.py's apply(rule, word), which rejects an input of 0 bytes or above 256 and whatever a
    reject or memory function rejects; a rejected choice drops the candidate; an empty result is an ordinary piece;
  * "a list word above 63 bytes drops" applies to the RESULT of a ruled part and to the raw word of an un-ruled one;
  * order (last part fastest), id = raw index, 8 <= total <= 63 and the compaction are the chain's.

The words carry mixed case and distinct digit tails, so that ':', 'c', 'u' (and 'l') give different strings, and a
reject function never stands alone in a rule (its survivors would equal those of ':').
"""
import random

from oracle import rules as OR
from tests import test_gpu_chain as G
from tests import test_gpu_recall as R

CUSTOM = G.CUSTOM
M6, ML = G.M6, G.ML  # ?1?2 (2 positions, K = 6) and ?1-?2 (3 positions, K = 6)

# ':', 'c', 'u', '$1', '^!', 'd', "'4", '[', one reject function ('>6': fewer than 6 bytes reject) and one memory
# sequence ('M [ 4': the word without its first byte, then the saved word)
RSA = [":", "c", "u", "$1", "^!", "d", "'4", "[", ">6 $#", "M [ 4"]
RSB = [":", "[", "d", "^!", "$1"]          # every result differs on a one-byte word too
RSC = ["c", "'4 $7", "M u 6", "_5 $3"]     # '_5': any length but 5 rejects; 'M u 6': the saved word before its upper case

REASONS = ("rule_reject", "input_0", "input_257", "result_above_63", "total_below_8", "total_above_63",
           "unruled_above_63")


class RuledChain(G.Chain):
    """G.Chain whose list parts may be (words, rules): radices, pieces and the filter as the module docstring says."""

    def __init__(self, parts, custom=CUSTOM):
        self.rules = [[OR.parse(r) for r in p[1]] if isinstance(p, tuple) else None for p in parts]
        assert all(ops is not None for rs in self.rules if rs for ops in rs)
        self.given = parts
        super().__init__([p[0] if isinstance(p, tuple) else p for p in parts], custom)
        self.radix = [r * len(rs) if rs else r for r, rs in zip(self.radix, self.rules)]
        self.k = 1
        for r in self.radix:
            self.k *= r

    def split(self, p, d):
        """(rule, word) of digit d at ruled part p."""
        return divmod(d, len(self.parts[p]))

    def pieces(self, i):
        """One piece per part; None where a ruled part rejects its choice."""
        out = []
        for p, d in enumerate(self.digits(i)):
            if self.sets[p] is not None:
                out.append(G.ref_candidate(self.sets[p][0], d))
            elif self.rules[p] is None:
                out.append(self.parts[p][d])
            else:
                r, w = self.split(p, d)
                out.append(OR.apply(self.rules[p][r], self.parts[p][w]))
        return out

    def why(self, i, minlen=8, maxlen=63):
        """The reasons candidate i is dropped (empty: kept), and its bytes (None when a part rejects)."""
        ps, why = self.pieces(i), set()
        for p, (x, d) in enumerate(zip(ps, self.digits(i))):
            if self.sets[p] is not None:
                continue
            if self.rules[p] is None:
                if len(x) > 63:
                    why.add("unruled_above_63")
                continue
            n = len(self.parts[p][self.split(p, d)[1]])
            if x is None:
                why.add("input_0" if n == 0 else "input_257" if n > 256 else "rule_reject")
            elif len(x) > 63:
                why.add("result_above_63")
        if None in ps:
            return why, None
        psk = b"".join(ps)
        if not why and len(psk) < minlen:
            why.add("total_below_8")
        if not why and len(psk) > maxlen:
            why.add("total_above_63")
        return why, psk

    def candidate(self, i, minlen=8, maxlen=63):
        why, psk = self.why(i, minlen, maxlen)
        return psk, not why

    def ruled_choices(self, i):
        """{(part, rule)} of candidate i's ruled parts."""
        return {(p, self.split(p, d)[0]) for p, d in enumerate(self.digits(i)) if self.rules[p] is not None}

    def unruled(self):
        """The same parts without their rules."""
        return G.Chain(self.parts, self.custom)


LOWER, UPPER = b"abcdefghijkmnopqrstuvwxyz", b"ABCDEFGHJKLMNPQRSTUVWXYZ"


def words(seed, lengths):
    """Distinct printable words of the given lengths (0: the empty word): a lower-case letter first, an upper-case
    one second, mixed case after it and a digit tail that no other word of the list has (a word too short for that is
    the end of its tail); no two words share their first four bytes."""
    rng = random.Random(seed)
    out, heads = [], set()
    for k, n in enumerate(lengths):
        tail = b"%d" % (k + 2)
        while True:
            room = n - len(tail)
            if room <= 0:
                w = tail[len(tail) - n:]
            else:
                head = bytes([rng.choice(LOWER)]) + (bytes([rng.choice(UPPER)]) if room >= 2 else b"")
                w = head + bytes(rng.choice(LOWER + UPPER) for _ in range(room - len(head))) + tail
            if not n or w[:4] not in heads:
                break
        heads.add(w[:4])
        out.append(w)
    assert [len(w) for w in out] == list(lengths) and len(set(out)) == len(out)
    return out


# the lists: every length the rule engine and the filter treat differently
LA = words(0xA1, (9, 0, 1, 8, 63, 64, 256, 257, 5, 40, 12))
LB = words(0xB2, (1, 0, 8, 257, 3, 62))
LC = words(0xC3, (5, 6, 9))
LD = words(0xD4, (1, 0, 8, 257, 40))
LE = words(0xE5, (9, 0, 1, 8, 63, 64, 256, 257, 5, 40, 12, 10, 11, 13, 20, 31, 62, 33))
LF = words(0xF6, (5, 6, 9, 64, 3))   # no empty word: ':' rejects one, an un-ruled part keeps it
LG = words(0x67, (1, 8, 257, 12, 62))
M2 = b"?1="  # 2 positions, K = 2
LU = [b"", b"U" * 64, b"u2", b"Unr3-"]  # un-ruled: an empty word, a 64-byte word

SHAPES = ("RM", "MR", "RR", "URMR")
# the drop reasons each shape must show (every reason its parts can give)
SHAPE_REASONS = {"RM": set(REASONS) - {"unruled_above_63"}, "MR": set(REASONS) - {"unruled_above_63"},
                 "RR": set(REASONS) - {"unruled_above_63"}, "URMR": set(REASONS)}


def shape(name):
    return RuledChain({"RM": [(LA, RSA), ML], "MR": [ML, (LA, RSA)], "RR": [(LC + LA[:1], RSA), (LB, RSB)],
                       "URMR": [LU, (LC, RSC), M2, (LD, RSB)]}[name])


LOOP_NWORDS = (1, 3, 63, 64, 65)
# 72 rules, so that the 64 raw indices of a wave can hold 64 of them; the reject rule second, where every nwords'
# first window crosses into it
RSL = (RSA[:1] + RSA[8:9] + RSA[1:8] + RSA[9:] + ["$" + chr(c) for c in range(ord("a"), ord("z") + 1)] + ["^" + chr(c) for c in range(ord("A"), ord("Z") + 1)]
       + ["$%d $%d" % (d, d) for d in range(10)])
assert len(RSL) == 72 and len(set(RSL)) == 72


def loop_chain(nwords):
    """The distinct-rule loop: the LAST part ruled, nwords words under the 72 rules of RSL, behind an un-ruled list
    long enough for K >= 600.  The 64 raw indices of a wave hold about 64 / nwords + 1 distinct rules: 64, 22, 2,
    1 or 2, 1 or 2 for nwords 1, 3, 63, 64, 65."""
    lead = [b"p%d-" % j for j in range(max(2, -(-600 // (nwords * len(RSL)))))]
    return RuledChain([lead, (words(0x100 + nwords, [(7, 5, 6, 8, 9, 10)[k % 6] for k in range(nwords)]), RSL)])


def loop_windows(ch, nwords):
    """Windows (first, count) that each cross a rule boundary (a multiple of nwords within the last part) away from
    the 64-lane wave boundaries of the launch, with `first` no multiple of 64: counts 63, 65, 200 (a partial last
    wave), 1, and two that end at K.  No slot holds in two windows what it held before."""
    n, per = nwords, ch.radix[1]
    bnd = lambda x: -(-x // n) * n  # the first rule boundary at or after x
    want = [(bnd(50), 63), (per + bnd(50), 65), (bnd(ch.k // 2 + 100), 200), (bnd(300), 1), (ch.k, 1), (ch.k, 130)]
    loads, held = [], set()
    for at, count in want:
        for back in ([count] if at == ch.k else range(1, 40) if count == 1 else range(count // 2 + 1, count)):
            first = at - back
            if first <= 0 or first % 64 == 0 or first + count > ch.k or (count > 1 and (at - first) % 64 == 0):
                continue
            slots = set(enumerate(i for i, psk in ch.kept(first, count)))
            if slots and not slots & held:
                break
        else:
            raise AssertionError("no window of %d across %d keeps its slots apart" % (count, at))
        held |= slots
        loads.append((first, count))
    return loads


def carry_windows(ch):
    """Windows that cross a multiple of every part's stride but the last's (a wrap of the parts behind it and a carry
    into it), with counts 65 and 3, and two that end at K (the first part's carry goes nowhere); slots kept apart as
    in loop_windows."""
    stride = [1] * len(ch.radix)
    for p in range(len(ch.radix) - 2, -1, -1):
        stride[p] = stride[p + 1] * ch.radix[p + 1]
    want = [(stride[p], count) for p in range(len(ch.radix) - 1) for count in (65, 3)]
    want += [(0, 300 if ch.k > 600 else ch.k // 3), (0, 1)]  # 0: ending at K
    loads, held = [], set()
    for step, count in want:
        ats = [ch.k] if not step else range(step * (-(-count // step)), ch.k, step)
        for at, back in ((at, back) for at in ats for back in ([count] if not step else range(count // 2 + 1, count))):
            first = at - back
            if first <= 0 or first + count > ch.k:
                continue
            slots = set(enumerate(i for i, psk in ch.kept(first, count)))
            if (slots or not step) and not slots & held:  # the very last candidate may be a dropped one
                break
        else:
            raise AssertionError("no window of %d across a multiple of %d keeps its slots apart" % (count, step))
        held |= slots
        loads.append((first, count))
    return loads


def rules_text(rules):
    return ("\n".join(rules) + "\n").encode()


def alone():
    """One ruled list and nothing else: what Scan.set_rules + load_rules give, under other ids."""
    return RuledChain([(LE, RSA)])


def colon():
    """':' on every list part: the un-ruled chain's candidates under the same ids (no list holds an empty word)."""
    return RuledChain([(LF, [":"]), ML, (LG, [":"])])


# dwpa_crack_chain_rules through the command line: a rules file whose last line hashcat's -r loader skips
CRACK_A = words(0x7A, (5, 64, 0, 300, 6, 9))
CRACK_B = [b"-one", b"-twoo", b"", b"-four4"]
CRACK_RULES = [":", "c", "$1", ">6 $#"]
CRACK_MASK = b"?d?1"
CRACK_CUSTOM = (b"ab",)


def crack_chain(full):
    """The crack test's chain as the library loads it: every rule (DWPA_RULE_MODE=full) or hashcat's -r loader's."""
    rules = CRACK_RULES if full else [r for r in CRACK_RULES if OR.hashcat_loads(r)]
    return RuledChain([(CRACK_A, rules), CRACK_B, CRACK_MASK], CRACK_CUSTOM)


def fixtures():
    """Every fixture the GPU tests plant: name -> (chain, windows or None for the whole key space, the drop reasons
    it must show)."""
    out = {name: (shape(name), None, SHAPE_REASONS[name]) for name in SHAPES}
    for n in LOOP_NWORDS:
        ch = loop_chain(n)
        out["loop%d" % n] = (ch, loop_windows(ch, n), {"rule_reject"} if n > 1 else set())  # one word: 7 bytes
    out["alone"] = (alone(), None, set(REASONS) - {"unruled_above_63", "total_above_63"})
    out["colon"] = (colon(), None, {"input_257", "result_above_63", "total_above_63"})
    for full in (False, True):
        out["crack_full" if full else "crack_hashcat"] = (crack_chain(full), None,
                                                          {"input_0", "input_257", "result_above_63"} |
                                                          ({"rule_reject"} if full else set()))
    return out


def planted(ch, windows):
    """[(id, psk)] to plant for a fixture: the kept candidates of its windows, each id once, in id order."""
    if windows is None:
        return ch.kept(0, ch.k)
    return sorted(dict(c for first, count in windows for c in ch.kept(first, count)).items())
