"""CPU: the conditions the GPU tests of rules on chain parts (tests/test_gpu_chain_rules.py) rest on, checked on the
fixtures of tests/chain_rules_plan.py without a GPU.

For every fixture: no two planted ids give the same string or the same HMAC key (tests/test_gpu_combinator.plant
needs it: a hit must name one id), at least one candidate is kept, every drop reason the fixture's parts can give
occurs, and for every such reason a candidate under the same rule survives -- so a kernel that dropped the whole rule
would be seen.  Over all fixtures every reason of the specification occurs.  The windows of the distinct-rule loop
hold the numbers of rules per wave the kernel's loop is specified for.
"""
import pytest

from tests import chain_rules_plan as P

FIXTURES = P.fixtures()
RULED_REASONS = {"rule_reject", "input_0", "input_257", "result_above_63"}


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_fixture_can_be_planted_and_shows_its_drops(name):
    ch, windows, reasons = FIXTURES[name]
    kept = P.planted(ch, windows)
    assert kept and len(kept) <= 1000, len(kept)
    psks = [psk for i, psk in kept]
    assert len(set(psks)) == len(psks) and len({p.rstrip(b"\0") for p in psks}) == len(psks)
    assert all(8 <= len(p) <= 63 for p in psks)
    ids = [i for i, psk in kept]
    assert ids != list(range(ids[0], ids[0] + len(ids)))  # slots move: ids[] must carry the id
    alive = set().union(*(ch.ruled_choices(i) for i in ids))  # the (part, rule) pairs of the kept candidates
    raw = range(ch.k) if windows is None else sorted({i for f, c in windows for i in range(f, f + c)})
    seen, kept_ids = {}, set(ids)
    for i in raw:
        why, psk = ch.why(i)
        assert (not why) == (i in kept_ids), i
        for r in why:
            if r in RULED_REASONS:  # the (part, rule) pairs at which this reason arose
                pieces, digits = ch.pieces(i), ch.digits(i)
                at = {(p, ch.split(p, digits[p])[0]) for p in range(len(digits)) if ch.rules[p] is not None and
                      (pieces[p] is None or len(pieces[p]) > 63)}
            else:
                at = ch.ruled_choices(i)
            seen.setdefault(r, set()).update(at)
    assert set(seen) >= reasons, (name, sorted(seen))
    for r in reasons:
        assert seen[r] & alive, (name, r)  # a candidate under the same rule survives


def test_every_reason_occurs_somewhere():
    assert set().union(*(reasons for ch, w, reasons in FIXTURES.values())) == set(P.REASONS)


def test_reference_is_rule_major_and_filters_the_result():
    ch = P.RuledChain([[b"x-", b"yy-"], ([b"aBcd12", b"e" * 100, b"f" * 40], [":", "'8", "d"])])
    assert ch.radix == [2, 9] and ch.k == 18
    assert [ch.pieces(i)[1] for i in range(9)] == [b"aBcd12", b"e" * 100, b"f" * 40, b"aBcd12", b"e" * 8, b"f" * 8,
                                                  b"aBcd12" * 2, b"e" * 200, b"f" * 80]
    assert ch.candidate(4) == (b"x-" + b"e" * 8, True)        # a 100-byte word under '8 is legal
    assert ch.candidate(8) == (b"x-" + b"f" * 80, False)       # a 40-byte word under d drops
    assert ch.candidate(1)[1] is False and ch.candidate(9 + 6) == (b"yy-" + b"aBcd12" * 2, True)
    # an un-ruled part keeps its empty word, a ruled one rejects it; an empty RESULT is an ordinary piece
    ch = P.RuledChain([[b"", b"12345678"], ([b"", b"q"], [":", "["])])
    assert [ch.candidate(i) for i in range(4, 8)] == [(None, False), (b"12345678q", True), (None, False),
                                                      (b"12345678", True)]
    assert ch.why(0)[0] == {"input_0"} and ch.why(1)[0] == {"total_below_8"}


@pytest.mark.parametrize("nwords,most", zip(P.LOOP_NWORDS, (64, 22, 2, 2, 2)))
def test_loop_windows_hold_the_specified_rules_per_wave(nwords, most):
    """The waves of the loop windows hold 64, 22, 2, 1-2 and 1-2 distinct rules; `first` is no multiple of 64, a rule
    boundary is crossed inside a wave, and the counts are 1, 63, 65 and ones that leave a partial last wave."""
    ch = P.loop_chain(nwords)
    windows = P.loop_windows(ch, nwords)
    assert {c for f, c in windows} >= {1, 63, 65, 200} and all(f % 64 for f, c in windows)
    assert any(f + c == ch.k for f, c in windows)
    per_wave, mid_wave = [], False
    for first, count in windows:
        for w0 in range(first, first + count, 64):
            rules = [ch.split(1, ch.digits(i)[1])[0] for i in range(w0, min(w0 + 64, first + count))]
            per_wave.append(len(set(rules)))
            mid_wave |= len(set(rules)) > 1
    assert max(per_wave) == most and mid_wave
    assert nwords < 64 or min(per_wave) == 1


@pytest.mark.parametrize("name", P.SHAPES)
def test_carry_windows_wrap_every_part(name):
    ch = P.shape(name)
    loads = P.carry_windows(ch)
    assert any(f + c == ch.k for f, c in loads) and {c for f, c in loads} >= {1, 3, 65}
    crossed = set()
    for first, count in loads:
        a, b = ch.digits(first), ch.digits(first + count - 1)
        crossed |= {p for p in range(len(a)) if a[p] != b[p]}
    assert crossed == set(range(len(ch.radix)))
