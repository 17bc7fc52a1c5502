"""CPU: what tests/test_gpu_table.py rests on.  The fixtures of tests/table_plan.py hold every case the GPU tests
claim to cover, the reference agrees with itertools.product, and the library's host side (dwpa_table_keyspace /
dwpa_table_candidates) agrees with the reference on every fixture -- so a GPU failure is the kernel's.

One case of the issue cannot exist: a word whose count is exactly 2^32 - 1.  2^32 - 1 = 3 * 5 * 17 * 257 * 65537, and
a byte has at most 16 alternatives, so no product of alternative counts has the prime factor 17.  The boundary is held
from both sides instead: 16^8 = 2^32 is dropped under word_max = 0, and 15 * 16^7 = 4,026,531,840 -- above 2^31, so it
needs all 32 bits of the count -- is kept; test_no_word_counts_2_32_minus_1 states the arithmetic.
"""
import itertools

import dwpa_amd
from tests import table_plan as T


def _lib(plan):
    return dwpa_amd.table_keyspace(plan.table, plan.words, plan.minlen, plan.maxlen, plan.word_max)


def test_reference_is_itertools_product():
    """candidate(start[j] + n) is element n of itertools.product over the word's alternative lists, for every kept
    word of every enumerable plan, and the library's candidates are the same."""
    for name, plan in T.PLANS.items():
        if plan.k > 4096:
            continue
        want = list(itertools.chain.from_iterable(plan.all_of_word(j) for j in range(plan.kept())))
        assert len(want) == plan.k
        assert [plan.candidate(i) for i in range(plan.k)] == want, name
        assert dwpa_amd.table_candidates(plan.table, plan.words, range(plan.k), plan.minlen, plan.maxlen,
                                         plan.word_max) == want, name


def test_no_two_planted_ids_give_one_string():
    for name, windows in T.PLANTED.items():
        plan = T.PLANS[name]
        psks = [plan.candidate(i) for f, c in windows for i in range(f, f + c)]
        assert len(set(psks)) == len(psks), name
        assert len({p.rstrip(b"\0") for p in psks}) == len(psks), (name, "two PSKs that are one HMAC key")
        assert all(8 <= len(p) <= 63 for p in psks), name


def test_every_drop_reason_between_kept_words():
    plan = T.PLAN_DROPS
    assert plan.why == [y for w, y in T.DROPS]
    assert [y != T.KEPT for y in plan.why] == [i % 2 == 0 for i in range(len(plan.words))], "every second word"
    assert plan.why[0] != T.KEPT and plan.why[-1] != T.KEPT
    by = {}
    for i, (w, k, y) in enumerate(zip(plan.words, plan.count, plan.why)):
        by.setdefault((len(w), y) if y == T.DROP_LEN else (k, y), []).append(i)
    dropped = [(7, T.DROP_LEN), (64, T.DROP_LEN), (T.WORD_MAX + 1, T.DROP_MAX), (2**32, T.DROP_MAX),
               (2**64, T.DROP_MAX), (16**63, T.DROP_MAX)]
    for key in dropped:
        for i in by[key]:
            assert 0 < i < len(plan.words) - 1 and plan.why[i - 1] == plan.why[i + 1] == T.KEPT, key
    assert (T.WORD_MAX, T.KEPT) in by, "a count of exactly word_max is kept"
    assert {len(plan.words[i]) for i in plan.kword} >= {8, 63}
    ks = _lib(plan)
    assert (ks["keyspace"], ks["kept"]) == (plan.k, plan.kept()) == (56, 8)
    assert ks["dropped_len"] == plan.why.count(T.DROP_LEN) == 4
    assert ks["dropped_max"] == plan.why.count(T.DROP_MAX) == 5


def test_saturation_under_the_widest_word_max():
    """word_max = 0 means 2^32 - 1: 2^32, 2^64 and 16^63 are dropped (never counted as 0 or 1), 15 * 16^7 is kept."""
    plan = T.PLAN_DROPS_WIDE
    why = dict(zip(plan.count, plan.why))
    assert why[2**32] == why[2**64] == why[16**63] == T.DROP_MAX
    assert why[15 * 16**7] == T.KEPT and 2**31 < 15 * 16**7 < 2**32
    assert why[T.WORD_MAX + 1] == why[64] == T.KEPT
    ks = _lib(plan)
    assert (ks["keyspace"], ks["kept"], ks["dropped_len"], ks["dropped_max"]) == (plan.k, plan.kept(), 4, 3)
    assert plan.k == 56 + 15 + 64 + 15 * 16**7
    ids = [0, 55, 56, plan.k - 15 * 16**7 - 1, plan.k - 15 * 16**7, plan.k - 2**31, plan.k - 1]
    assert dwpa_amd.table_candidates(plan.table, plan.words, ids, word_max=0) == [plan.candidate(i) for i in ids]


def test_no_word_counts_2_32_minus_1():
    """2^32 - 1 has the prime factors 17, 257 and 65537; a count is a product of numbers 1..16."""
    assert 3 * 5 * 17 * 257 * 65537 == 2**32 - 1
    assert all((2**32 - 1) % p == 0 and all(p % q for q in range(2, 17)) for p in (17, 257, 65537))


def test_shapes_the_gpu_tests_name():
    assert T.PLAN_ONES.kept() == T.PLAN_ONES.k == 200 and set(T.PLAN_ONES.count) == {1}
    assert T.PLAN_WIDE.k == 3 * 5 * 7 * 11 == 1155 and T.PLAN_WIDE.kept() == 1
    m = T.PLAN_MIXED
    assert m.start[70] == 70 and m.start[71] == 70 + 1155 and m.k == 1295
    assert T.PLAN_ONE_KEPT.kept() == 1 and T.PLAN_ONE_KEPT.k == 3 and T.PLAN_65.kept() == 65
    b = T.PLAN_BYTES
    assert sorted(len(w) for w in b.words) == [8, 10, 63, 63]
    offs = list(itertools.accumulate([0] + [len(w) for w in b.words]))[:-1]
    assert any(o % 2 for o in offs) and {o % 4 for o in offs} >= {0, 1, 3}
    used = {len(b.alt[c]) for w in b.words for c in w}
    assert used >= {1, 2, 3, 16}
    for byte in (0x00, 0x80, 0xff):
        assert any(byte in w for w in b.words) and any(byte in b.alt[c] for w in b.words for c in w if c != byte)
    assert b.alt[ord("q")] == b"Q", "a key without identity"
    big = T.PLAN_BIG
    assert big.count == [2**31] * 3 and big.k == 3 * 2**31 > 2**32
    for (first, count), edge in zip(T.BIG_WINDOWS, big.start[1:]):
        assert count == 128 and first < edge <= first + count
    assert T.BIG_WINDOWS[-1][0] + 128 == big.k
    for name, plan in T.PLANS.items():
        ks = _lib(plan)
        assert (ks["keyspace"], ks["kept"]) == (plan.k, plan.kept()), name
