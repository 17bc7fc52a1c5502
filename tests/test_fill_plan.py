"""CPU: the fixtures of tests/fill_plan.py hold what tests/test_gpu_fill_recall.py relies on.

The library's item cuts depend on the reader's chunking, so the model of the sizing loop is not compared with the
library's counters.  It proves here that each fixture reaches the overflow path, the empty-load path or neither for
every plausible cut of the words into items: a condition asserted here is not hoped for on the GPU.
"""
import time

import pytest

from tests import fill_plan as P

BATCHES = (64, 256)


def _sims(kpw, cap, nr):
    return {cut: P.simulate(kpw, cap, nr, sizes) for cut, sizes in P.item_cuts(len(kpw), cap, nr).items()}


def _share(kpw, at, n=64):
    return sum(kpw[at:at + n]) / n


def test_simulate_restates_the_loop():
    """Hand-checked runs of the model: keep == 1 loads exactly a batch; a sparse stretch widens the next load, which
    overflows into a dense one and is repeated; a load that keeps nothing moves on without changing the estimate."""
    assert P.simulate([1] * 130, 64, 1, [130]) == (3, 0, 0, 130)
    # 64 words keep 8: keep = 1/8, want = 0.995 * 64 * 8 = 509 -> all 136 left: 1 + 128 kept > 64, repeated with
    # keep = max(129/136, 0.13) -> 67 words (1 + 59 kept): keep = 60/67 -> 71 words, the 69 dense ones left: 69 > 64,
    # repeated with keep = max(1, 0.94) in loads of 64 and 5
    kpw = ([0] * 7 + [1]) * 9 + [1] * 128
    assert P.simulate(kpw, 64, 1, [len(kpw)]) == (6, 2, 0, 137)
    assert P.simulate([0] * 200 + [1], 64, 1, [201]) == (4, 0, 3, 1)
    assert P.simulate([65], 64, 65, [1]) == "E_OVERFLOW"
    assert P.item_cuts(3400, 64, 1)["doubling"][:10] == [4, 8, 16, 32, 64, 128, 256, 512, 1024, 1024]
    assert P.item_cuts(10, 64, 1025) == {"doubling": [1] * 10, "whole": [10], "fixed": [1] * 10}


def test_swing():
    f = P.swing()
    kpw, segs = f["kept_per_word"], f["segments"]
    assert 3400 <= len(f["words"]) <= 3800 and 1650 <= f["candidates"] <= 1750
    assert len(f["lines"]) == f["candidates"] + 1 == len(f["psk"]) + 1
    assert {len(w) for w, k in zip(f["words"], kpw) if not k} == set(P.JUNK_LENGTHS)
    assert any(_share(kpw, at) <= 0.15 for at in range(len(kpw) - 64))
    assert any(_share(kpw, at) == 1.0 for at in range(len(kpw) - 64))
    assert [k for k, _, _ in segs] == ["sparse", "dense", "sparse", "dense", "junk"]
    assert segs[0][2] > 16 * 64 and segs[1][1] == segs[0][1] + segs[0][2]  # dense directly after a long sparse one
    assert all(kpw[i] for i in range(segs[1][1], segs[1][1] + segs[1][2]))
    tail = segs[-1]
    assert tail[2] > 16 * 64 and tail[1] + tail[2] == len(kpw) and not any(kpw[tail[1]:])
    for cap in BATCHES:
        for cut, res in _sims(kpw, cap, 1).items():
            assert res != "E_OVERFLOW", (cap, cut)
            loads, over, empty, cands = res
            assert over >= 3 and empty >= 1 and cands == f["candidates"], (cap, cut, res)


def test_all_kept():
    f = P.all_kept()
    assert len(f["words"]) == 5 * 64 + 1 == len(set(f["words"])) == f["candidates"]
    assert all(8 <= len(w) <= 63 for w in f["words"])
    for cap in BATCHES:
        for cut, res in _sims(f["kept_per_word"], cap, 1).items():
            assert res != "E_OVERFLOW" and res[1:] == (0, 0, f["candidates"]), (cap, cut, res)
    assert P.simulate(f["kept_per_word"], 64, 1, [321])[0] == 6


def test_rules_swing():
    f = P.rules_swing()
    nr = len(f["rules"])
    assert nr == 8 and f["outcomes"] == {"reject", "short", "long", "kept"}
    assert any(len(ids) > 1 for ids in f["by_psk"].values())  # two rules, one candidate
    assert sum(len(ids) for ids in f["by_psk"].values()) == f["candidates"] > len(f["psk"])
    kpw = f["kept_per_word"]
    assert any(sum(kpw[at:at + 32]) <= 0.2 * 32 * nr for at in range(len(kpw) - 32))   # a sparse run
    assert any(sum(kpw[at:at + 12]) >= 0.85 * 12 * nr for at in range(len(kpw) - 12))  # a dense run
    for cap in BATCHES:
        for cut, res in _sims(kpw, cap, nr).items():
            assert res != "E_OVERFLOW", (cap, cut)
            loads, over, empty, cands = res
            assert over >= 3 and empty >= 1 and cands == f["candidates"], (cap, cut, res)


def test_hybrid_narrow():
    f = P.hybrid_narrow()
    kept = [w for w in f["words"] if 7 <= len(w) <= 62]
    assert f["K"] == 10 and f["candidates"] == 10 * len(kept)
    assert {len(w) for w in f["words"]} >= {0, 6, 7, 62, 63, 64, 300}
    for mode in (6, 7):
        assert len(f[mode]["psk"]) == f["candidates"] and len(f[mode]["lines"]) == f["candidates"] + 1
    assert f[6]["psk"][0] == kept[0] + b"0" and f[7]["psk"][9] == b"9" + kept[0]
    for cut, res in _sims(f["kept_per_word"], 64, 10).items():
        assert res != "E_OVERFLOW", cut
        loads, over, empty, cands = res
        assert over >= 1 and empty >= 1 and cands == f["candidates"], (cut, res)


@pytest.mark.parametrize("K", [64, 65])
def test_hybrid_edge(K):
    f = P.hybrid_edge(K)
    assert f["K"] == K and f["candidates"] == 3 * K
    cands = P.mask_candidates(f["mask"], f["custom"])
    assert (cands[0], cands[1], cands[-1]) == ((b"00", b"01", b"77") if K == 64 else (b"a0", b"a1", b"eC"))
    for mode in (6, 7):
        assert len(f[mode]["psk"]) == 3 * len({0, 63, K - 1})
    if K == 64:  # stays in the sizing loop: one word per load, the estimate never moves
        for cut, res in _sims(f["kept_per_word"], 64, K).items():
            assert res == (len(f["words"]), 0, len(f["words"]) - 3, 3 * K), (cut, res)


@pytest.mark.parametrize("A", [64, 63])
def test_combi_edge(A):
    f = P.combi_edge(A, 0)
    g = P.combi_edge(A, 1)
    assert len(f["amp"]) == A and f["amp"] == g["amp"] and f["words"] == g["words"]
    assert f["candidates"] == g["candidates"] == len(f["psk"]) <= 1500
    assert f["psk"][0] == f["words"][1] + f["amp"][32] and g["psk"][0] == f["amp"][32] + f["words"][1]
    loads, kpw = f["loads"], f["kept_per_word"]
    assert sum(n for _, n, _ in loads) == len(kpw) and sum(k for _, _, k in loads) == f["candidates"]
    assert all(k <= 64 for _, _, k in loads) and any(k == 0 for _, _, k in loads)
    # the running sum lands on exactly a batch, and the loop breaks before a word that would make it a batch + 1
    assert any(k == 64 for _, _, k in loads)
    assert any(first + n < len(kpw) and k + kpw[first + n] == 65 for first, n, k in loads)
    assert any(n == 16 * 64 // A for _, n, _ in loads)  # the bound on a fill-mode load's raw pairs ends a load too


@pytest.mark.parametrize("nrules", [64, 65, 1025])
def test_rules_wide(nrules):
    f = P.rules_wide(nrules)
    assert len(f["rules"]) == nrules and f["candidates"] == 6 * nrules
    at = {(v // nrules, v % nrules) for v in f["plants"].values()}
    assert len(at) == len(f["plants"]) == len(f["psk"])
    assert {(w, r) for w in (0, 5) for r in range(nrules)} <= at
    some = {0, 63, 64, nrules - 1} & set(range(nrules))
    assert {(w, r) for w, r in at if 0 < w < 5} == {(w, r) for w in (1, 2, 3, 4) for r in some}
    assert len(some) == {64: 2, 65: 3, 1025: 4}[nrules]
    for cut, res in _sims(f["kept_per_word"], 64, nrules).items():
        # the sizing loop alone gives up on a word whose kept results pass the batch: with more rules than the batch
        # the library goes one word at a time over rule ranges instead (rule_window_loads)
        assert res == ((6, 0, 0, 6 * nrules) if nrules == 64 else "E_OVERFLOW"), (cut, res)
    assert P.rule_window_loads([len(w) for w in f["words"]], 64, nrules) == 6 * -(-nrules // 64)
    assert P.rule_window_loads([0, 8, 257, 256], 64, 65) == 4


def test_fixtures_build_quickly():
    """Every fixture from scratch (the oracle derives every plant's PMK) in a few seconds."""
    for fn in (P.swing, P.all_kept, P.rules_swing, P.hybrid_narrow, P.hybrid_edge, P.combi_edge, P.rules_wide):
        fn.cache_clear()
    P._PMK.clear()
    t = time.monotonic()
    P.swing(), P.all_kept(), P.rules_swing(), P.hybrid_narrow()
    for K in (64, 65):
        P.hybrid_edge(K)
    for A in (64, 63):
        for side in (0, 1):
            P.combi_edge(A, side)
    for n in (64, 65, 1025):
        P.rules_wide(n)
    took = time.monotonic() - t
    print("fixtures built in %.1f s" % took)
    assert took < 30, took
