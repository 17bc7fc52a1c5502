"""The retirement plans of tests/retire_plan.py, checked without a GPU: the schedules the GPU tests rely on, the model's
counts, and the oracle's agreement with itself."""
import pytest

import dwpa_amd
from oracle import oracle as O
from tests import retire_plan as P
from tests.test_gpu_chain import Chain


@pytest.fixture(scope="module", params=["A", "B"])
def plan(request):
    return P.plan(request.param)


def test_active_sequences():
    """|active_b| before every batch, the launch counts, and the counters the model gives for one worker."""
    a, b = P.plan("A"), P.plan("B")
    assert a["active"] == [8, 7, 7, 7, 7, 7, 7, 7, 6, 6, 6, 6, 6, 4, 3, 2] and a["launches"] == [1] * 16
    assert a["uncracked"][0] == a["crackable"] + 1 == 86 and a["uncracked"][-1] == 12 + 3 + 1
    assert tuple(b["active"]) == P.B_ACTIVE == (40, 33, 32, 17, 16, 15, 1, 1)
    assert tuple(b["launches"]) == P.B_LAUNCHES == (3, 3, 2, 2, 1, 1, 1, 1)
    assert b["launch_sizes"][:4] == [[14, 13, 13], [11, 11, 11], [16, 16], [9, 8]]
    assert b["work"] == {"groups_derived": sum(P.B_ACTIVE), "pbkdf2_launches": 14, "line_rows": sum(b["uncracked"])}
    assert a["work"] == {"groups_derived": sum(a["active"]), "pbkdf2_launches": 16, "line_rows": sum(a["uncracked"])}
    for p in (a, b):  # a strict drop after the first batch, and a line that keeps the run going to the keyspace's end
        assert p["active"][1] < p["active"][0] and p["nbatches"] * p["batch_size"] == p["keyspace"]
        assert sum(1 for k, bt in enumerate(p["batch"]) if bt is None and not p["never"][k]) == 1


def test_plan_a_patterns():
    """Every retirement pattern of plan A, read back from the schedule in the scan's line order."""
    p = P.plan("A")
    assert p["groups"] == list(P.A_ESSIDS.values()) and len(p["groups"][4]) == 52
    assert p["table"] != sorted(p["table"])  # the file is shuffled
    sched = {}
    for i in p["table"]:
        if not p["never"][i] and p["batch"][i] is not None:
            sched.setdefault(p["essid"][i], []).append((p["cls"][i], p["batch"][i]))
    e = P.A_ESSIDS
    assert [c for c, _ in sched[e["first"]]] == [0] * 3 + [1] * 3 + [2] * 3 + [3] * 3
    assert {b for _, b in sched[e["first"]]} == {0} and {b for _, b in sched[e["until_end"]]} == {15}
    assert [b for _, b in sched[e["front_to_back"]]] == list(range(1, 13))
    assert [b for _, b in sched[e["back_to_front"]]] == list(range(12, 0, -1))
    io = [b for _, b in sched[e["inside_out"]]]
    assert all(io[r + 1] < io[r] < io[r + 2] for r in (0, 3, 6, 9)) and len(set(io)) == 12
    ca = sched[e["class_at_once"]]
    assert {b for c, b in ca if c == 2} == {3} and all(b > 3 for c, b in ca if c != 2)
    assert all(len({b for c, b in ca if c == k}) == 1 for k in range(4))
    assert sched[e["single"]] == [(3, 7)]
    nf = [i for i in range(len(p["lines"])) if p["essid"][i] == e["never_finishes"]]
    assert sorted(p["cls"][i] for i in nf if p["never"][i]) == [0, 1]  # a short PMKID and a short MIC
    assert [p["psk"][i] for i in nf if p["batch"][i] is None and not p["never"][i]] == [P.A_OUTSIDE]
    assert set(P.A_OUTSIDE) - set(b"01")
    for i in nf:
        info = dwpa_amd.parse_m22000(p["lines"][i], P.NC)
        assert info["never_matches"] == p["never"][i], i


def test_every_psk_lies_in_its_batch(plan):
    """The candidate at a line's index is its PSK, and the index lies in the scheduled batch; PSKs are unique, also as
    HMAC keys (no two differ only by trailing NULs)."""
    p = plan
    live = [k for k in range(len(p["lines"])) if p["batch"][k] is not None]
    assert len(live) == p["crackable"] == len(p["records"])
    for k in live:
        assert p["index"][k] // p["batch_size"] == p["batch"][k], k
        if p["name"] == "A":
            assert p["psk"][k] == P.a_candidate(p["index"][k]) == b"%010d" % int(format(p["index"][k], "b"))
            assert dwpa_amd.mask_candidate(p["mask"], p["index"][k], p["custom"]) == p["psk"][k]
    psks = [p["psk"][k] for k in range(len(p["lines"])) if not p["never"][k]]
    assert len(psks) == p["crackable"] + 1
    assert len({q.rstrip(b"\0") for q in psks}) == len(psks) and all(8 <= len(q) <= 63 for q in psks)
    assert len({p["index"][k] for k in live}) == len(live)


def test_chain_kept_set_equals_the_reference():
    """Plan B's chain through the reference expander (tests/test_gpu_chain.py Chain).  Whether a candidate is kept
    follows from the lengths of its two words alone and every word of list A has 3 bytes, so the kept continuations
    of one A-word are those of every A-word: the first and the last row are expanded whole, as are both sides of every
    batch boundary, and every planted index."""
    p = P.plan("B")
    la, lb = p["chain"]
    ch = Chain([la, lb], ())
    assert ch.k == p["keyspace"] == 1 << 23 and {len(w) for w in la} == {3}
    assert len(set(la)) == len(la) and len(set(lb)) == len(lb)
    long_b = sorted(P.B_LONG)
    assert [j for j, w in enumerate(lb) if len(w) != 3] == long_b == [0, 1000, 2047]
    for a in (0, len(la) - 1):
        assert ch.kept(a * len(lb), len(lb)) == [(a * len(lb) + j, la[a] + lb[j]) for j in long_b]
    rows = p["batch_size"] // len(lb)
    assert p["kept_per_batch"] == rows * len(long_b) == 1536
    for b in range(1, p["nbatches"]):  # the last A-word of batch b - 1 and the first of batch b
        first = b * p["batch_size"] - len(lb)
        assert [i for i, _ in ch.kept(first, 2 * len(lb))] == [first + r * len(lb) + j for r in (0, 1) for j in long_b]
    for k, i in enumerate(p["index"]):
        if i is not None:
            assert ch.candidate(i) == (p["psk"][k], True), k
    outside = next(p["psk"][k] for k in range(len(p["lines"])) if p["batch"][k] is None)
    assert outside[:3] in la and outside[3:] not in lb and len(outside) == 9


def test_c_oracle_agrees_with_python_oracle(plan):
    """A stride of the lines through oracle/oracle.py: the same result as the C oracle's, which built the plan."""
    p = plan
    for k in range(0, len(p["lines"]), 8):
        psk = p["psk"][k] or b"no-such-psk"
        c = O.c_check_key_m22000(p["lines"][k], [psk], p["pmk"][k], P.NC)
        assert O.py_check_key_m22000(p["lines"][k], [psk], p["pmk"][k], P.NC) == c, k
        assert bool(c) == (not p["never"][k])
