"""CPU: tests/pmk_plan.py is what tests/test_gpu_pmk.py takes it for.  The ESSID list is the one the oracle accepts and
the library's parser agrees; the oracle's tables are hashlib's PBKDF2; the sample sets hold their structural positions at
several device sizes; the plans have the shapes the GPU cases claim (salt block counts per launch and per wave); and
compare() catches each of five deliberately wrong PBKDF2 models on every table the slip can touch."""
import hashlib
import random

import numpy as np
import pytest

from dwpa_amd import _lib as L
from dwpa_amd import m22000 as M
from tests import pmk_plan as P

CUS = 256  # the tables are a function of the CU count: an MI355X's here, others where only positions are counted


@pytest.fixture(scope="module")
def tb():
    t = P.Tables(CUS)
    print("oracle: %d PMKs in %.2f s (%.0f PMK/s)" % (len(t.pmk), t.seconds, len(t.pmk) / t.seconds))
    return t


# ---------------------------------------------------------------------------------------------------------------
# ESSIDs
# ---------------------------------------------------------------------------------------------------------------
def test_essid_list_is_the_oracles_decision():
    """Every length 0..32, 33, 51, 52, 115, 116 once; the oracle refuses the empty ESSID alone (PHP's valid_hex('') is
    false), so the list drops it; the library's parser gives the same verdict on the same lines."""
    assert [len(e) for e in P.ALL_ESSIDS] == list(range(33)) + [33, 51, 52, 115, 116]
    assert len(set(P.ALL_ESSIDS)) == len(P.ALL_ESSIDS)
    assert tuple(e for e in P.ALL_ESSIDS if P.oracle_takes(e)) == P.ESSIDS
    assert P.REFUSED == (b"",) and len(P.ESSIDS) == 37
    for e in P.ALL_ESSIDS:
        info = M.parse_m22000(P.scan_line(e))
        assert (info == L.DWPA_E_HEX) if e in P.REFUSED else (info["essid_len"] == len(e)), e
    used = set(b"".join(P.ESSIDS))
    assert {0x00, 0x0a, 0xff} <= used
    assert any(e[:1] == b"\0" for e in P.ESSIDS) and any(e[-1:] == b"\0" for e in P.ESSIDS)
    assert (P.by_len(1), P.by_len(32)) == P.SLOT_ESSIDS


def test_salt_block_boundaries():
    """51 | 52 and 115 | 116 bytes are where the salt message takes another SHA-1 block, by SHA-1's padding rule."""
    for n in (1, 32, 33, 51, 52, 115, 116):
        msg = 64 + n + 4  # the key block, the ESSID, INT(i)
        blocks = -(-(msg + 1 + 8) // 64)  # 0x80 and the 64-bit length must fit
        assert P.nsalt(bytes(n)) == blocks - 1, n
    assert [P.nsalt(bytes(n)) for n in (1, 51, 52, 115, 116)] == [1, 1, 2, 2, 3]


# ---------------------------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------------------------
def test_tables_are_hashlibs(tb):
    """Four candidates of every ESSID of every table: the first, the last and two seeded ones."""
    rng = random.Random(0x7ab1e)
    checked = 0
    for name, rows in P.requests(CUS).items():
        for e, keys in rows:
            for k in {keys[0], keys[-1], rng.choice(keys), rng.choice(keys)}:
                assert tb.pmk[(e, k)] == hashlib.pbkdf2_hmac("sha1", k, e, 4096, 32), (name, e, k)
                checked += 1
    assert checked >= 4 * len(P.ESSIDS)
    w = tb.words(P.ESSID_1, [P.psk(P.SWEEP_FIRST)])
    assert w.shape == (8, 1) and w.dtype == np.uint32
    assert b"".join(int(x).to_bytes(4, "big") for x in w[:, 0]) == tb.pmk[(P.ESSID_1, P.psk(P.SWEEP_FIRST))]


def test_table_sizes(tb):
    req = P.requests(CUS)
    count = {name: sum(len(k) for _, k in rows) for name, rows in req.items()}
    assert count["slots"] == 2 * (P.SLOTS + len(P.COUNTS)) and count["sweep"] == 37 * (P.SWEEP + 1)
    assert count["queue"] == 1024 and count["groups"] == 3 * 512 and count["check"] == P.CHECK_JOBS
    assert len(tb.pmk) <= sum(count.values()) <= P.MAX_PMKS
    assert all(len(k) == P.DIGITS for name in ("slots", "sweep", "queue", "groups", "prio_one", "prio_mg")
               for _, keys in req[name] for k in keys)
    assert sorted(P.COUNTS) == [1, 63, 64, 65, 255, 256, 257, 1023, 1087] and P.SLOTS == 4 * 256 + 64


@pytest.mark.parametrize("cus", [256, 304, 64, 36])
def test_samples_hold_their_structural_positions(cus):
    q = P.queue_threshold(cus)
    qc = P.queue_case(cus)
    n, pos = qc["n"], set(qc["sample"])
    assert n == q + 193 and len(pos) == 1024 and all(0 <= p < n for p in pos)
    last_full = n // 64 * 64
    # tests/test_gpu_pbkdf2_queue_lds.py's _sample
    assert {0, 1, 63, 64, 65, 127, 128, 255, 256, q - 64, q - 1, q, last_full - 64, last_full - 1, n - 1,
            q + 1, q + 63, q + 64, last_full} <= pos
    for m in range(q // 8, n, q // 8):
        assert {m - 1, m} <= pos, m
    gc = P.group_case(cus)
    batch = gc["batch"]
    assert batch % 64 == 0 and 3 * batch > q >= 3 * (batch - 64) and gc["n"] == batch - 37
    assert [len(e) for e in gc["essids"]] and {len(e) for e in gc["essids"]} == {1, 52, 116}
    seen = 0
    for c, pos in enumerate(gc["sample"]):
        pos = set(pos)
        assert len(pos) == 512 and all(0 <= p < gc["n"] for p in pos)
        assert {0, 63, 64, 255, 256, gc["n"] - 1} <= pos
        for m in range(q // 8, 3 * batch + 1, q // 8):  # the launch's lane space: group c holds [c, c + 1) * batch
            for lane in (m - 1, m):
                if c * batch <= lane < c * batch + gc["n"]:
                    assert lane - c * batch in pos, (c, m)
                    seen += 1
    assert seen >= 14  # both sides of the seven inner multiples, but for sides in the unloaded tails
    assert len({tuple(p) for p in gc["sample"]}) == 3
    pc = P.prio_cases(cus)
    s = P.sizes(cus)
    assert pc["one"]["batch"] == s["one"]["p"] and pc["mg"]["batch"] == s["mg"]["p"]
    assert 2 * (s["one"]["p"] - 64) <= s["level_lanes"] < 2 * s["one"]["p"] <= 8 * s["level_lanes"]
    assert 6 * (s["mg"]["p"] - 64) <= s["level_lanes"] < 6 * s["mg"]["p"] <= 8 * s["level_lanes"]
    assert {0, 63, 64, 255, 256, pc["one"]["batch"] - 1} <= set(pc["one"]["sample"])


def test_sweep_puts_one_two_and_three_blocks_in_one_launch():
    order = P.group_order(P.ESSIDS)
    ns = [P.nsalt(e) for e in order]
    assert set(ns) == {1, 2, 3}
    assert any(a != b for a, b in zip(ns, ns[1:]))           # neighbouring groups differ
    assert len(order) * 64 <= 1 << 24                         # engine.cpp MG_SLOTS: one launch holds them all
    assert order == sorted(order) and order[0] == b"\x00\x0a"  # byte order, NUL first


@pytest.mark.parametrize("rules", [False, True])
def test_assoc_waves_mix_block_counts(rules):
    ac = P.assoc_case(rules)
    ns = [P.nsalt(e) for e in ac["essid_of"]]
    assert 64 < len(ns) <= 128 and {P.nsalt(e) for e, m in ac["nets"]} == {1, 2, 3}
    assert {len(e) for e, m in ac["nets"]} == {1, 51, 52, 115, 116, 32}
    assert sorted({len(w) for w in ac["plan"].words}) == [1, 2, 3]
    for wave in range(0, len(ns), 64):
        assert set(ns[wave:wave + 64]) == {1, 2, 3}, wave
    nets = [ac["plan"].net_of(i) for i in range(ac["plan"].k)]
    assert max(sum(1 for _ in g) for g in _runs(nets)) <= 3
    assert all(c.endswith(b"!") == rules for c in ac["cands"]) and all(8 <= len(c) <= 63 for c in ac["cands"])
    assert P.PLANT_PSK not in ac["cands"]


def _runs(xs):
    run = []
    for x in xs:
        if run and run[-1] != x:
            yield run
            run = []
        run.append(x)
    if run:
        yield run


def test_check_jobs_cycle_the_lengths():
    jobs = P.check_case()
    assert [len(e) for e, k in jobs[:8]] == [1, 51, 52, 116] * 2 and len(jobs) == 192
    assert len({k for e, k in jobs}) == 192


# ---------------------------------------------------------------------------------------------------------------
# compare() and its teeth
# ---------------------------------------------------------------------------------------------------------------
def test_compare_names_slots_words_and_stale_columns():
    rng = np.random.default_rng(5)
    want = rng.integers(0, 2**32, size=(8, 70), dtype=np.uint32)
    ids = list(range(100, 170))
    assert P.compare(want.copy(), want, ids) == ""
    got = want.copy()
    got[7, 3] ^= 1
    got[:, 69] = 0
    prev = np.zeros_like(want)
    msg = P.compare(got, want, ids, prev)
    assert msg.startswith("2 of 70 PMKs differ; 1 of them stale")
    assert "103: words [7]" in msg and "169 stale: words [0, 1, 2, 3, 4, 5, 6, 7]" in msg
    assert P.compare(got[:, :5], want, ids).startswith("shapes differ")
    assert P.compare(got, want, ids, shown=1).count("words") == 1


# which tables a slip cannot show on: one ESSID only, so no neighbouring group's salt to take
BLIND = {"neighbour_salt": {"queue", "prio_one"}}


def test_the_models_f_is_pbkdf2(tb):
    for e, k in ((P.ESSID_1, P.psk(P.SWEEP_FIRST)), (P.by_len(116), P.psk(P.SWEEP_FIRST + 1))):
        assert P.model_right(k, e, None) == tb.pmk[(e, k)]


@pytest.mark.parametrize("slip", sorted(P.WRONG))
def test_a_wrong_model_is_caught(tb, slip):
    """Per table: the right PMKs with three columns (of different ESSIDs where the table has them) replaced by the
    wrong model's -- far fewer than a wrong kernel would get wrong -- fail compare(), which names exactly them."""
    req = P.requests(CUS)
    assert set(req) == {"slots", "sweep", "queue", "groups", "prio_one", "prio_mg", "check", "assoc_plain",
                        "assoc_rules"}
    for name, rows in req.items():
        keys = tb.names[name]
        want = P.words_of([tb.pmk[x] for x in keys])
        order = [e for e, _ in rows]
        if len(order) == 1:
            assert name in BLIND["neighbour_salt"]
        cols = sorted({0, len(keys) // 2, len(keys) - 1})
        got = want.copy()
        for j in cols:
            e, k = keys[j]
            nb = order[(order.index(e) + 1) % len(order)]
            got[:, j] = P.words_of([P.WRONG[slip](k, e, nb)])[:, 0]
        msg = P.compare(got, want, list(range(len(keys))))
        if name in BLIND.get(slip, ()):
            assert msg == "", (name, slip)
            continue
        assert msg.startswith("%d of %d PMKs differ" % (len(cols), len(keys))), (name, slip, msg)
        if slip == "word7_dropped":
            assert "words [7]" in msg
        if slip == "block2_salt1":
            assert "words [5, 6, 7]" in msg
