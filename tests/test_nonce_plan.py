"""The hashcat-nonce-window plans of tests/nonce_plan.py, checked without a GPU: the model's list lengths against the
library's parser, every plan's own coverage claims, and the equality of windows that licenses the PHP oracle as the
reference.  (The oracle's agreement with the model is asserted while a plan is built: building one is that test.)"""
import time

import pytest

import dwpa_amd
from dwpa_amd import _lib as L
from oracle import oracle as O
from tests import check_recall as C
from tests import nonce_plan as N


@pytest.fixture(scope="module", params=N.PLANS)
def plan(request):
    return N.plan(request.param)


def test_windows_are_the_same_ordered_list():
    """Without a restricting message pair the hashcat window +-nec is PHP's window +-nec (nc = 2 * nec - 2), attempt
    for attempt; nc = 2 * nec, which the plans hand the oracle, is that list and +-(nec + 1) behind it."""
    for nec in (1, 2, 8, 16, 64):
        for mp in (0x00, 0x80, 0x02, 0x60):
            assert N.hashcat_attempts(nec, mp)[1:] == C.attempts(2 * nec - 2)[1:], (nec, mp)
            assert N.hashcat_attempts(nec, mp) == C.attempts(2 * nec)[:1 + 4 * nec]
    assert N.hashcat_attempts(0, 0) == [(0, None)] == C.attempts(0)[:1]
    assert N.hashcat_attempts(8, 0x20)[1:5] == [(1, "LE"), (-1, "LE"), (2, "LE"), (-2, "LE")]
    assert N.hashcat_attempts(8, 0xc0)[1:5] == [(1, "BE"), (-1, "BE"), (2, "BE"), (-2, "BE")]
    assert N.hashcat_attempts(8, 0x70) == [(0, None)]


def test_plans_build_quickly():
    """Every plan, the oracle's asserts included: PMKs are derived once per (ESSID, word), the oracle gets the PMK."""
    N.plan.cache_clear()
    N.dictionary.cache_clear()
    t = time.perf_counter()
    rows = sum(len(N.plan(name)["rows"]) for name in N.PLANS)
    dt = time.perf_counter() - t
    print("%d rows of %d plans built in %.2f s" % (rows, len(N.PLANS), dt))
    assert dt < 20, dt


def test_the_dictionary():
    d = N.dictionary()
    words, kept = d["words"], d["kept"]
    assert len(kept) == N.NKEPT == 130 and kept == [i for i, w in enumerate(words) if 8 <= len(w) <= 63]
    assert kept != list(range(130)) and kept[0] > 0  # ids != slots, from the first slot on
    assert {len(w) for i, w in enumerate(words) if i not in kept} == {0, 7, 64, 65, 300}
    assert len({words[i] for i in kept}) == 130
    assert (len(words[kept[0]]), len(words[kept[129]])) == (8, 63)
    assert N.POS == (0, 63, 64, 127, 128, 129) and set(N.CONTROL_POS) == {63, 64}
    assert sorted(len(e) for e in N.ESSIDS) == [5, 32]


def test_attempt_counts_equal_the_parsers(plan):
    """parse_m22000(...)["attempts"] in hashcat mode is the length of the model's list, for every row; a row has one
    attempt list (also the short-ANONCE ones: nothing is carried from key to key)."""
    lens = set()
    for r in plan["rows"]:
        info = dwpa_amd.parse_m22000(r["line"], plan["nec"], L.DWPA_NC_HASHCAT)
        n = len(N.hashcat_attempts(plan["nec"], r["mp"]))
        assert info["attempts"] == n and info["lists"] == 1 and info["keyver"] == r["kv"], r["tag"]
        assert n in (1, 1 + 2 * plan["nec"], 1 + 4 * plan["nec"])
        lens.add(n)
    for k, _ in plan["controls"]:
        assert dwpa_amd.parse_m22000(plan["lines"][k], plan["nec"], L.DWPA_NC_HASHCAT)["type"] == 1
    if plan["name"] == "message_pair":
        assert lens == {1, 17, 33}
    if plan["name"] == "tails":
        assert lens == {17, 33}


def test_layout(plan):
    """Rows alternate between the ESSIDs; every (keyver, nonce order) is there, read back from the lines, with both
    ESSIDs; its found rows use every position (as many distinct ones as it has rows, where those are fewer than 6);
    EAPOL lengths cycle, keyver 3 through both cmac_complete values; every hit is one (line, candidate)."""
    p = plan
    rows = p["rows"]
    assert [r["essid"] for r in rows] == [i % 2 for i in range(len(rows))]
    assert len(p["lines"]) == len(rows) + 2 and len(set(p["lines"])) == len(p["lines"])
    assert p["classes"] == {1, 2, 3}
    for r in rows:
        f = r["line"].split(b"*")
        assert bytes.fromhex(f[5].decode()) == N.ESSIDS[r["essid"]] and N.line_fields(r["line"])[0] == r["kv"]
        assert C.line_swap(r["line"]) == r["swap"]
        assert r["psk"] == p["words"][p["kept"][r["pos"]]] and r["pos"] in N.POS
    big = p["name"] in ("every_8", "every_16", "wide_64", "message_pair", "tails", "short_anonce")
    for kv in N.KEYVERS:
        for swap in (False, True):
            mine = [r for r in rows if r["kv"] == kv and r["swap"] == swap]
            found = [r for r in mine if r["want"]]
            assert found and {r["essid"] for r in mine} == {0, 1}, (kv, swap)
            assert len({r["pos"] for r in found}) == min(6, len(found)), (kv, swap)
            if big:
                assert {r["pos"] for r in found} == set(N.POS), (kv, swap)
        lens = {r["eapol_len"] for r in rows if r["kv"] == kv}
        assert set(N.EAPOL_LENS) <= lens <= set(N.EAPOL_LENS_KV3 if kv == 3 else N.EAPOL_LENS), (kv, lens)
        if big:
            assert lens == set(N.EAPOL_LENS_KV3 if kv == 3 else N.EAPOL_LENS), (kv, lens)
    assert {len(N.line_fields(r["line"])[2]) % 16 == 0 for r in rows if r["kv"] == 3} == {False, True}
    assert len({h[:2] for h in p["hits"]}) == len(p["hits"]) == sum(1 for r in rows if r["want"]) + 2
    assert {h[0] for h in p["hits"] if h[2] is None} == {k for k, _ in p["controls"]}
    assert N.hits_within(p, 130) == p["hits"]
    early = N.hits_within(p, 64)
    assert {p["kept"].index(h[1]) for h in early} <= {0, 63} and {p["kept"].index(h[1]) for h in p["hits"] - early} \
        <= {64, 127, 128, 129}


def test_every_index_is_planted():
    """every_8, every_16, small_*: every attempt index of the window, per keyver and nonce order; wide_64: the seven
    chosen ones; each reported at the planted index."""
    for name, indices in (("every_8", range(33)), ("every_16", range(65)), ("wide_64", N.WIDE_INDICES),
                          ("small_0", range(1)), ("small_1", range(5))):
        p = N.plan(name)
        att = N.hashcat_attempts(p["nec"], 0)
        assert len(att) == {"every_8": 33, "every_16": 65, "wide_64": 257, "small_0": 1, "small_1": 5}[name]
        for kv in N.KEYVERS:
            for swap in (False, True):
                got = sorted(r["want"][0] for r in p["rows"] if r["want"] and r["kv"] == kv and r["swap"] == swap)
                assert got == list(indices), (name, kv, swap)
        for r in p["rows"]:
            if r["want"]:
                assert r["want"][1:] == att[r["want"][0]] == r["plant"]
    assert {r["mp"] for r in N.plan("every_8")["rows"]} == {0x00, 0x80, 0x02}
    assert len(N.plan("every_8")["rows"]) == 198 and len(N.plan("every_16")["rows"]) == 390


def test_misses_are_the_windows_doing():
    """small_*, edges_*: one past the window in both endians and directions is planted and missed, per keyver and
    nonce order, and +-nec itself is found; message_pair: a forbidden endian is missed.  (That each such line is
    genuine -- the oracle finds its PSK in PHP's wider, unmasked window -- is asserted when the plan is built.)"""
    for name in ("small_0", "small_1", "edges_8", "edges_16"):
        p = N.plan(name)
        nec = p["nec"]
        past = {(nec + 1, "LE"), (-nec - 1, "LE"), (nec + 1, "BE"), (-nec - 1, "BE")}
        for kv in N.KEYVERS:
            for swap in (False, True):
                mine = [r for r in p["rows"] if r["kv"] == kv and r["swap"] == swap]
                assert {r["plant"] for r in mine if not r["want"]} == past, (name, kv, swap)
                if nec:
                    assert {(nec, "LE"), (-nec, "LE"), (nec, "BE"), (-nec, "BE")} <= \
                        {r["plant"] for r in mine if r["want"]}, (name, kv, swap)
    p = N.plan("message_pair")
    assert {r["mp"] for r in p["rows"]} == set(N.MP_MASKS) == {0x10, 0x20, 0x40, 0x60, 0x30, 0x90, 0xa0}
    for mp in N.MP_MASKS:
        for kv in N.KEYVERS:
            found = {r["plant"] for r in p["rows"] if r["mp"] == mp and r["kv"] == kv and r["want"]}
            missed = {r["plant"] for r in p["rows"] if r["mp"] == mp and r["kv"] == kv and not r["want"]}
            assert found | missed == set(N.MP_PLANTS) and not found & missed
            if mp & 0x10:
                assert found == {(0, None)}
            elif mp & 0x60 == 0x20:
                assert found == {(0, None), (3, "LE"), (8, "LE")}
            elif mp & 0x60 == 0x40:
                assert found == {(0, None), (-3, "BE"), (-8, "BE")}
            else:
                assert not missed


def test_twin_tails_report_the_first_allowed_attempt():
    p = N.plan("tails")
    seen = set()
    for r in p["rows"]:
        tail = r["tag"].split("-")[0]
        seen.add((tail, r["mp"], r["want"][1:]))
    assert {s for s in seen if s[0] == "ffffffff"} == {("ffffffff", 0x00, (1, "LE")), ("ffffffff", 0x20, (1, "LE")),
                                                       ("ffffffff", 0x40, (1, "BE"))}
    assert {s for s in seen if s[0] == "00000000"} == {("00000000", 0x00, (-1, "LE")), ("00000000", 0x20, (-1, "LE")),
                                                       ("00000000", 0x40, (-1, "BE"))}
    assert {s[0] for s in seen} == {t for t, _, _ in C.TAILS} and all(s[1] == 0 for s in seen if s[0][:8] not in
                                                                        ("ffffffff", "00000000"))


def test_short_anonce_model():
    """The short-ANONCE plan: ANONCEs of 20 and 31 bytes, every attempt index 0..8 per keyver and nonce order, both
    the lines whose nonce pair the correction lengthens (SNONCE first: bytes 60.. lie past a 52- or 63-byte pair) and
    those it does not; the nine messages of a line are distinct; and the Python oracle agrees with the C oracle's
    index-0 result."""
    p = N.plan("short_anonce")
    assert p["nec"] == 2
    for alen in N.SHORT_LENS:
        for kv in N.KEYVERS:
            for swap in (False, True):
                got = sorted(r["want"][0] for r in p["rows"] if (r["short"], r["kv"], r["swap"]) == (alen, kv, swap))
                assert got == [0, 1, 2, 2, 3, 5, 6, 7, 8], (alen, kv, swap)  # planted 0..8; 4 is 2's twin
    att = N.hashcat_attempts(2, 0)
    assert N.SHORT_TWIN == {4: 2} and (att[2], att[4]) == ((-1, "LE"), (-1, "BE"))
    for r in p["rows"]:
        msgs = N.short_messages(r["line"], 2)
        assert len(msgs) == 9 and len(set(msgs)) == 8 and msgs[2] == msgs[4]
        assert len(N.line_fields(r["line"])[1]) == r["short"]
        assert {len(m) for m in msgs} == ({r["short"] + 32} if r["swap"] else {64} if r["short"] == 31 else {56})
        if r["plant"] == 0 and r["essid"] == 0:
            o = O.py_check_key_m22000(r["line"], [r["psk"]], r["pmk"], 4)
            assert o == [r["psk"], 0, None, r["pmk"]], r["tag"]


def test_c_oracle_agrees_with_python_oracle(plan):
    """A stride of the rows through oracle/oracle.py: the same result as the C oracle's, which confirmed the plan."""
    p = plan
    rows = [r for r in p["rows"] if not r["short"] or r["plant"] == 0]  # short ANONCE: PHP's first attempt only
    for r in rows[::max(1, len(rows) // 12)]:
        c = O.c_check_key_m22000(r["line"], [r["psk"]], r["pmk"], 2 * p["nec"])
        assert c and O.py_check_key_m22000(r["line"], [r["psk"]], r["pmk"], 2 * p["nec"]) == c, r["tag"]


def test_model_hits_at_the_crack_leg_window():
    """The dwpa_crack_files leg runs edges_8, edges_16 and message_pair at nonce_error_corrections = 8: the model,
    re-evaluated at that window, finds edges_16 nowhere and the others as planned."""
    assert N.model_hits(N.plan("edges_16")["rows"], 8) == []
    for name in ("edges_8", "message_pair"):
        p = N.plan(name)
        assert N.model_hits(p["rows"], 8) == [i for i, r in enumerate(p["rows"]) if r["want"]]
    r = N.plan("edges_8")["rows"][0]
    assert N.record(r["line"], r["psk"]).count(b":") >= 4
