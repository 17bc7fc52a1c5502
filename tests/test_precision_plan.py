"""CPU: the precision fixtures of tests/precision_plan.py against the C oracle, against comparers with a defect, and
through the library's host backend.

The GPU tests (tests/test_gpu_precision.py) take their expected results from the plan's model.  Here the oracle is
shown to agree with the model on every line of every fixture -- a one-bit-off target matches with probability 2^-128,
which is asserted, not assumed -- and the fixture is shown to have teeth: every comparer that is blind to one bit, one
byte or one word of the target, or reads one word byte-swapped, accepts a line the plan says must be missed, for every
line kind.  Then the host backend's comparison sites (host_check.cpp: the 4-wide keyver 1/2 groups, the PMKID path,
keyver 3 / CMAC with its byte-swapped target) answer the same jobs, with SHA-NI / AES-NI and, in a child process, with
the scalar primitives.
"""
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

import dwpa_amd
from dwpa_amd import _lib as L
from dwpa_amd import m22000 as M
from oracle import oracle as O
from tests import nonce_plan as N
from tests import precision_plan as P
from tests.conftest import ROOT

THREADS = min(16, os.cpu_count() or 8)
HOST_FIXTURES = ("single", "wide")  # nc 8 and nc 128
SINGLES = 40


def _oracle_many(jobs):
    with ThreadPoolExecutor(THREADS) as ex:
        return list(ex.map(lambda a: O.c_check_key_m22000(*a), jobs))


def _gpu_present():
    return os.path.exists("/dev/kfd") and os.environ.get("HIP_VISIBLE_DEVICES", "0") != ""


# ---------------------------------------------------------------------------------------------------------------
# the fixture itself
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(P.FIXTURES))
def test_fixture_shape(name):
    """Per kind: the controls, 128 one-bit and 4 byte-swap near-misses, the long-target triple and one zero line per
    ESSID; both frame lengths and every planted correction among the controls AND among the near-misses; the
    dictionary's copies of the PSK at the wave edges."""
    fx = P.fixture(name)
    rows = fx["rows"]
    plants = set(P.PLANTS[fx["variant"]])
    for kind in P.KINDS:
        mine = [r for r in rows if r["kind"] == kind]
        tags = [r["tag"] for r in mine]
        frames = P.FRAME_LENS.get(kind, (None,))
        ncontrol = 1 if kind == "pmkid" else 16
        assert tags.count("control") == ncontrol and tags.count("zero") == len(fx["essids"])
        assert sorted(t for t in tags if t.startswith("bit")) == sorted("bit%d" % b for b in range(128))
        assert sorted(t for t in tags if t.startswith("swap")) == ["swap%d" % w for w in range(4)]
        assert [t for t in tags if t.startswith("long")] == ["long_hit", "long_miss", "long_hit17"]
        assert len(mine) == ncontrol + 128 + 4 + 3 + len(fx["essids"])
        if kind != "pmkid":
            assert {(r["frame"], r["plant"]) for r in mine if r["tag"] == "control"} == \
                {(f, p) for f in frames for p in plants}
            assert {(r["frame"], r["plant"]) for r in mine if r["tag"].startswith("bit")} == \
                {(f, p) for f in frames for p in plants}
            for r in mine:  # the frame in the line is the frame the row names
                assert len(bytes.fromhex(r["line"].split(b"*")[7].decode())) == r["frame"]
        for r in mine:
            t = P.target_of(r["line"])
            if r["tag"].startswith(("bit", "swap")):  # only the target differs from the control
                c = rows[r["control"]]
                assert c["tag"] == "control" and c["true"] == r["true"] and P.with_target(r["line"], c["true"]) == c["line"]
                diff = bytes(a ^ b for a, b in zip(t, r["true"]))
                if r["tag"].startswith("bit"):
                    assert len(t) == 16 and diff == P.flip(bytes(16), int(r["tag"][3:]))
            elif r["tag"] == "long_hit":
                assert len(t) == 20 and t[:16] == r["true"]
            elif r["tag"] == "long_miss":
                assert len(t) == 20 and t[:15] == r["true"][:15] and t[15] == r["true"][15] ^ 1 and \
                    t[16:] == P.target_of(rows[r["control"]]["line"])[16:]
            elif r["tag"] == "long_hit17":
                assert len(t) == 20 and t[:16] == r["true"] and t[16:] != P.LONG_TAIL
    w = fx["words"]
    assert len(w) == 130 and all(8 <= len(x) <= 63 for x in w)
    assert [i for i, x in enumerate(w) if x == fx["psk"]] == [0, 63, 64, 129] and len(set(w)) == 127
    assert 520 <= len(rows) <= 610


@pytest.mark.parametrize("name", sorted(P.FIXTURES))
def test_lines_are_distinct(name):
    """The lines are pairwise distinct, no line that must miss carries the true target of ANY line of the fixture (as
    its first 16 bytes), and a zero line's target is no hit line's."""
    fx = P.fixture(name)
    lines = fx["lines"]
    assert len(set(lines)) == len(lines)
    true = {r["true"] for r in fx["rows"] if r["true"] is not None}
    true |= {P.target_of(r["line"])[:16] for r in fx["rows"] if r["hit"]}
    for r in fx["rows"]:
        if not r["hit"]:
            assert P.target_of(r["line"])[:16] not in true, (r["kind"], r["tag"])


def test_planted_attempts_cover_every_residue():
    """The planted corrections lie at every residue mod 4 of the attempt list, in both endians (an endian reaches two
    residues: +k LE 1, -k LE 2, +k BE 3, -k BE 0), inside PHP's window at the fixture's nc; the list is the model's
    (nonce_plan.hashcat_attempts), which test_nonce_plan ties to PHP's order."""
    for variant, plants in P.PLANTS.items():
        att = N.hashcat_attempts(P.halfnc(P.NC[variant]), 0)
        idx = [att.index(p) for p in plants]
        assert {(i % 4, p[1]) for i, p in zip(idx, plants)} == {(1, "LE"), (2, "LE"), (3, "BE"), (0, "BE")}
        assert max(idx) == len(att) - 1  # the window's last attempt is planted
    assert len(N.hashcat_attempts(P.halfnc(8), 0)) == 21 and len(N.hashcat_attempts(P.halfnc(128), 0)) == 261


# ---------------------------------------------------------------------------------------------------------------
# the oracle agrees with the model
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_results():
    """name -> the oracle's result of every job of the fixture, computed once."""
    return {name: _oracle_many(P.jobs(P.fixture(name))) for name in P.FIXTURES}


@pytest.mark.parametrize("name", sorted(P.FIXTURES))
def test_oracle_agrees_with_the_plan(oracle_results, name):
    """Every control and long-target hit: [PSK, nc, endian, pmk] with the planted attempt.  Every near-miss, long
    miss and zero line: the oracle's miss value.  Both routes (keys [decoy, PSK, decoy] with a derive, and the PMK
    handed over) occur among the hits and among the misses of every kind."""
    fx = P.fixture(name)
    js = P.jobs(fx)
    exp, key_index = P.job_results(fx, js)
    got = oracle_results[name]
    bad = [i for i, (g, e) in enumerate(zip(got, exp)) if g != e]
    assert not bad, P.describe(fx, bad[:5])
    for r, g in zip(fx["rows"], got):
        assert (g is not P.MISS) == r["hit"] == (r["tag"] in ("control", "long_hit", "long_hit17"))
    for kind in P.KINDS:
        for hit in (True, False):
            routes = {bool(j[2]) for r, j in zip(fx["rows"], js) if r["kind"] == kind and r["hit"] == hit}
            assert routes == {False, True}, (kind, hit)
    assert {k for k in key_index if k is not None} == {0, 1}


def test_oracle_takes_the_zero_lines_with_the_zero_pmk():
    """The zero lines are sound: with the zero PMK handed over (common.php:592) the oracle reports them."""
    for name in ("single", "wide", "multi"):
        js, exp = P.zero_jobs(P.fixture(name))
        assert len(js) == 4 * len(P.fixture(name)["essids"])
        assert _oracle_many(js) == exp


def test_model_scan_hits_and_records():
    """What the GPU tests derive from the plan: a scan's hit set (every hit row x every copy of the PSK loaded) and a
    crack call's records (one per hit row; a record holds the first 16 target bytes and the MACs, so the hit rows of one frame give the same
    record: 2 distinct ones for the PMKID kind, 3 per key version)."""
    fx = P.fixture("single")
    nhit = sum(r["hit"] for r in fx["rows"])
    assert nhit == 3 + 3 * (16 + 2) == 57
    assert len(P.scan_hits(fx)) == 4 * nhit and len(P.scan_hits(fx, nwords=1)) == nhit
    assert len(P.scan_hits(fx, nwords=65)) == 3 * nhit
    rec = P.records(fx)
    assert len(rec) == nhit and len(set(rec)) == 2 + 3 * 3


# ---------------------------------------------------------------------------------------------------------------
# the fixture has teeth
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(P.FIXTURES))
def test_every_weak_comparer_is_detected(name):
    """A comparer blind to one bit (128), one byte (16) or one word (4) of the target, or reading one word
    byte-swapped (4): each accepts at least one line of every kind that the plan says must be missed -- a verifier
    with that defect reports it, and the tests that compare with the plan fail.  The sound comparer accepts exactly
    the plan's hits."""
    fx = P.fixture(name)
    rows = [r for r in fx["rows"] if r["true"] is not None]  # the PSK's value for a zero line is not part of the plan
    sound = P.weak_match(())
    for r in rows:
        assert sound(P.target_of(r["line"]), r["true"]) == r["hit"], (r["kind"], r["tag"])
    comparers = P.weak_comparers()
    assert len(comparers) == 128 + 16 + 4 + 4
    detected = 0
    for kind in P.KINDS:
        must_miss = [r for r in rows if r["kind"] == kind and not r["hit"]]
        assert len(must_miss) == 128 + 4 + 1
        for cname, match in comparers.items():
            accepted = [r["tag"] for r in must_miss if match(P.target_of(r["line"]), r["true"])]
            assert accepted, (kind, cname, "slips through")
            detected += 1
            if cname.startswith("bit"):  # and it is the line with that very bit flipped
                assert cname in accepted
    assert detected == 4 * (128 + 16 + 4 + 4)


def test_byte_swap_needs_lines_of_its_own():
    """Why the swap lines exist: no one-bit near-miss satisfies a byte-swapped comparer."""
    fx = P.fixture("single")
    for w in range(4):
        match = P.swapped_match(w)
        for r in fx["rows"]:
            if r["tag"].startswith("bit"):
                assert not match(P.target_of(r["line"]), r["true"])


# ---------------------------------------------------------------------------------------------------------------
# the host backend
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture
def _host_backend(monkeypatch):
    monkeypatch.setenv("DWPA_CPU_FALLBACK", "1")
    monkeypatch.setenv("DWPA_HOST_MAX_PMKS", "1000000000")
    yield


def _assert_host():
    if not _gpu_present():
        assert M.check_stats()["backend"] in (L.DWPA_BACKEND_HOST_SMALL, L.DWPA_BACKEND_HOST_FALLBACK)


@pytest.mark.parametrize("name", HOST_FIXTURES)
def test_host_backend_equals_the_oracle(_host_backend, oracle_results, name):
    """All jobs through dwpa_check_batch and the first 40 through dwpa_check_m22000, at nc 8 and at nc 128, derived
    and caller PMKs: exactly the oracle's list."""
    fx = P.fixture(name)
    js = P.jobs(fx)
    exp = oracle_results[name]
    got = dwpa_amd.check_batch(js)
    _assert_host()
    bad = [i for i, (g, e) in enumerate(zip(got, exp)) if g != e]
    assert not bad, P.describe(fx, bad[:5])
    st = M.check_stats()
    assert st["jobs"] == len(js) and st["hits"] == sum(1 for e in exp if e)
    for i in range(SINGLES):
        assert dwpa_amd.check_key_m22000(*js[i]) == exp[i], P.describe(fx, [i])
    assert {bool(j[2]) for j in js[:SINGLES]} == {False, True}
    zj, zexp = P.zero_jobs(fx)
    assert dwpa_amd.check_batch(zj) == zexp


_SCALAR_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import dwpa_amd
from tests import precision_plan as P
out = {}
for name in sys.argv[2:]:
    fx = P.fixture(name)
    js = P.jobs(fx)
    exp, _ = P.job_results(fx, js)
    got = dwpa_amd.check_batch(js)
    bad = [i for i, (g, e) in enumerate(zip(got, exp)) if g != e]
    bad += [i for i in range(40) if dwpa_amd.check_key_m22000(*js[i]) != exp[i]]
    zj, zexp = P.zero_jobs(fx)
    out[name] = {"jobs": len(js), "bad": repr(P.describe(fx, bad[:5])) if bad else "",
                 "zero_ok": dwpa_amd.check_batch(zj) == zexp}
print(json.dumps(out))
"""


def test_scalar_primitives_subprocess(oracle_results):
    """DWPA_HOST_SIMD=0: the same jobs on the portable SHA-1 / SHA-256 / MD5 / AES-128, in a child process (the switch
    is read once).  The child compares with the plan's model, which the oracle equals here."""
    for name in HOST_FIXTURES:
        fx = P.fixture(name)
        assert oracle_results[name] == P.job_results(fx, P.jobs(fx))[0]
    env = dict(os.environ, DWPA_HOST_SIMD="0", DWPA_CPU_FALLBACK="1", DWPA_HOST_MAX_PMKS="1000000000")
    r = subprocess.run([sys.executable, "-c", _SCALAR_CHILD, ROOT] + list(HOST_FIXTURES), capture_output=True,
                       text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    for name in HOST_FIXTURES:
        assert out[name] == {"jobs": len(P.fixture(name)["rows"]), "bad": "", "zero_ok": True}, name
