"""GPU recall of the server check path: every (key, attempt) item of a check call must be found.

dwpa_check_m22000 / dwpa_check_batch is the path the server trusts for accepting a submitted key, and a hit its
verifiers lose is reported as "wrong password".  EAPOL lines with >= 64 attempts go to the attempt-parallel verifier
(k_eapol_keys + k_verify_att), whose index arithmetic maps a lane to one (key, attempt) item: item -> (k, a), a
binary search over the segments, the per-key scratch, waves that span two keys, the idle lanes of a segment's last
wave, segments of 16 keys in rank order and the first-hit early exit.  A mistake in any of them loses hits only at
particular (key position, attempt index) pairs.  The plans of tests/check_recall.py plant a hit at EVERY attempt
index of the 261-, 65-, 521- and (key-parallel) 61-attempt windows at chosen key positions, for keyver 1, 2 and 3
and both nonce orders, and every job's result and key_index must equal what the C oracle decided -- bit-exact.

Each test asserts the exact set of verify kernels that ran (the library's dwpa_debug_verify_kernels hook), so a
change to the 64-attempt switch or to queue_verify's buckets fails here instead of quietly moving the plans to the
other verifier.  The runs with the early exit off (one 40-key segment of 163.1 waves instead of 16 + 16 + 8 keys)
and with 128-slot chunks need a process of their own: tests/check_recall_child.py, one child at a time.
"""
import json
import os
import pickle
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

import dwpa_amd  # noqa: E402
from dwpa_amd import _lib as L  # noqa: E402
from dwpa_amd import m22000 as M  # noqa: E402
from tests import check_recall as C  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINGLE_STRIDE = 97  # every 97th job (a prime: all key positions and attempt residues) also goes through one call alone


def expected_kernels(p):
    """queue_verify's rule, restated: an EAPOL line with >= 64 attempts is verified attempt-parallel, keyver 1 and 2
    by the combined class (also when only one of them is in the call), keyver 3 by its own; a shorter list
    key-parallel by its keyver's class."""
    out = set()
    for (line, keys, pmk, nc), m in zip(p["jobs"], p["meta"]):
        natt = 1 + 4 * ((nc >> 1) + 1)
        if natt >= 64:
            out.add("k_verify_att<kv3>" if m[0] == 3 else "k_verify_att<kv1|kv2>")
        else:
            out.add("k_verify<kv%d>" % m[0])
    return out


def _plan(name):
    t = time.perf_counter()
    p = C.plan(name)
    dt = time.perf_counter() - t
    if dt > 0.05:
        print("%s: plan of %d jobs, %d slots built in %.2f s" % (name, len(p["jobs"]),
                                                                  sum(len(j[1]) for j in p["jobs"]), dt))
    return p


def _recall(p, singles=()):
    assert dwpa_amd.device_count() >= 1
    L.verify_kernels(reset=True)
    t = time.perf_counter()
    got, key_index = C.run_batch(p)
    dt = time.perf_counter() - t
    st = M.check_stats()
    print("%s: %d jobs, %d slots, %d PMKs, call %.3f s" % (p["name"], st["jobs"], st["slots"], st["pmks"], dt))
    assert st["backend"] == L.DWPA_BACKEND_DEVICE
    bad = C.mismatches(p, got, key_index)
    assert not bad, C.describe(p, bad)
    assert st["jobs"] == len(p["jobs"]) and st["slots"] == sum(len(j[1]) for j in p["jobs"])
    assert st["pmks"] == len(p["keys"])  # the (ESSID, key) dedup: K derives, gathered into K x jobs slots
    assert st["hits"] == sum(1 for e in p["exp"] if e)
    for i in singles:
        assert dwpa_amd.check_key_m22000(*p["jobs"][i]) == p["exp"][i], (p["name"], p["meta"][i])
        assert M.check_stats()["backend"] == L.DWPA_BACKEND_DEVICE
    assert L.verify_kernels() == expected_kernels(p)


@pytest.mark.parametrize("name", ["items_261", "items_65", "items_521"])
def test_attempt_parallel_finds_every_item(name):
    """Every attempt index of the window at every planned key position, keyver 1, 2 and 3 in one call (keyver 1 and
    2 share one launch of the combined kernel, keyver 3 has its own), the early exit on: segments of 16 + 16 + 8 keys
    (items_521: 16 + 4).  items_65: nearly every wave spans two keys.  items_521 adds the jobs that hand over the
    PMK of key 0.  Every SINGLE_STRIDE-th job, and every caller-PMK job, also runs through dwpa_check_m22000."""
    p = _plan(name)
    nc, nkeys, positions = C.ITEMS[name]
    extra = 9 if name == "items_521" else 0
    assert len(p["jobs"]) == 3 * len(positions) * C.ATTEMPTS[nc] + extra and C.ATTEMPTS[nc] >= 64
    singles = sorted(set(range(0, len(p["jobs"]), SINGLE_STRIDE)) | set(range(len(p["jobs"]) - extra, len(p["jobs"]))))
    _recall(p, singles)
    assert L.verify_kernels() == {"k_verify_att<kv1|kv2>", "k_verify_att<kv3>"}


@pytest.mark.parametrize("keyver", [1, 2])
@pytest.mark.parametrize("name", ["items_261", "items_65", "items_521"])
def test_attempt_parallel_one_keyver_alone(name, keyver):
    """Keyver 1 alone and keyver 2 alone: the combined keyver 1|2 kernel with lines of one kind only."""
    q = C.subset(_plan(name), (keyver,))
    assert len(q["jobs"]) >= len(C.ITEMS[name][2]) * C.ATTEMPTS[C.ITEMS[name][0]]
    _recall(q)
    assert L.verify_kernels() == {"k_verify_att<kv1|kv2>"}


def test_key_parallel_finds_every_item():
    """nc = 28, 61 attempts: the longest list under the 64-attempt switch, verified key-parallel from per-attempt KW
    blocks, at the same 40 positions x every attempt as items_65 on the other side of the switch.  (Key-parallel
    launches are one per keyver anyway, so there is no run of one keyver alone.)"""
    p = _plan("items_61")
    assert len(p["jobs"]) == 3 * 40 * 61
    _recall(p, range(0, len(p["jobs"]), SINGLE_STRIDE))
    assert L.verify_kernels() == {"k_verify<kv1>", "k_verify<kv2>", "k_verify<kv3>"}


def test_one_past_the_window_misses():
    """+-(halfnc + 1) in both endians, per keyver and verifier, and a line whose PSK the list does not hold: False."""
    p = _plan("misses")
    _recall(p, range(len(p["jobs"])))
    assert L.verify_kernels() == {"k_verify<kv1>", "k_verify<kv2>", "k_verify<kv3>", "k_verify_att<kv1|kv2>",
                                  "k_verify_att<kv3>"}


def test_carry_wrap_and_double_match_tails():
    """Stored nonce tails whose correction carries into the next byte, wraps 32 bits, or makes the LE and the BE
    attempt one value (two attempts of one key match: PHP's first, LE, is reported)."""
    p = _plan("tails")
    _recall(p, range(len(p["jobs"])))


def test_every_key_matches_twice():
    """300 copies of the PSK, every slot with two matching attempts: key_index 0 and the LE attempt."""
    p = _plan("double_full")
    assert len(p["jobs"][0][1]) == 300 and p["key_index"] == [0] and p["exp"][0][1:3] == [1, "LE"]
    _recall(p, [0])


# ---------------------------------------------------------------------------------------------------------------
# the early exit off, and small chunks: one child process each
# ---------------------------------------------------------------------------------------------------------------
def _child(tmp_path, names, batch, exit_on):
    fxp = tmp_path / "plans.pkl"
    with open(fxp, "wb") as f:
        pickle.dump({n: _plan(n) for n in names}, f)
    env = dict(os.environ, DWPA_FIRST_KEY_EXIT=exit_on)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "check_recall_child.py"), str(fxp), str(batch)]
                       + list(names), cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["exit"] == exit_on and res["batch"] == batch
    for n in names:
        o, p = res["plans"][n], C.plan(n)
        print(n, {k: o[k] for k in ("jobs", "records", "stats", "call_s")})
        assert o["nbad"] == 0, o["bad"]
        assert o["kernels"] == sorted(expected_kernels(p))
        assert o["stats"] == {"jobs": len(p["jobs"]), "slots": sum(len(j[1]) for j in p["jobs"]),
                              "pmks": len(p["keys"]) if batch == 0 else o["stats"]["pmks"],
                              "hits": sum(1 for e in p["exp"] if e), "backend": L.DWPA_BACKEND_DEVICE}
    return res["plans"]


@pytest.mark.parametrize("name", ["items_261", "items_65", "tails", "double_full"])
def test_early_exit_off_finds_every_item(tmp_path, name):
    """DWPA_FIRST_KEY_EXIT=0: a 40-key job is one segment of 163.1 waves (items_261), every key of a job is verified,
    and the host picks the first key and PHP's first attempt among all the hits.  double_full then reports two hit
    records per slot: 600 (dwpa_check_stats.hits counts the jobs with a hit, 1; the records are read from the
    library's dwpa_debug_check_hit_records hook)."""
    o = _child(tmp_path, [name], 0, "0")[name]
    if name == "double_full":
        assert o["records"] == 600 and o["stats"]["hits"] == 1
    else:  # every planted key reported at least once, twice where both endians match
        assert o["records"] >= o["stats"]["hits"]


def test_every_key_matches_twice_in_128_slot_chunks(tmp_path):
    """double_full with dwpa_init batch = 128 and the early exit off: chunks of 128 + 128 + 44 slots, the full ones
    filling 256 of their 2 x 128 + 64 hit records."""
    o = _child(tmp_path, ["double_full"], 128, "0")["double_full"]
    assert o["records"] == 600 and o["stats"]["hits"] == 1
