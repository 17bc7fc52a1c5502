"""CPU: the check-path recall plans (tests/check_recall.py), reduced, through the library's host backend.

Every attempt index of the 261-, 65- and 61-attempt windows is planted at the first and the last position of a 6-key
list, for keyver 1, 2 and 3 and both nonce orders; then the stored-nonce tails whose corrections carry, wrap or make
the LE and the BE attempt one value, and a job of 20 copies of the PSK in which every key matches twice.  The host
backend verifies keyver 1/2 attempts four at a time (sha1_compress_x4): 261, 65 and 61 are all 1 mod 4, so its
remainder path and every place within a group of four get a plant.  Every result and key_index must equal the plan's,
which the C oracle decided.  This is also what proves the plan module sound without a device.
"""
import os

import pytest

import dwpa_amd
from dwpa_amd import _lib as L
from dwpa_amd import m22000 as M
from tests import check_recall as C


def _gpu_present():
    return os.path.exists("/dev/kfd") and os.environ.get("HIP_VISIBLE_DEVICES", "0") != ""


@pytest.fixture(autouse=True)
def _host_backend(monkeypatch):
    """Every call with a derive on the host backend, and the host backend for the rest when there is no device."""
    monkeypatch.setenv("DWPA_CPU_FALLBACK", "1")
    monkeypatch.setenv("DWPA_HOST_MAX_PMKS", "1000000000")
    yield


def _check(p, jobs_with_a_hit):
    got, key_index = C.run_batch(p)
    st = M.check_stats()
    assert st["backend"] in (L.DWPA_BACKEND_HOST_SMALL, L.DWPA_BACKEND_HOST_FALLBACK) or _gpu_present()
    bad = C.mismatches(p, got, key_index)
    assert not bad, C.describe(p, bad)
    assert st["jobs"] == len(p["jobs"]) and st["slots"] == sum(len(j[1]) for j in p["jobs"])
    assert st["hits"] == jobs_with_a_hit == sum(1 for e in p["exp"] if e)
    return got


@pytest.mark.parametrize("name", ["items_261_host", "items_65_host", "items_61_host"])
def test_every_attempt_index_is_found(name):
    p = C.plan(name)
    nc, nkeys, positions = C.ITEMS[name]
    assert len(p["jobs"]) == 3 * len(positions) * C.ATTEMPTS[nc] and all(len(j[1]) == nkeys == 6 for j in p["jobs"])
    _check(p, len(p["jobs"]))
    for i in range(0, len(p["jobs"]), 29):  # and singly, for a fixed stride
        assert dwpa_amd.check_key_m22000(*p["jobs"][i]) == p["exp"][i], p["meta"][i]
    one = C.subset(p, (2,))  # a call of one keyver
    _check(one, len(one["jobs"]))


def test_carry_wrap_and_double_match_tails():
    p = C.plan("tails")
    got = _check(p, 36)
    assert {tuple(g[1:3]) for g in got[:12]} == {(1, "LE"), (-1, "LE")}  # both endians match there: PHP's first


def test_one_past_the_window_misses():
    _check(C.plan("misses"), 0)


def test_every_key_matches_twice():
    p = C.plan("double_full_host")
    assert len(p["jobs"][0][1]) == 20 and len(set(p["jobs"][0][1])) == 1
    got = _check(p, 1)
    assert got[0][1:3] == [1, "LE"] and p["key_index"] == [0]
    assert dwpa_amd.check_key_m22000(*p["jobs"][0]) == p["exp"][0]
