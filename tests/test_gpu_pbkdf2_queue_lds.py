"""GPU: the work-queue PBKDF2 kernels with their cold words in LDS derive bit-exact PMKs.

k_pbkdf2_gfx950_q and k_pbkdf2_gfx950_mg_q keep T and the digest addends h0, h1, h3, h4 of both HMAC midstates in
LDS (pbkdf2_dev.hpp pbkdf2_lane_lds): a column per lane that a wave's successive items reuse, T accumulated with
no-return LDS xors.  What can go wrong there is per lane and per item -- a column shared by two lanes, a T that keeps
the previous item's words, a read-back ahead of the last xor, a lane past the last slot that writes -- so the scans
below are the smallest that reach every such case, and the sampled slots sit where the cases are.

A launch runs as a work queue only above 8 x level_lanes / 2 PMKs (pbkdf2_module.cpp use_prio; level_lanes = CUs x 4
SIMDs x 64, so 262,144 on 256 CUs), and one resident round is 8 x level_lanes / 64 waves / 2 output blocks = the same
number of slots.  So Q + 1 candidates (Q = that threshold) give 2 items more than there are resident waves: waves
take a second item, and the last item is a wave with one live lane.  Q + 64 * 3 + 1 gives a slot count that is no
multiple of 256 (the workgroup) with several second items.  Every numeric candidate at a sampled slot is the PSK of
one PMKID line; a hit carries the PMK the device derived (all 32 bytes: output block 1 is bytes 0..19, block 2 bytes
20..31), which must equal the CPU oracle's, and the hits must be exactly the planted ones.  The set of PBKDF2
kernels that ran (dwpa_debug_pbkdf2_kernels) proves which code derived them.
"""
import ctypes
import random

import pytest

pytestmark = pytest.mark.gpu

import dwpa_amd  # noqa: E402
from dwpa_amd import _lib as L  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import synth as S  # noqa: E402

DIGITS = 9
FIRST = 100_000_037
ESSID_1 = b"q"
ESSID_32 = bytes(0x41 + i % 26 for i in range(32))


def _cu_count():
    L.load()
    with open("/proc/self/maps") as f:
        path = next((ln.split()[-1] for ln in f if "libamdhip64.so" in ln), None)
    assert path, "the library maps no libamdhip64"
    hip = ctypes.CDLL(path)
    v = ctypes.c_int(0)
    assert hip.hipDeviceGetAttribute(ctypes.byref(v), 63, 0) == 0  # 63: hipDeviceAttributeMultiprocessorCount
    assert 1 <= v.value <= 4096, v.value
    return v.value


@pytest.fixture(scope="module")
def q_threshold():
    """The largest PMK count that does not run as a work queue: 2 * pmks <= 8 * level_lanes."""
    assert dwpa_amd.device_count() >= 1
    return 4 * _cu_count() * 4 * 64


def _sample(n, q):
    """Slots of an n-candidate scan (n > q): the first and the last slot, lanes 0, 63 and 64, both sides of a
    workgroup's end, the last slot of the resident round and the first slot of a wave's second item (slot q), the
    last full wave's ends, and a few seeded others."""
    last_full = (n // 64) * 64
    pos = {0, 1, 63, 64, 65, 127, 128, 255, 256, q - 64, q - 1, q, last_full - 64, last_full - 1, n - 1}
    if n - 1 > q:
        pos |= {q + 1, q + 63, q + 64, last_full}
    rng = random.Random(n)
    while len(pos) < 24:
        pos.add(rng.randrange(n))
    assert all(0 <= p < n for p in pos) and {0, 63, 64, q, n - 1} <= pos
    return sorted(pos)


_ref = {}


def _planted(essid, slots):
    """One PMKID line per slot, whose PSK is the numeric candidate of that slot; the oracle's PMKs, computed once."""
    key = (essid, tuple(slots))
    if key not in _ref:
        psks = [b"%0*d" % (DIGITS, FIRST + s) for s in slots]
        raw = O.c_pbkdf2_many(psks, essid, threads=8)
        rng = random.Random(len(essid))
        lines, pmks = [], []
        for i, psk in enumerate(psks):
            pmk = raw[32 * i:32 * i + 32]
            line = S.pmkid_line(psk, essid, rng.randbytes(6), rng.randbytes(6), the_pmk=pmk)
            assert O.c_check_key_m22000(line, [psk], pmk, 8) == [psk, None, None, pmk]
            lines.append(line)
            pmks.append(pmk)
        _ref[key] = (lines, pmks)
    return _ref[key]


def _scan(lines, n, per_group):
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(lines, nc=8, batch=n)
    try:
        sc.load_numeric(FIRST, n, DIGITS)
        assert sc.loaded() == n
        groups = sc.groups
        if per_group:
            for g in range(groups):
                sc.pbkdf2(g)
                sc.verify(g)
        else:
            sc.run()
        hits = sc.hits(cap=4096)
    finally:
        sc.close()
    got = [(h["line"], h["cand"], h["pmk"]) for h in hits]
    assert len(set(got)) == len(got), "a hit was reported twice"
    return groups, set(got), L.pbkdf2_kernels()


@pytest.mark.parametrize("extra", [1, 64 * 3 + 1])
@pytest.mark.parametrize("essid", [ESSID_1, ESSID_32], ids=["essid1", "essid32"])
def test_queue_kernel_pmks_are_bit_exact(q_threshold, essid, extra):
    """k_pbkdf2_gfx950_q (one ESSID per launch): ESSIDs of 1 and 32 bytes."""
    n = q_threshold + extra
    slots = _sample(n, q_threshold)
    lines, pmks = _planted(essid, slots)
    groups, got, ran = _scan(lines, n, per_group=True)
    assert groups == 1
    exp = {(k, FIRST + s, pmk) for k, (s, pmk) in enumerate(zip(slots, pmks))}
    assert got == exp, ("missing", sorted(exp - got)[:3], "extra", sorted(got - exp)[:3])
    assert ran == {"k_pbkdf2_gfx950_q"}, ran


@pytest.mark.parametrize("extra", [1, 64 * 3 + 1])
def test_group_queue_kernel_pmks_are_bit_exact(q_threshold, extra):
    """k_pbkdf2_gfx950_mg_q: the same candidates against two ESSID groups (1 and 32 bytes) in one launch; the
    second group's items start behind the first group's empty tail waves."""
    n = q_threshold + extra
    slots = _sample(n, q_threshold)
    lines, exp = [], set()
    for essid in (ESSID_1, ESSID_32):
        gl, gp = _planted(essid, slots)
        exp |= {(len(lines) + k, FIRST + s, pmk) for k, (s, pmk) in enumerate(zip(slots, gp))}
        lines += gl
    groups, got, ran = _scan(lines, n, per_group=False)
    assert groups == 2
    assert got == exp, ("missing", sorted(exp - got)[:3], "extra", sorted(got - exp)[:3])
    assert ran == {"k_pbkdf2_gfx950_mg_q"}, ran
