"""CPU: the gfx950 issue pass and its equivalence check with LDS instructions and waits in the loop body.

The work-queue PBKDF2 kernels keep cold words in LDS (pbkdf2_dev.hpp pbkdf2_lane_lds), so their 4096-iteration loop
holds ds_read_b32, no-return ds_xor_b32 and s_waitcnt lgkmcnt(N).  dwpa_amd/csrc/gen/issue_pass.py treats them as
fixed points: they keep their order among themselves, a read's consumers stay behind the wait that retires it, the
producers of an LDS operand stay in front of the instruction, and anything else unknown still stops the build.
tools/issue_equiv.py models LDS as a per-lane array and a read's destination as undefined until the wait.  The six
kernels that hold no LDS instruction must come out of the compiler and of the pass exactly as a build with the plain
lane (-DDWPA_QUEUE_LDS=0) gives them.
"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dwpa_amd", "csrc", "gen"))
import issue_pass as P  # noqa: E402
from tools import issue_equiv as E  # noqa: E402
from tools import kernel_asm as K  # noqa: E402

RULE = "sched=1:alt:orig:asmnop,before_half".split(",")
UNTOUCHED = ["k_pbkdf2_gfx950", "k_pbkdf2_gfx950_ms", "k_pbkdf2_gfx950_mg", "k_pbkdf2_gfx950_p",
             "k_pbkdf2_gfx950_ms_p", "k_pbkdf2_gfx950_mg_p"]
QUEUE = ["k_pbkdf2_gfx950_q", "k_pbkdf2_gfx950_mg_q"]


def _kernel(body):
    return ["k_test:", "\ts_mov_b32 s4, 4096", ".LBB0_1:                                ; =>This Inner Loop Header: Depth=1",
            *body, "\ts_add_i32 s4, s4, -1", "\ts_cmp_lg_u32 s4, 0", "\ts_cbranch_scc1 .LBB0_1", "\ts_endpgm", ""]


# v0 = the lane's LDS address.  Two reads, VALU work that does not need them, the wait, their consumers, the
# producers of the xor operands, the xors.
BODY = ["\tv_add_u32_e32 v1, v2, v3",
        "\tv_alignbit_b32 v4, v1, v1, 27",
        "\tds_read_b32 v10, v0 offset:5120",
        "\tds_read_b32 v11, v0 offset:6144",
        "\tv_xor_b32_e32 v5, v4, v2",
        "\tv_add3_u32 v6, v5, s8, v1",
        "\tv_alignbit_b32 v7, v6, v6, 2",
        "\ts_waitcnt lgkmcnt(0)",
        "\tv_add_u32_e32 v8, v10, v6",
        "\tv_add_u32_e32 v9, v11, v7",
        "\tv_xor_b32_e32 v2, v8, v9",
        "\tv_alignbit_b32 v3, v9, v9, 31",
        "\tds_xor_b32 v0, v8",
        "\tds_xor_b32 v0, v9 offset:1024",
        "\tv_add_u32_e32 v12, v8, v3"]


def _body_of(out):
    h, e, _ = P.main_loop_range(out, "k_test")
    return [l for l in out[h + 1:e] if l.strip() and l.strip() != "s_nop 0"]


def _is_fixed(l):
    return l.strip().startswith(("ds_", "s_waitcnt"))


def test_loop_with_lds_is_scheduled_and_keeps_the_fixed_points():
    out = P.nopify(_kernel(BODY), "k_test", RULE)
    new = _body_of(out)
    assert sorted(new) == sorted(BODY + ["\ts_add_i32 s4, s4, -1", "\ts_cmp_lg_u32 s4, 0"])  # nothing lost or added
    assert [l for l in new if _is_fixed(l)] == [l for l in BODY if _is_fixed(l)]  # same LDS ops, same order
    at = {l: i for i, l in enumerate(new)}
    wait = at["\ts_waitcnt lgkmcnt(0)"]
    # consumers of the reads behind the wait, the reads in front of it
    assert at["\tds_read_b32 v10, v0 offset:5120"] < wait < at["\tv_add_u32_e32 v8, v10, v6"]
    assert at["\tds_read_b32 v11, v0 offset:6144"] < wait < at["\tv_add_u32_e32 v9, v11, v7"]
    # producers of an xor's data in front of the xor
    assert at["\tv_add_u32_e32 v8, v10, v6"] < at["\tds_xor_b32 v0, v8"]
    assert at["\tv_add_u32_e32 v9, v11, v7"] < at["\tds_xor_b32 v0, v9 offset:1024"]
    # every VALU the compiler placed in front of a fixed point is still in front of it
    for k, l in enumerate(BODY):
        if _is_fixed(l):
            assert all(at[v] < at[l] for v in BODY[:k] if not _is_fixed(v)), l
    # the loop counter stays last, and the spacers still go in front of the 4-cycle ops
    assert new[-2:] == ["\ts_add_i32 s4, s4, -1", "\ts_cmp_lg_u32 s4, 0"]
    assert sum(1 for l in out if l.strip() == "s_nop 0") == sum(1 for l in BODY if "alignbit" in l or "add3" in l)


def test_scheduled_lds_loop_is_equivalent(tmp_path):
    src = tmp_path / "k.s"
    src.write_text("\n".join(_kernel(BODY)))
    ok, bad = E.check(str(src), "k_test", RULE, trials=3)
    assert ok, bad


@pytest.mark.parametrize("bad", [
    ["\tds_read_b64 v[10:11], v0"],                       # a register pair
    ["\tds_read2_b32 v[10:11], v0 offset1:1"],
    ["\tds_bpermute_b32 v10, v0, v1"],                    # crosses lanes
    ["\tds_xor_rtn_b32 v10, v0, v1"],                     # an atomic with return
    ["\tds_read_b32 v10, v0 gds"],                        # a modifier the pass does not know
    ["\ts_waitcnt vmcnt(0)"],                             # another counter
    ["\ts_waitcnt vmcnt(0) lgkmcnt(0)"],
    ["\tglobal_load_dword v10, v[0:1], off"],             # not LDS at all
    ["\tscratch_load_dword v10, off, off offset:4"],      # a spill
    ["\ts_barrier"],
    ["\tds_read_b32 v20, v0", "\tv_add_u32_e32 v9, v20, v1", "\ts_waitcnt lgkmcnt(0)"],  # used before the wait
    ["\tds_read_b32 v20, v0", "\tv_mov_b32_e32 v20, v1", "\ts_waitcnt lgkmcnt(0)"],      # overwritten in flight
    ["\tds_read_b32 v20, v0", "\tds_xor_b32 v0, v20", "\ts_waitcnt lgkmcnt(0)"],         # stored before it arrived
    ["\tds_read_b32 v20, v0"],                            # still outstanding at the loop's end
    ["\tds_read_b32 v20, v0", "\ts_waitcnt lgkmcnt(1)"],  # a wait that does not retire it
])
def test_unmodelled_lds_use_stops_the_pass(bad, tmp_path):
    P.nopify(_kernel(BODY), "k_test", RULE)  # the loop itself is fine
    lines = _kernel(BODY + bad)
    with pytest.raises(ValueError):
        P.nopify(lines, "k_test", RULE)
    src, dst = tmp_path / "in.s", tmp_path / "out.s"
    src.write_text("\n".join(lines))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "dwpa_amd", "csrc", "gen", "issue_pass.py"), str(src),
                        str(dst), "k_test", ",".join(RULE)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "refusing to schedule" in r.stderr
    assert not dst.exists()


def _differs(ref, new):
    init = {f"{c}{i}": (i * 2654435761 + (c == "s")) & 0xFFFFFFFF for c in "vs" for i in range(256)}
    l1, l2 = E.Lds(7), E.Lds(7)
    r1, r2 = E.run(ref, dict(init), l1), E.run(new, dict(init), l2)
    return (any(r1[k] != r2[k] or r2[k] is E.UNDEF for k in r1) or
            any(l1.get(a) != l2.get(a) or l2.get(a) is E.UNDEF for a in set(l1.mem) | set(l2.mem)))


def _swap(body, a, b):
    i, j = body.index(a), body.index(b)
    out = list(body)
    out[i], out[j] = out[j], out[i]
    return out


def test_the_checker_catches_misordered_lds_neighbours():
    assert not _differs(BODY, list(BODY))
    # a VALU that reads a register in front of the ds_read that redefines it, moved behind that read
    war = BODY[:2] + ["\tv_add_u32_e32 v13, v10, v1"] + BODY[2:]
    assert _differs(war, _swap(war, "\tv_add_u32_e32 v13, v10, v1", "\tds_read_b32 v10, v0 offset:5120"))
    # a read's consumer moved in front of the wait: the data has not arrived
    assert _differs(BODY, _swap(BODY, "\ts_waitcnt lgkmcnt(0)", "\tv_add_u32_e32 v8, v10, v6"))
    # the producer of an xor's data moved behind the xor: LDS gets the old value
    prod = BODY[:12] + ["\tv_add_u32_e32 v8, v8, v3"] + BODY[12:]
    assert _differs(prod, _swap(prod, "\tv_add_u32_e32 v8, v8, v3", "\tds_xor_b32 v0, v8"))
    # two xors to one word commute, a write and an xor to one word do not
    two = BODY + ["\tds_write_b32 v0, v12 offset:1024"]
    assert _differs(two, _swap(two, "\tds_xor_b32 v0, v9 offset:1024", "\tds_write_b32 v0, v12 offset:1024"))


# ------------------------------------------------------------------------------------------------------------------
# the product kernels: the six without LDS against a plain build, the two with it against the fit they must meet
# ------------------------------------------------------------------------------------------------------------------
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # the Makefile's


def _compile(dst, lds):
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only",
                    f"-DDWPA_QUEUE_LDS={lds}", "-S", os.path.join(ROOT, "dwpa_amd", "csrc", "pbkdf2_gfx950.hip"),
                    "-o", str(dst)], check=True, capture_output=True, timeout=300)
    return open(dst).read().split("\n")


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    """(LDS build, plain build) of pbkdf2_gfx950.hip as the compiler's assembly, compiled the way the Makefile does."""
    d = tmp_path_factory.mktemp("asm")
    built = os.path.join(ROOT, "build", "pbkdf2", "pbkdf2_gfx950.s")  # make's own, if no source is newer than it
    srcs = [os.path.join(ROOT, "dwpa_amd", "csrc", f) for f in ("pbkdf2_gfx950.hip", "pbkdf2_dev.hpp", "crypto_dev.hpp")]
    if os.path.exists(built) and all(os.path.getmtime(built) >= os.path.getmtime(s) for s in srcs):
        lds = open(built).read().split("\n")
        assert K.loop_ops(lds, QUEUE[0])["ds_xor_b32"] == 5, "the build has the LDS lane switched off"
    else:
        lds = _compile(d / "lds.s", 1)
    return lds, _compile(d / "plain.s", 0)


def test_kernels_without_lds_are_unchanged_against_a_plain_build(builds):
    lds, plain = builds
    for k in UNTOUCHED:
        assert K.kernel_text(lds, k) == K.kernel_text(plain, k), k
        assert not any(l.strip().startswith("ds_") for l in K.kernel_text(lds, k)), k
        assert K.resources(lds, k)["LDSByteSize"] == 0, k
    names = UNTOUCHED + QUEUE
    a, b = list(lds), list(plain)
    for k in names:  # the pass, kernel by kernel as the Makefile runs it
        a, b = P.nopify(a, k, RULE), P.nopify(b, k, RULE)
    for k in UNTOUCHED:
        assert K.kernel_text(a, k) == K.kernel_text(b, k), k
    for k in QUEUE:  # and the switch does switch: the plain build's queue kernels hold no LDS instruction
        assert K.loop_ops(a, k)["ds_xor_b32"] == 5 and "ds_xor_b32" not in K.loop_ops(b, k), k


@pytest.mark.parametrize("kernel", QUEUE)
def test_queue_kernels_fit_and_stay_equivalent(builds, kernel, tmp_path):
    lds, _ = builds
    out = P.nopify(list(lds), kernel, RULE)
    fits, report = K.gate(out, kernel)
    print(report)
    assert fits, report
    r = K.resources(out, kernel)
    assert r["NumVgprs"] <= 64 and r["ScratchSize"] == 0 and r["Occupancy"] == 8 and r["LDSByteSize"] <= 16384
    ops = K.loop_ops(out, kernel)
    assert ops["ds_xor_b32"] == 5 and ops["ds_read_b32"] == 8  # T, and four digest addends per compression
    src = tmp_path / "lds.s"
    src.write_text("\n".join(lds))
    ok, bad = E.check(str(src), kernel, RULE, trials=2)
    assert ok, bad


def test_makefile_gates_the_queue_kernels():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "build/pbkdf2/issue_equiv.ok build/pbkdf2/queue_lds_gate.ok" in mk
    assert "python3 tools/kernel_asm.py gate $< $(PBKDF2_QUEUE_KERNELS)" in mk
