"""Per-kernel views of a gfx950 assembly file (the compiler's build/pbkdf2/pbkdf2_gfx950.s or the issue pass's
build/pbkdf2/pbkdf2_issue.s): one kernel's text, its resources, and what its main loop holds.

    python3 tools/kernel_asm.py text FILE KERNEL            the kernel's code, descriptor and resource comments
    python3 tools/kernel_asm.py same A.s B.s KERNEL[+...]   exit 1 unless every named kernel's text is equal in both
    python3 tools/kernel_asm.py gate FILE KERNEL[+...]      the fit of the LDS work-queue kernels:
                                                            <= 64 VGPRs, no scratch, 8 waves per SIMD, <= 16 KiB LDS,
                                                            exactly 5 LDS xors and no scratch access in the main loop;
                                                            prints one line per kernel, exit 1 if one does not fit
"""
import collections
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dwpa_amd", "csrc", "gen"))
import issue_pass as P  # noqa: E402

LDS_CEILING = 16384


def kernel_text(lines, kernel):
    """The lines of one kernel: from its label to the end of the resource comments after .Lfunc_end."""
    start = next(i for i, l in enumerate(lines) if l.startswith(kernel + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    end += 1
    while end < len(lines) and not lines[end].startswith(("\t.text", "\t.globl", "\t.protected", "\t.type")):
        end += 1
    return lines[start:end]


def resources(lines, kernel):
    """{NumVgprs, ScratchSize, Occupancy, LDSByteSize} from the compiler's comments after the kernel."""
    out = {}
    for l in kernel_text(lines, kernel):
        m = re.match(r"; (NumVgprs|ScratchSize|Occupancy|LDSByteSize): (\d+)", l)
        if m:
            out[m.group(1)] = int(m.group(2))
    return out


def loop_ops(lines, kernel):
    """Counter of the opcodes in the kernel's main loop (s_nop spacers included)."""
    h, e, _ = P.main_loop_range(lines, kernel)
    c = collections.Counter()
    for l in lines[h + 1:e]:
        m = re.match(r"\s+([a-z]\w+)", l)
        if m and not l.strip().startswith((";", ".")):
            c[m.group(1)] += 1
    return c


def gate(lines, kernel):
    """(fits, one-line report) of an LDS work-queue kernel."""
    r = resources(lines, kernel)
    ops = loop_ops(lines, kernel)
    valu = sum(n for o, n in ops.items() if o.startswith("v_"))
    xors = ops.get("ds_xor_b32", 0)
    reads = ops.get("ds_read_b32", 0)
    spill = sum(n for o, n in ops.items() if o.startswith(("scratch_", "buffer_", "flat_", "global_")))
    fits = (r["NumVgprs"] <= 64 and r["ScratchSize"] == 0 and r["Occupancy"] == 8 and
            0 < r["LDSByteSize"] <= LDS_CEILING and xors == 5 and spill == 0)
    return fits, (f"{kernel}: {r['NumVgprs']} VGPR, ScratchSize {r['ScratchSize']}, Occupancy {r['Occupancy']}, "
                  f"LDS {r['LDSByteSize']} B; main loop {valu} VALU, {xors} ds_xor_b32 (no return), {reads} "
                  f"ds_read_b32, {ops.get('s_waitcnt', 0)} s_waitcnt, {spill} memory ops: "
                  + ("fits" if fits else "DOES NOT FIT"))


def _read(path):
    return open(path).read().split("\n")


if __name__ == "__main__":
    cmd = sys.argv[1]
    if cmd == "text":
        print("\n".join(kernel_text(_read(sys.argv[2]), sys.argv[3])))
    elif cmd == "same":
        a, b = _read(sys.argv[2]), _read(sys.argv[3])
        bad = [k for k in sys.argv[4].split("+") if kernel_text(a, k) != kernel_text(b, k)]
        for k in sys.argv[4].split("+"):
            print(f"kernel_asm: {k}: " + ("DIFFERENT" if k in bad else "identical"))
        sys.exit(1 if bad else 0)
    elif cmd == "gate":
        src = _read(sys.argv[2])
        res = [gate(src, k) for k in sys.argv[3].split("+")]
        for _, line in res:
            print(line)
        sys.exit(0 if all(ok for ok, _ in res) else 1)
    else:
        sys.exit(__doc__)
