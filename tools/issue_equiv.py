"""Checks that the issue pass leaves a PBKDF2 loop body's results unchanged: both bodies run on the same random
register file, in a small interpreter of the loop's VALU ops. After one pass through the body every register must
match. That holds for the schedule (same instructions, dependences kept) and for the bank renaming (a renamed value
lives in a register the body writes again before reading it).

LDS (the work-queue kernels) is a per-lane array of words keyed by address value + offset, with the same random
contents for both bodies; after the body the arrays must match as well. LDS operations complete in order and only at a
wait: a ds_read_b32 leaves its destination UNDEFINED until an s_waitcnt lgkmcnt(N) retires it (all but the N youngest
operations), and an undefined value spreads through every VALU that reads it and into LDS. A consumer moved in front
of its read or of the wait, or a producer moved behind the LDS instruction that reads it, therefore shows up.

    python3 tools/issue_equiv.py build/pbkdf2/pbkdf2_gfx950.s KERNEL[+KERNEL...] RULES [trials]

`make` runs it on every kernel the pass schedules (build/pbkdf2/issue_equiv.ok): the library is not linked unless
the scheduled loops compute what the compiler's do.
"""
import random
import re
import sys
import os

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dwpa_amd", "csrc", "gen"))
import issue_pass as P  # noqa: E402

M = 0xFFFFFFFF


def _val(t, regs):
    if re.fullmatch(r"[vs]\d+", t):
        return regs[t]
    return int(t, 0) & M


UNDEF = None  # a register an LDS read has not delivered yet, and whatever is computed from it


class Lds:
    """One lane's LDS: words keyed by byte address, random (seeded) where nothing was written yet."""

    def __init__(self, seed):
        self.seed, self.mem = seed, {}

    def get(self, addr):
        if addr not in self.mem:
            self.mem[addr] = random.Random(f"{self.seed}:{addr}").getrandbits(32)
        return self.mem[addr]


def run(body, regs, lds=None):
    lds = lds if lds is not None else Lds(0)
    pending = []  # (destination, value) of LDS reads, (None, None) of xors / writes, oldest first

    def retire(keep):
        while len(pending) > keep:
            d, v = pending.pop(0)
            if d is not None:
                regs[d] = v

    for l in body:
        d = P.lds_op(l)
        if d:
            op, dst, addr, data, off = d
            a = regs[addr]
            key = UNDEF if a is UNDEF else (a + off) & M
            if key is UNDEF:
                raise ValueError(f"LDS address undefined: {l!r}")
            if op == "ds_read_b32":
                pending.append((dst, lds.get(key)))
                regs[dst] = UNDEF
            else:
                v = regs[data]
                old = lds.get(key)
                lds.mem[key] = UNDEF if v is UNDEF or old is UNDEF else (old ^ v if op == "ds_xor_b32" else v)
                pending.append((None, None))
            continue
        if re.match(r"\s+s_waitcnt\b", l):
            retire(P.lds_wait_count(l))
            continue
        m = re.match(r"\s+([vs]_\w+)\s*(.*)$", l)
        if not m:
            continue
        op = m.group(1)
        if op.startswith("s_"):
            continue  # the loop counter
        parts = [p.strip() for p in m.group(2).split(",")]
        mod = parts[-1].split()[1:] if len(parts[-1].split()) > 1 else []
        parts[-1] = parts[-1].split()[0]
        d, a = parts[0], [_val(t, regs) for t in parts[1:]]
        base = op.replace("_e32", "").replace("_e64", "")
        if any(x is UNDEF for x in a) or any(d == pd for pd, _ in pending):
            r = UNDEF  # reads a value not delivered yet, or writes a register a read in flight will overwrite
            if base not in ("v_add3_u32", "v_add_u32", "v_xor_b32", "v_alignbit_b32", "v_bitop3_b32", "v_mov_b32"):
                raise ValueError(f"op not modelled: {l!r}")
        elif base == "v_add3_u32":
            r = (a[0] + a[1] + a[2]) & M
        elif base == "v_add_u32":
            r = (a[0] + a[1]) & M
        elif base == "v_xor_b32":
            r = a[0] ^ a[1]
        elif base == "v_alignbit_b32":
            r = (((a[0] << 32) | a[1]) >> (a[2] & 31)) & M
        elif base == "v_bitop3_b32":
            tt = int(mod[0].split(":")[1], 0)
            r = 0
            for bit in range(32):
                x, y, z = (a[0] >> bit) & 1, (a[1] >> bit) & 1, (a[2] >> bit) & 1
                r |= ((tt >> (x * 4 + y * 2 + z)) & 1) << bit
        elif base == "v_mov_b32":
            r = a[0]
        else:
            raise ValueError(f"op not modelled: {l!r}")
        regs[d] = r
    retire(0)
    return regs


def check(path, kernel, rules, trials=3):
    lines = open(path).read().split("\n")
    h, e, _ = P.main_loop_range(lines, kernel)
    ref = lines[h + 1:e]
    out = P.nopify(lines, kernel, rules)
    h2, e2, _ = P.main_loop_range(out, kernel)
    new = out[h2 + 1:e2]
    for t in range(trials):
        rng = random.Random(t)
        init = {f"{c}{i}": rng.getrandbits(32) for c in "vs" for i in range(256)}
        l1, l2 = Lds(t), Lds(t)
        r1 = run(ref, dict(init), l1)
        r2 = run(new, dict(init), l2)
        keys = set(r1) | set(r2)
        bad = [k for k in keys if r1.get(k) != r2.get(k) or r2.get(k) is UNDEF]
        bad += [f"lds[{a:#x}]" for a in sorted(set(l1.mem) | set(l2.mem))
                if l1.get(a) != l2.get(a) or l2.get(a) is UNDEF]
        if bad:
            return False, bad
    return True, []


if __name__ == "__main__":
    # kernels "+"-separated (the Makefile checks every kernel the pass scheduled); exit 1 on any difference
    trials = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    failed = False
    for kern in sys.argv[2].split("+"):
        ok, bad = check(sys.argv[1], kern, sys.argv[3].split(","), trials)
        print(f"issue_equiv: {kern}: " + ("equal" if ok else f"DIFFERENT: {sorted(bad)[:10]}"))
        failed |= not ok
    sys.exit(1 if failed else 0)
