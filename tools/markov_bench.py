#!/usr/bin/env python3
"""C4's count and length through the Markov-ordered mask path, beside the numeric path (GPU, one device).

One PMKID line, planted PSK 73019412, a scan of 16,777,216 slots.  The mask is ?d x 8 under a model trained here from
a small seeded digit list, threshold 0: 10^8 candidates of 8 bytes, the set load_numeric's 8-digit keyspace holds, in
Markov order.  Three legs of equal step count run one after the other in one child process under one time limit:

  1. numeric   load_numeric + run
  2. markov    set_mask(markov=) once, load_mask + run          (k_prep_markov)
  3. numeric   again

A step is one batch of indices (the sixth step the remaining 16,113,920).  Each leg reports PMK/s (candidates of the
timed steps / their wall time, the hit read-back included), the load's device time from dwpa_event_* around it, and
its hits as (line, PSK, PMK), the Markov leg's PSK rebuilt from the hit's index on the host.  The numeric legs are
code the Markov attack does not change, so they are the yardstick, and the three legs' hits must be equal.  Then, in
a second child, one dwpa_crack_mask_markov call over the keyspace until the plant is found: rc, wall time, candidates.
Then, in a third child and as a number only, the dependent-load chain's worst case: a mask of 63 positions of ?l
under threshold 2 (K = 2^63, so one load fills), the load's device time over two steps.

  python3 tools/markov_bench.py [--steps 6] [--out profiles/markov/markov_bench.jsonl]

Every result is one JSON line on stdout and in --out; the last line is the verdict.  Exit status 0: the hits are equal
and the crack call found the plant.  --trace-leg KIND (numeric, mask, markov, markov63) runs one leg alone and prints
its line: the form to put behind a kernel tracer ("mask" is the plain ?d x 8 through k_prep_mask, for comparison).
--judge TRACE_DIR holds the legs of --out to DESIGN.md 4.9's rule with the kernel times of
TRACE_DIR/numeric_kernel_stats.csv and TRACE_DIR/markov_kernel_stats.csv (`rocprofv3 --kernel-trace --stats`, one run
per leg with no counters in it, one full load each) and appends its line to --out; k_prep_mask's and the 63-position
load's times are added to that line where TRACE_DIR has mask_kernel_stats.csv / markov63_kernel_stats.csv:

  markov >= lower numeric leg x (1 - numeric spread - prep share),
  prep share = (k_prep_markov time - k_prep_numeric time) / the step's PBKDF2 launch time.
"""
import argparse
import csv
import ctypes
import json
import os
import random
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLANT = 73019412
K = 10**8
BATCH = 1 << 24
NC = 8
LEGS = ("numeric", "markov", "numeric")
MASK = b"?d" * 8
LONG_MASK, LONG_T = b"?l" * 63, 2


def the_line():
    from tests import synth as S
    rng = random.Random(3)
    essid, ap, sta, an, sn = S.random_net(rng, essid_len=8)
    return S.pmkid_line(b"%08d" % PLANT, essid, ap, sta), essid


def the_model(tmp):
    """A model file trained from 20,000 seeded words: 8..10 digits, skewed towards low digits, and lowercase words of
    63 letters for the long mask's rows.  Returns its path."""
    from dwpa_amd import m22000 as M
    rng = random.Random(22000)
    words = [b"".join(b"%d" % min(9, int(rng.expovariate(0.4))) for _ in range(rng.randint(8, 10))) for _ in range(19000)]
    words += [bytes(rng.choice(b"etaoinshrdlucmfw") for _ in range(63)) for _ in range(1000)]
    lst, out = os.path.join(tmp, "digits.txt"), os.path.join(tmp, "digits.dwmk")
    with open(lst, "wb") as f:
        f.write(b"".join(w + b"\n" for w in words))
    assert M.markov_train([lst], out) == len(words)
    return out


def leg(kind, steps, warmup):
    import dwpa_amd
    from dwpa_amd import _lib as L
    from dwpa_amd import m22000 as M
    lib = L.load()
    M.init(host_max_pmks=-1, allow_cpu_fallback=-1)
    line, essid = the_line()
    sc = dwpa_amd.Scan([line], nc=NC, nc_mode=0, batch=BATCH)
    hs = ctypes.c_void_p()
    L.check(lib.dwpa_stream_create(0, ctypes.byref(hs)), "stream_create")
    ev = []
    for _ in range(2 * steps):
        e = ctypes.c_void_p()
        L.check(lib.dwpa_event_create(0, ctypes.byref(e)), "event_create")
        ev.append(e)
    model, keyspace, mask, t = None, K, MASK, 0
    with tempfile.TemporaryDirectory() as tmp:
        if kind in ("markov", "markov63"):
            model = M.markov_load(the_model(tmp))
    if kind == "markov63":
        mask, t = LONG_MASK, LONG_T
        keyspace = sc.set_mask(mask, markov=model, threshold=t)
        assert keyspace == 2**63
    elif kind == "markov":
        assert sc.set_mask(mask, markov=model) == K
    elif kind == "mask":
        assert sc.set_mask(mask) == K
    nb = (keyspace + BATCH - 1) // BATCH

    def step(i, e0=None, e1=None):
        first = (i % nb) * BATCH
        count = min(BATCH, keyspace - first)
        if e0:
            L.check(lib.dwpa_event_record(e0, hs), "event_record")
        if kind == "numeric":
            sc.load_numeric(first, count, 8, hs.value)
        else:
            sc.load_mask(first, count, hs.value)
        if e1:
            L.check(lib.dwpa_event_record(e1, hs), "event_record")
        sc.run(hs.value)
        return count, sc.hits(hs.value)

    for i in range(warmup):
        step(i)
    L.pbkdf2_kernels(reset=True)
    cands, hits = 0, []
    t0 = time.perf_counter()
    for i in range(steps):
        c, h = step(i, ev[2 * i], ev[2 * i + 1])
        cands += c
        hits += h
    wall = time.perf_counter() - t0
    load_ms = []
    for i in range(steps):
        ms = ctypes.c_float(0)
        L.check(lib.dwpa_event_elapsed_ms(ev[2 * i], ev[2 * i + 1], ctypes.byref(ms)), "event_elapsed")
        load_ms.append(round(ms.value, 4))
    for e in ev:
        lib.dwpa_event_destroy(e)
    sc.close()
    lib.dwpa_stream_destroy(hs)

    def psk(h):
        if model is not None:
            return M.mask_candidate(mask, h["cand"], markov=model, threshold=t).decode("latin-1")
        return "%08d" % h["cand"]

    return {"leg": kind, "steps": steps, "warmup": warmup, "batch": BATCH, "candidates": cands, "seconds": round(wall, 4),
            "pmk_per_s": round(cands / wall, 1), "load_device_ms": load_ms, "kernels": sorted(L.pbkdf2_kernels()),
            "ids": [h["cand"] for h in hits], "hits": [[h["line"], psk(h), h["pmk"].hex()] for h in hits]}


def crack():
    import dwpa_amd
    from dwpa_amd import m22000 as M
    line, essid = the_line()
    with tempfile.TemporaryDirectory() as tmp:
        hf, out = os.path.join(tmp, "c4.hash"), os.path.join(tmp, "c4.key")
        with open(hf, "wb") as f:
            f.write(line + b"\n")
        model = the_model(tmp)
        t0 = time.perf_counter()
        rc = dwpa_amd.crack_mask(hf, MASK, nonce_error_corrections=NC, out_file=out, batch=BATCH, markov=model)
        wall = time.perf_counter() - t0
        rec = open(out, "rb").read().decode("latin-1").strip() if os.path.exists(out) else ""
    cs = M.crack_stats()
    return {"leg": "crack_mask_markov", "rc": rc, "seconds": round(wall, 3), "candidates": cs["candidates"],
            "words": cs["words"], "cracked": cs["cracked"], "pmk_per_s": round(cs["candidates"] / wall, 1),
            "psk": rec.rsplit(":", 1)[-1], "workers": M.crack_worker_stats()}


def kernel_ns(path, stem):
    """Mean duration in ns of the kernel whose name holds `stem`, from a kernel_stats.csv."""
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if stem in row["Name"]:
                return float(row["AverageNs"])
    raise SystemExit("%s: no kernel named *%s*" % (path, stem))


def judge(out_path, trace_dir):
    rows = [json.loads(ln) for ln in open(out_path) if ln.strip()]
    legs = [r for r in rows if r.get("leg") in ("numeric", "markov")]
    n1, mk, n2 = legs[:3]
    assert (n1["leg"], mk["leg"], n2["leg"]) == LEGS
    num, mar, msk, m63 = (os.path.join(trace_dir, k + "_kernel_stats.csv") for k in ("numeric", "markov", "mask", "markov63"))
    prep_markov, prep_numeric = kernel_ns(mar, "k_prep_markov"), kernel_ns(num, "k_prep_numeric")
    pbkdf2 = kernel_ns(mar, "k_pbkdf2")
    lo, hi = sorted((n1["pmk_per_s"], n2["pmk_per_s"]))
    spread = (hi - lo) / ((lo + hi) / 2)
    share = (prep_markov - prep_numeric) / pbkdf2
    bound = lo * (1 - spread - share)
    row = {"rule": "markov >= lower numeric x (1 - numeric spread - prep share)",
           "k_prep_markov_ms": round(prep_markov / 1e6, 4), "k_prep_numeric_ms": round(prep_numeric / 1e6, 4),
           "pbkdf2_launch_ms": round(pbkdf2 / 1e6, 3), "prep_share": round(share, 6), "numeric_spread": round(spread, 6),
           "lower_numeric_pmk_per_s": lo, "bound_pmk_per_s": round(bound, 1), "markov_pmk_per_s": mk["pmk_per_s"],
           "margin_pmk_per_s": round(mk["pmk_per_s"] - bound, 1), "rule_met": mk["pmk_per_s"] >= bound}
    if os.path.exists(msk):
        row["k_prep_mask_ms"] = round(kernel_ns(msk, "k_prep_mask") / 1e6, 4)
    if os.path.exists(m63):
        row["k_prep_markov_63_positions_ms"] = round(kernel_ns(m63, "k_prep_markov") / 1e6, 4)
    print(json.dumps(row))
    with open(out_path, "a") as f:
        f.write(json.dumps(row) + "\n")
    return 0 if row["rule_met"] else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=6, help="timed steps per leg (6 = one pass over the keyspace)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "markov", "markov_bench.jsonl"))
    ap.add_argument("--trace-leg", choices=["numeric", "mask", "markov", "markov63"],
                    help="run this one leg alone in this process and print its line")
    ap.add_argument("--judge", metavar="TRACE_DIR", help="hold the legs of --out to the rule with TRACE_DIR's kernel times")
    ap.add_argument("--child", choices=["legs", "crack_mask_markov", "markov63"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.judge:
        return judge(a.out, a.judge)
    if a.trace_leg:
        print(json.dumps(leg(a.trace_leg, a.steps, a.warmup)))
        return 0
    if a.child == "legs":
        for kind in LEGS:
            print(json.dumps(leg(kind, a.steps, a.warmup)), flush=True)
        return 0
    if a.child == "markov63":
        print(json.dumps(leg("markov63", 2, 1)))
        return 0
    if a.child:
        print(json.dumps(crack()))
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    rows = []
    with open(a.out, "w") as out:
        def emit(row):
            rows.append(row)
            s = json.dumps(row)
            print(s, flush=True)
            out.write(s + "\n")
            out.flush()

        # one batch is ~3.3 s at C4's rate: the limit leaves a leg four times that, and start-up
        limit = 60 + 3 * 14 * (a.steps + a.warmup)
        for kind, n in (("legs", len(LEGS)), ("crack_mask_markov", 1), ("markov63", 1)):
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--steps", str(a.steps),
                                    "--warmup", str(a.warmup)], capture_output=True, text=True,
                                   timeout=limit if kind == "legs" else 120)
            except subprocess.TimeoutExpired:
                emit({"verdict": "failed", "why": kind + " ran into its time limit"})
                return 1
            if r.returncode != 0:
                emit({"verdict": "failed", "why": "%s exited with %d" % (kind, r.returncode),
                      "stderr": r.stderr[-1500:]})
                return 1
            for ln in r.stdout.strip().splitlines()[-n:]:
                emit(json.loads(ln))
        n1, mk, n2, c, long = rows
        lo, hi = sorted((n1["pmk_per_s"], n2["pmk_per_s"]))
        mean = (lo + hi) / 2
        line, essid = the_line()
        from tests import synth as S
        nb = (K + BATCH - 1) // BATCH
        assert a.steps % nb == 0, "the legs' hits are compared over whole passes of the keyspace: --steps 6, 12, ..."
        want = [0, "%08d" % PLANT, S.pmk(b"%08d" % PLANT, essid).hex()]
        ok_hits = n1["hits"] == mk["hits"] == n2["hits"] == [want] * (a.steps // nb)
        ok_crack = c["rc"] == 0 and c["psk"] == "%08d" % PLANT and c["words"] == 0
        ok = ok_hits and ok_crack
        emit({"verdict": "accepted" if ok else "refused", "numeric_pmk_per_s": [n1["pmk_per_s"], n2["pmk_per_s"]],
              "numeric_spread": round((hi - lo) / mean, 6), "markov_pmk_per_s": mk["pmk_per_s"],
              "markov_vs_numeric_mean": round(mk["pmk_per_s"] / mean, 5),
              "markov_at_least_lower_numeric": mk["pmk_per_s"] >= lo,
              "markov_63_positions_load_device_ms": long["load_device_ms"],
              "hits_equal": ok_hits, "crack_mask_markov_ok": ok_crack})
        return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
