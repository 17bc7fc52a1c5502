#!/usr/bin/env python3
"""C4's count and length through the chain path, beside the numeric path (GPU, one device).

One PMKID line, planted PSK 73019412, a scan of 16,777,216 slots.  The chain is list 00..99 x the same list x mask
?d?d?d?d: 10^8 candidates of 8 bytes, the set load_numeric's 8-digit keyspace holds, in the same order -- candidate i
is the zero-padded decimal i, so a hit's id is the PSK's value on both paths.  Three legs of equal step count run one
after the other in one child process under one time limit:

  1. numeric   load_numeric + run
  2. chain     set_chain once, load_chain + run
  3. numeric   again

A step is one batch of raw indices (the sixth step the remaining 16,113,920); every candidate is kept, so the numeric
legs load the same counts.  Each leg reports PMK/s (candidates of the timed steps / their wall time, the hit read-back
included), the load's device time from dwpa_event_* around it, and its hits as (line, PSK, PMK).  The numeric legs are
code the chain attack does not change, so they are the yardstick, and the three legs' hits must be equal.  Then, in a
second child, one dwpa_crack_chain call (the list as a file, twice) over the keyspace until the plant is found (~73 %
of it): rc, wall time, candidates.

  python3 tools/chain_bench.py [--steps 6] [--out profiles/chain/chain_bench.jsonl]

Every result is one JSON line on stdout and in --out; the last line is the verdict.  Exit status 0: the hits are equal
and the crack call found the plant.  --trace-leg KIND runs one leg alone and prints its line: the form to put behind a
kernel tracer.  --judge TRACE_DIR holds the legs of --out to DESIGN.md 4.9's rule with the kernel times of
TRACE_DIR/numeric_kernel_stats.csv and TRACE_DIR/chain_kernel_stats.csv (`rocprofv3 --kernel-trace --stats`, one run
per leg, one full load each) and appends its line to --out:

  chain >= lower numeric leg x (1 - numeric spread - prep share),
  prep share = (k_prep_chain time - k_prep_numeric time) / the step's PBKDF2 launch time.
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
LEGS = ("numeric", "chain", "numeric")


def the_line():
    from tests import synth as S
    rng = random.Random(3)
    essid, ap, sta, an, sn = S.random_net(rng, essid_len=8)
    return S.pmkid_line(b"%08d" % PLANT, essid, ap, sta), essid


def the_words():
    return [b"%02d" % w for w in range(100)]


def leg(kind, steps, warmup):
    import dwpa_amd
    from dwpa_amd import _lib as L
    from dwpa_amd import m22000 as M
    from dwpa_amd.device import Dictionary
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
    d = None
    if kind == "chain":
        d = Dictionary.from_words(the_words())
        part = (L.DWPA_CHAIN_LIST, d.off.ptr, d.data.ptr, 100)
        assert sc.set_chain([part, part, (L.DWPA_CHAIN_MASK, b"?d?d?d?d")]) == K
    nb = (K + BATCH - 1) // BATCH

    def step(i, e0=None, e1=None):
        first = (i % nb) * BATCH
        count = min(BATCH, K - first)
        if e0:
            L.check(lib.dwpa_event_record(e0, hs), "event_record")
        if kind == "numeric":
            sc.load_numeric(first, count, 8, hs.value)
        else:
            sc.load_chain(first, count, 8, 63, hs.value)
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
    return {"leg": kind, "steps": steps, "warmup": warmup, "batch": BATCH, "candidates": cands, "seconds": round(wall, 4),
            "pmk_per_s": round(cands / wall, 1), "load_device_ms": load_ms, "kernels": sorted(L.pbkdf2_kernels()),
            "ids": [h["cand"] for h in hits],
            "hits": [[h["line"], "%08d" % h["cand"], h["pmk"].hex()] for h in hits]}


def crack():
    import dwpa_amd
    from dwpa_amd import _lib as L
    from dwpa_amd import m22000 as M
    line, essid = the_line()
    with tempfile.TemporaryDirectory() as tmp:
        hf, out, lf = os.path.join(tmp, "c4.hash"), os.path.join(tmp, "c4.key"), os.path.join(tmp, "list.txt")
        with open(hf, "wb") as f:
            f.write(line + b"\n")
        with open(lf, "wb") as f:
            f.write(b"".join(w + b"\n" for w in the_words()))
        parts = [(L.DWPA_CHAIN_LIST, lf), (L.DWPA_CHAIN_LIST, lf), (L.DWPA_CHAIN_MASK, "?d?d?d?d")]
        t0 = time.perf_counter()
        rc, st = dwpa_amd.crack_chain(hf, parts, nonce_error_corrections=NC, out_file=out, batch=BATCH)
        wall = time.perf_counter() - t0
        rec = open(out, "rb").read().decode("latin-1").strip() if os.path.exists(out) else ""
    cs = M.crack_stats()
    return {"leg": "crack_chain", "rc": rc, "part_status": st, "seconds": round(wall, 3),
            "candidates": cs["candidates"], "words": cs["words"], "cracked": cs["cracked"],
            "pmk_per_s": round(cs["candidates"] / wall, 1), "psk": rec.rsplit(":", 1)[-1],
            "workers": M.crack_worker_stats()}


def kernel_ns(path, stem):
    """Mean duration in ns of the kernel whose name holds `stem`, from a kernel_stats.csv."""
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if stem in row["Name"]:
                return float(row["AverageNs"])
    raise SystemExit("%s: no kernel named *%s*" % (path, stem))


def judge(out_path, trace_dir):
    rows = [json.loads(ln) for ln in open(out_path) if ln.strip()]
    legs = [r for r in rows if r.get("leg") in ("numeric", "chain")]
    n1, ch, n2 = legs[:3]
    assert (n1["leg"], ch["leg"], n2["leg"]) == LEGS
    num, cha = (os.path.join(trace_dir, k + "_kernel_stats.csv") for k in ("numeric", "chain"))
    prep_chain, prep_numeric = kernel_ns(cha, "k_prep_chain"), kernel_ns(num, "k_prep_numeric")
    pbkdf2 = kernel_ns(cha, "k_pbkdf2")
    lo, hi = sorted((n1["pmk_per_s"], n2["pmk_per_s"]))
    spread = (hi - lo) / ((lo + hi) / 2)
    share = (prep_chain - prep_numeric) / pbkdf2
    bound = lo * (1 - spread - share)
    row = {"rule": "chain >= lower numeric x (1 - numeric spread - prep share)",
           "k_prep_chain_ms": round(prep_chain / 1e6, 4), "k_prep_numeric_ms": round(prep_numeric / 1e6, 4),
           "pbkdf2_launch_ms": round(pbkdf2 / 1e6, 3), "prep_share": round(share, 6), "numeric_spread": round(spread, 6),
           "lower_numeric_pmk_per_s": lo, "bound_pmk_per_s": round(bound, 1), "chain_pmk_per_s": ch["pmk_per_s"],
           "margin_pmk_per_s": round(ch["pmk_per_s"] - bound, 1), "rule_met": ch["pmk_per_s"] >= bound}
    print(json.dumps(row))
    with open(out_path, "a") as f:
        f.write(json.dumps(row) + "\n")
    return 0 if row["rule_met"] else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=6, help="timed steps per leg (6 = one pass over the keyspace)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain", "chain_bench.jsonl"))
    ap.add_argument("--trace-leg", choices=["numeric", "chain"],
                    help="run this one leg alone in this process and print its line")
    ap.add_argument("--judge", metavar="TRACE_DIR", help="hold the legs of --out to the rule with TRACE_DIR's kernel times")
    ap.add_argument("--child", choices=["legs", "crack_chain"], help=argparse.SUPPRESS)
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
        for kind, n in (("legs", len(LEGS)), ("crack_chain", 1)):
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--steps", str(a.steps),
                                    "--warmup", str(a.warmup)], capture_output=True, text=True,
                                   timeout=120 if kind == "crack_chain" else limit)
            except subprocess.TimeoutExpired:
                emit({"verdict": "failed", "why": kind + " ran into its time limit"})
                return 1
            if r.returncode != 0:
                emit({"verdict": "failed", "why": "%s exited with %d" % (kind, r.returncode),
                      "stderr": r.stderr[-1500:]})
                return 1
            for ln in r.stdout.strip().splitlines()[-n:]:
                emit(json.loads(ln))
        n1, ch, n2, c = rows
        lo, hi = sorted((n1["pmk_per_s"], n2["pmk_per_s"]))
        mean = (lo + hi) / 2
        line, essid = the_line()
        from tests import synth as S
        nb = (K + BATCH - 1) // BATCH
        times = a.steps // nb + (a.steps % nb > PLANT // BATCH)
        want = [0, "%08d" % PLANT, S.pmk(b"%08d" % PLANT, essid).hex()]
        ok_hits = n1["hits"] == ch["hits"] == n2["hits"] == [want] * times
        ok_ids = ch["ids"] == [PLANT] * times
        ok_crack = c["rc"] == 0 and c["psk"] == "%08d" % PLANT and c["words"] == 200
        ok = ok_hits and ok_ids and ok_crack
        emit({"verdict": "accepted" if ok else "refused", "numeric_pmk_per_s": [n1["pmk_per_s"], n2["pmk_per_s"]],
              "numeric_spread": round((hi - lo) / mean, 6), "chain_pmk_per_s": ch["pmk_per_s"],
              "chain_vs_numeric_mean": round(ch["pmk_per_s"] / mean, 5),
              "chain_at_least_lower_numeric": ch["pmk_per_s"] >= lo,
              "hits_equal": ok_hits, "ids_exact": ok_ids, "crack_chain_ok": ok_crack})
        return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
