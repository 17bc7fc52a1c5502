#!/usr/bin/env python3
"""C4's shape through the mask path, beside the numeric path it generalises (GPU, one device).

One PMKID line, planted PSK 73019412, batch 16,777,216.  Three legs of equal step count, each in a child process of its
own under its own time limit -- the script stops at the first failure:

  1. numeric   load_numeric + run
  2. mask      set_mask ?d x 8 + load_mask + run
  3. numeric   again

Each leg reports PMK/s (candidates of the timed steps / their wall time, the hit read-back included), the load's device
time from dwpa_event_* around it, and its hits.  The numeric legs are code the mask attack does not change, so they
are the yardstick: the mask leg's PMK/s must lie within the spread of the two numeric legs of the same run, and the
three legs' hits must be equal.  Then one dwpa_crack_mask call over the 10^8 keyspace until the plant is found
(~73 % of it): rc, wall time, candidates.

  python3 tools/mask_bench.py [--steps 6] [--out profiles/mask/mask_bench.jsonl]

Every result is one JSON line on stdout and in --out; the last line is the verdict.  Exit status 0 = accepted.
"""
import argparse
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
KEYSPACE = 10**8
BATCH = 1 << 24
NC = 8


def the_line():
    from tests import synth as S
    rng = random.Random(3)
    essid, ap, sta, an, sn = S.random_net(rng, essid_len=8)
    return S.pmkid_line(b"%08d" % PLANT, essid, ap, sta), essid


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
    if kind == "mask":
        assert sc.set_mask("?d" * 8) == KEYSPACE
    nb = (KEYSPACE + BATCH - 1) // BATCH

    def step(i, e0=None, e1=None):
        first = (i % nb) * BATCH
        cnt = min(BATCH, KEYSPACE - first)
        if e0:
            L.check(lib.dwpa_event_record(e0, hs), "event_record")
        if kind == "mask":
            sc.load_mask(first, cnt, hs.value)
        else:
            sc.load_numeric(first, cnt, 8, hs.value)
        if e1:
            L.check(lib.dwpa_event_record(e1, hs), "event_record")
        sc.run(hs.value)
        return cnt, sc.hits(hs.value)

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
            "hits": [[h["line"], h["cand"], h["pmk"].hex()] for h in hits]}


def crack():
    import dwpa_amd
    from dwpa_amd import m22000 as M
    line, essid = the_line()
    with tempfile.TemporaryDirectory() as tmp:
        hf, out = os.path.join(tmp, "c4.hash"), os.path.join(tmp, "c4.key")
        with open(hf, "wb") as f:
            f.write(line + b"\n")
        t0 = time.perf_counter()
        rc = dwpa_amd.crack_mask(hf, "?d" * 8, nonce_error_corrections=NC, out_file=out, batch=BATCH)
        wall = time.perf_counter() - t0
        rec = open(out, "rb").read().decode("latin-1").strip() if os.path.exists(out) else ""
    st = M.crack_stats()
    return {"leg": "crack_mask", "rc": rc, "seconds": round(wall, 3), "candidates": st["candidates"], "words": st["words"],
            "cracked": st["cracked"], "pmk_per_s": round(st["candidates"] / wall, 1), "psk": rec.rsplit(":", 1)[-1],
            "workers": M.crack_worker_stats()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=6, help="timed steps per leg (6 = one pass over the keyspace)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask", "mask_bench.jsonl"))
    ap.add_argument("--child", choices=["numeric", "mask", "crack_mask"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(crack() if a.child == "crack_mask" else leg(a.child, a.steps, a.warmup)))
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
        limit = 60 + 14 * (a.steps + a.warmup)
        for kind in ("numeric", "mask", "numeric", "crack_mask"):
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--steps", str(a.steps),
                                    "--warmup", str(a.warmup)], capture_output=True, text=True,
                                   timeout=120 if kind == "crack_mask" else limit)
            except subprocess.TimeoutExpired:
                emit({"verdict": "failed", "why": kind + " leg ran into its time limit"})
                return 1
            if r.returncode != 0:
                emit({"verdict": "failed", "why": "%s leg exited with %d" % (kind, r.returncode),
                      "stderr": r.stderr[-1500:]})
                return 1
            emit(json.loads(r.stdout.strip().splitlines()[-1]))
        n1, m, n2, c = rows
        lo, hi = sorted((n1["pmk_per_s"], n2["pmk_per_s"]))
        line, essid = the_line()
        from tests import synth as S
        want = [[0, PLANT, S.pmk(b"%08d" % PLANT, essid).hex()]] * (a.steps // 6 + (a.steps % 6 > PLANT // BATCH))
        ok_hits = n1["hits"] == m["hits"] == n2["hits"] == want
        ok_rate = lo <= m["pmk_per_s"] <= hi
        ok_crack = c["rc"] == 0 and c["psk"] == "%08d" % PLANT and c["words"] == 0
        emit({"verdict": "accepted" if ok_hits and ok_rate and ok_crack else "refused",
              "numeric_pmk_per_s": [n1["pmk_per_s"], n2["pmk_per_s"]], "mask_pmk_per_s": m["pmk_per_s"],
              "mask_vs_numeric_mean": round(m["pmk_per_s"] / ((lo + hi) / 2), 5),
              "mask_within_numeric_spread": ok_rate, "hits_equal": ok_hits, "crack_mask_ok": ok_crack})
        return 0 if ok_hits and ok_rate and ok_crack else 1


if __name__ == "__main__":
    sys.exit(main())
