#!/usr/bin/env python3
"""C4's count and length through the table attack, beside the numeric path (GPU, one device).

One PMKID line, planted PSK 73019412, a scan of 16,777,216 slots.  The table gives the byte `z` the ten digits as
alternatives; the list is the 10^4 words 0000zzzz .. 9999zzzz, each of 10^4 candidates: 10^8 candidates of 8 bytes, the
set load_numeric's 8-digit keyspace holds, and candidate id = its decimal value.  Three legs of equal step count run
one after the other in one child process under one time limit:

  1. numeric   load_numeric + run
  2. table     set_table once, load_table + run                 (k_table_count once, k_prep_table per load)
  3. numeric   again

A step is one batch of indices (the sixth step the remaining 16,113,920).  Each leg reports PMK/s (candidates of the
timed steps / their wall time, the hit read-back included), the load's device time from dwpa_event_* around it, and
its hits as (line, PSK, PMK), the table leg's PSK rebuilt from the hit's index on the host.  The numeric legs are code
the table attack does not change, so they are the yardstick, and the three legs' hits must be equal.  Then, in a second
child and as a number only, the index's other extreme: a list of 16,777,216 words of ONE candidate each (the 8-digit
numbers 67108864 .. 83886079, which hold the plant), so every wave spans 64 index entries; the same load six times.
Then, in a third child, one dwpa_crack_table call over the 10^8 keyspace until the plant is found.

  python3 tools/table_bench.py [--steps 6] [--out profiles/table/table_bench.jsonl]

Every result is one JSON line on stdout and in --out; the last line is the verdict.  Exit status 0: the hits are equal
and the crack call found the plant.  --trace-leg KIND (numeric, table, ones) runs one leg alone and prints its line: the
form to put behind a kernel tracer.  --judge TRACE_DIR holds the legs of --out to DESIGN.md 4.9's rule with the kernel
times of TRACE_DIR/numeric_kernel_stats.csv and TRACE_DIR/table_kernel_stats.csv (`rocprofv3 --kernel-trace --stats`,
one run per leg with no counters in it, one full load each) and appends its line to --out; the one-candidate list's
times are added to that line where TRACE_DIR has ones_kernel_stats.csv:

  table >= lower numeric leg x (1 - numeric spread - prep share),
  prep share = (k_prep_table time - k_prep_numeric time) / the step's PBKDF2 launch time.
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

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLANT = 73019412
K = 10**8
BATCH = 1 << 24
NC = 8
LEGS = ("numeric", "table", "numeric")
TABLE = b"".join(b"z=%d\n" % d for d in range(10))
ONES_FIRST = 4 * BATCH  # the batch of the numeric keyspace that holds the plant


def the_line():
    from tests import synth as S
    rng = random.Random(3)
    essid, ap, sta, an, sn = S.random_net(rng, essid_len=8)
    return S.pmkid_line(b"%08d" % PLANT, essid, ap, sta), essid


def digits(values, width):
    """values as zero-padded decimal text: a uint8 array of len(values) x width."""
    v = np.asarray(values, dtype=np.int64)[:, None]
    return ((v // 10 ** np.arange(width - 1, -1, -1, dtype=np.int64)) % 10 + 48).astype(np.uint8)


def the_list(kind):
    """(offsets, bytes) of the leg's list: 10^4 words NNNNzzzz, or 2^24 eight-digit numbers."""
    if kind == "ones":
        data = digits(np.arange(ONES_FIRST, ONES_FIRST + BATCH), 8)
    else:
        data = np.concatenate([digits(np.arange(10**4), 4), np.full((10**4, 4), ord("z"), dtype=np.uint8)], axis=1)
    return np.arange(len(data) + 1, dtype=np.uint64) * 8, data.reshape(-1)


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
    keyspace, set_s, dev = K, 0.0, None
    if kind != "numeric":
        off, data = the_list(kind)
        dev = Dictionary(off, data)
        t0 = time.perf_counter()
        keyspace, kept = sc.set_table(dev.off.ptr, dev.data.ptr, dev.n, TABLE)
        set_s = time.perf_counter() - t0
        assert (keyspace, kept) == ((K, 10**4) if kind == "table" else (BATCH, BATCH))
    nb = (keyspace + BATCH - 1) // BATCH

    def step(i, e0=None, e1=None):
        first = (i % nb) * BATCH
        count = min(BATCH, keyspace - first)
        if e0:
            L.check(lib.dwpa_event_record(e0, hs), "event_record")
        if kind == "numeric":
            sc.load_numeric(first, count, 8, hs.value)
        else:
            sc.load_table(first, count, hs.value)
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

    def psk(h):  # the table legs rebuild it from the index: the list is arithmetic, the library is not asked
        if kind == "table":
            return "%04d%04d" % divmod(h["cand"], 10**4)
        return "%08d" % (h["cand"] + (ONES_FIRST if kind == "ones" else 0))

    return {"leg": kind, "steps": steps, "warmup": warmup, "batch": BATCH, "candidates": cands, "seconds": round(wall, 4),
            "pmk_per_s": round(cands / wall, 1), "load_device_ms": load_ms, "set_table_s": round(set_s, 4),
            "kernels": sorted(L.pbkdf2_kernels()), "ids": [h["cand"] for h in hits],
            "hits": [[h["line"], psk(h), h["pmk"].hex()] for h in hits]}


def crack():
    import dwpa_amd
    from dwpa_amd import m22000 as M
    line, essid = the_line()
    with tempfile.TemporaryDirectory() as tmp:
        hf, out, lst, tab = (os.path.join(tmp, n) for n in ("c4.hash", "c4.key", "c4.list", "c4.table"))
        with open(hf, "wb") as f:
            f.write(line + b"\n")
        with open(lst, "wb") as f:
            f.write(b"".join(b"%04dzzzz\n" % n for n in range(10**4)))
        with open(tab, "wb") as f:
            f.write(TABLE)
        t0 = time.perf_counter()
        rc = dwpa_amd.crack_table(hf, lst, tab, nonce_error_corrections=NC, out_file=out, batch=BATCH)
        wall = time.perf_counter() - t0
        rec = open(out, "rb").read().decode("latin-1").strip() if os.path.exists(out) else ""
    cs = M.crack_stats()
    return {"leg": "crack_table", "rc": rc, "seconds": round(wall, 3), "candidates": cs["candidates"],
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
    legs = [r for r in rows if r.get("leg") in ("numeric", "table")]
    n1, tb, n2 = legs[:3]
    assert (n1["leg"], tb["leg"], n2["leg"]) == LEGS
    num, tab, one = (os.path.join(trace_dir, k + "_kernel_stats.csv") for k in ("numeric", "table", "ones"))
    prep_table, prep_numeric = kernel_ns(tab, "k_prep_table"), kernel_ns(num, "k_prep_numeric")
    pbkdf2 = kernel_ns(tab, "k_pbkdf2")
    lo, hi = sorted((n1["pmk_per_s"], n2["pmk_per_s"]))
    spread = (hi - lo) / ((lo + hi) / 2)
    share = (prep_table - prep_numeric) / pbkdf2
    bound = lo * (1 - spread - share)
    row = {"rule": "table >= lower numeric x (1 - numeric spread - prep share)",
           "k_prep_table_ms": round(prep_table / 1e6, 4), "k_prep_numeric_ms": round(prep_numeric / 1e6, 4),
           "k_table_count_ms": round(kernel_ns(tab, "k_table_count") / 1e6, 4),
           "pbkdf2_launch_ms": round(pbkdf2 / 1e6, 3), "prep_share": round(share, 6), "numeric_spread": round(spread, 6),
           "lower_numeric_pmk_per_s": lo, "bound_pmk_per_s": round(bound, 1), "table_pmk_per_s": tb["pmk_per_s"],
           "margin_pmk_per_s": round(tb["pmk_per_s"] - bound, 1), "rule_met": tb["pmk_per_s"] >= bound}
    if os.path.exists(one):
        row["k_prep_table_one_candidate_words_ms"] = round(kernel_ns(one, "k_prep_table") / 1e6, 4)
        row["k_table_count_16m_words_ms"] = round(kernel_ns(one, "k_table_count") / 1e6, 4)
    print(json.dumps(row))
    with open(out_path, "a") as f:
        f.write(json.dumps(row) + "\n")
    return 0 if row["rule_met"] else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=6, help="timed steps per leg (6 = one pass over the keyspace)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "table", "table_bench.jsonl"))
    ap.add_argument("--trace-leg", choices=["numeric", "table", "ones"],
                    help="run this one leg alone in this process and print its line")
    ap.add_argument("--judge", metavar="TRACE_DIR", help="hold the legs of --out to the rule with TRACE_DIR's kernel times")
    ap.add_argument("--child", choices=["legs", "ones", "crack_table"], help=argparse.SUPPRESS)
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
    if a.child == "ones":
        print(json.dumps(leg("ones", a.steps, a.warmup)))
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
        limit = 60 + 14 * (a.steps + a.warmup)
        for kind, n in (("legs", len(LEGS)), ("ones", 1), ("crack_table", 1)):
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--steps", str(a.steps),
                                    "--warmup", str(a.warmup)], capture_output=True, text=True,
                                   timeout=3 * limit if kind == "legs" else limit)
            except subprocess.TimeoutExpired:
                emit({"verdict": "failed", "why": kind + " ran into its time limit"})
                return 1
            if r.returncode != 0:
                emit({"verdict": "failed", "why": "%s exited with %d" % (kind, r.returncode),
                      "stderr": r.stderr[-1500:]})
                return 1
            for ln in r.stdout.strip().splitlines()[-n:]:
                emit(json.loads(ln))
        n1, tb, n2, ones, c = rows
        lo, hi = sorted((n1["pmk_per_s"], n2["pmk_per_s"]))
        mean = (lo + hi) / 2
        line, essid = the_line()
        from tests import synth as S
        nb = (K + BATCH - 1) // BATCH
        assert a.steps % nb == 0, "the legs' hits are compared over whole passes of the keyspace: --steps 6, 12, ..."
        want = [0, "%08d" % PLANT, S.pmk(b"%08d" % PLANT, essid).hex()]
        ok_hits = n1["hits"] == tb["hits"] == n2["hits"] == [want] * (a.steps // nb) and ones["hits"] == [want] * a.steps
        ok_crack = c["rc"] == 0 and c["psk"] == "%08d" % PLANT and c["words"] == 10**4
        ok = ok_hits and ok_crack
        emit({"verdict": "accepted" if ok else "refused", "numeric_pmk_per_s": [n1["pmk_per_s"], n2["pmk_per_s"]],
              "numeric_spread": round((hi - lo) / mean, 6), "table_pmk_per_s": tb["pmk_per_s"],
              "table_vs_numeric_mean": round(tb["pmk_per_s"] / mean, 5),
              "table_at_least_lower_numeric": tb["pmk_per_s"] >= lo,
              "one_candidate_words_pmk_per_s": ones["pmk_per_s"],
              "one_candidate_words_load_device_ms": ones["load_device_ms"],
              "hits_equal": ok_hits, "crack_table_ok": ok_crack})
        return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
