#!/usr/bin/env python3
"""C4's count and length through the combinator path, beside the numeric path (GPU, one device).

One PMKID line, planted PSK 73019412, a scan of 16,777,216 slots.  Both lists are the 10,000 words 0000..9999 in HBM:
10^8 candidates of 8 bytes, the set load_numeric's 8-digit keyspace holds.  Four legs of equal step count run one after
the other in one child process under one time limit:

  1. numeric      load_numeric + run
  2. combi_right  load_combinator(amp_side 0: base word + amplifier word) + run
  3. combi_left   the same with amp_side 1 (amplifier word + base word)
  4. numeric      again

A combinator load is whole base words x the whole amplifier, so a step holds 1,677 base words = 16,770,000 candidates
(the sixth step the remaining 1,615 words); the numeric legs load the same counts per step.  Each leg reports PMK/s
(candidates of the timed steps / their wall time, the hit read-back included), the load's device time from
dwpa_event_* around it, and its hits as (line, PSK rebuilt from the id, PMK).  The numeric legs are code the
combinator attack does not change, so they are the yardstick: their mean is the reference and their spread the
margin, and the four legs' hits must be equal.  The plant's id is base index * 10^4 + amplifier index: 7301 * 10^4 +
9412 with the amplifier right, 9412 * 10^4 + 7301 with the amplifier left (there the streamed word is the right half).
Then, in a second child, one dwpa_crack_combinator call (amplifier right, both lists as files) over the keyspace until
the plant is found (~73 % of it): rc, wall time, candidates.

  python3 tools/combi_bench.py [--steps 6] [--out profiles/combinator/combi_bench.jsonl]

Every result is one JSON line on stdout and in --out; the last line is the verdict.  Exit status 0: the hits are equal
and the crack call found the plant (whether a combinator leg lies inside the numeric spread is reported, not judged).
--trace-leg KIND runs one leg alone and prints its line: the form to put behind a kernel tracer.
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
NWORDS = 10**4
A = 10**4
BATCH = 1 << 24
WORDS_PER_STEP = BATCH // A
NC = 8
LEGS = ("numeric", "combi_right", "combi_left", "numeric")


def the_line():
    from tests import synth as S
    rng = random.Random(3)
    essid, ap, sta, an, sn = S.random_net(rng, essid_len=8)
    return S.pmkid_line(b"%08d" % PLANT, essid, ap, sta), essid


def the_words():
    return [b"%04d" % w for w in range(NWORDS)]


def psk_of(kind, cand):
    """The PSK a hit's id names: the decimal value (numeric, combi_right: base * A + amplifier index) or amplifier
    word || base word."""
    if kind == "combi_left":
        return "%04d%04d" % (cand % A, cand // A)
    return "%08d" % cand


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
    base = amp = None
    if kind != "numeric":
        base, amp = Dictionary.from_words(the_words()), Dictionary.from_words(the_words())
    side = {"combi_right": L.DWPA_COMBI_AMP_RIGHT, "combi_left": L.DWPA_COMBI_AMP_LEFT}.get(kind)
    nb = (NWORDS + WORDS_PER_STEP - 1) // WORDS_PER_STEP

    def step(i, e0=None, e1=None):
        w0 = (i % nb) * WORDS_PER_STEP
        nw = min(WORDS_PER_STEP, NWORDS - w0)
        if e0:
            L.check(lib.dwpa_event_record(e0, hs), "event_record")
        if kind == "numeric":
            sc.load_numeric(w0 * A, nw * A, 8, hs.value)
        else:
            sc.load_combinator(base.off.ptr, base.data.ptr, w0, nw, amp.off.ptr, amp.data.ptr, A, 0, A, side, 8, 63,
                               hs.value)
        if e1:
            L.check(lib.dwpa_event_record(e1, hs), "event_record")
        sc.run(hs.value)
        return nw * A, sc.hits(hs.value)

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
            "hits": [[h["line"], psk_of(kind, h["cand"]), h["pmk"].hex()] for h in hits]}


def crack():
    import dwpa_amd
    from dwpa_amd import m22000 as M
    line, essid = the_line()
    with tempfile.TemporaryDirectory() as tmp:
        hf, out = os.path.join(tmp, "c4.hash"), os.path.join(tmp, "c4.key")
        lf, rf = os.path.join(tmp, "left.txt"), os.path.join(tmp, "right.txt")
        with open(hf, "wb") as f:
            f.write(line + b"\n")
        for path in (lf, rf):
            with open(path, "wb") as f:
                f.write(b"".join(w + b"\n" for w in the_words()))
        t0 = time.perf_counter()
        rc, st = dwpa_amd.crack_combinator(hf, lf, rf, 0, nonce_error_corrections=NC, out_file=out, batch=BATCH)
        wall = time.perf_counter() - t0
        rec = open(out, "rb").read().decode("latin-1").strip() if os.path.exists(out) else ""
    cs = M.crack_stats()
    return {"leg": "crack_combinator", "rc": rc, "dict_status": st, "seconds": round(wall, 3),
            "candidates": cs["candidates"], "words": cs["words"], "cracked": cs["cracked"],
            "pmk_per_s": round(cs["candidates"] / wall, 1), "psk": rec.rsplit(":", 1)[-1],
            "workers": M.crack_worker_stats()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=6, help="timed steps per leg (6 = one pass over the keyspace)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "combinator", "combi_bench.jsonl"))
    ap.add_argument("--trace-leg", choices=["numeric", "combi_right", "combi_left"],
                    help="run this one leg alone in this process and print its line")
    ap.add_argument("--child", choices=["legs", "crack_combinator"], help=argparse.SUPPRESS)
    a = ap.parse_args()
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
        limit = 60 + 4 * 14 * (a.steps + a.warmup)
        for kind, n in (("legs", len(LEGS)), ("crack_combinator", 1)):
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--steps", str(a.steps),
                                    "--warmup", str(a.warmup)], capture_output=True, text=True,
                                   timeout=120 if kind == "crack_combinator" else limit)
            except subprocess.TimeoutExpired:
                emit({"verdict": "failed", "why": kind + " ran into its time limit"})
                return 1
            if r.returncode != 0:
                emit({"verdict": "failed", "why": "%s exited with %d" % (kind, r.returncode),
                      "stderr": r.stderr[-1500:]})
                return 1
            for ln in r.stdout.strip().splitlines()[-n:]:
                emit(json.loads(ln))
        n1, cr, cl, n2, c = rows
        lo, hi = sorted((n1["pmk_per_s"], n2["pmk_per_s"]))
        mean = (lo + hi) / 2
        line, essid = the_line()
        from tests import synth as S
        nb = (NWORDS + WORDS_PER_STEP - 1) // WORDS_PER_STEP
        times = a.steps // nb + (a.steps % nb > PLANT // (WORDS_PER_STEP * A))
        times_left = a.steps // nb + (a.steps % nb > (PLANT % A) // WORDS_PER_STEP)
        want = [0, "%08d" % PLANT, S.pmk(b"%08d" % PLANT, essid).hex()]
        ok_hits = n1["hits"] == cr["hits"] == n2["hits"] == [want] * times and cl["hits"] == [want] * times_left
        ok_ids = cr["ids"] == [PLANT] * times and cl["ids"] == [(PLANT % A) * A + PLANT // A] * times_left
        ok_crack = c["rc"] == 0 and c["psk"] == "%08d" % PLANT and c["words"] <= NWORDS
        ok = ok_hits and ok_ids and ok_crack
        emit({"verdict": "accepted" if ok else "refused", "numeric_pmk_per_s": [n1["pmk_per_s"], n2["pmk_per_s"]],
              "numeric_spread": round((hi - lo) / mean, 6),
              "combi_right_pmk_per_s": cr["pmk_per_s"], "combi_left_pmk_per_s": cl["pmk_per_s"],
              "combi_right_vs_numeric_mean": round(cr["pmk_per_s"] / mean, 5),
              "combi_left_vs_numeric_mean": round(cl["pmk_per_s"] / mean, 5),
              "combi_right_at_least_lower_numeric": cr["pmk_per_s"] >= lo,
              "combi_left_at_least_lower_numeric": cl["pmk_per_s"] >= lo,
              "hits_equal": ok_hits, "ids_exact": ok_ids, "crack_combinator_ok": ok_crack})
        return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
