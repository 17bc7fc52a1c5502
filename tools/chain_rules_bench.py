#!/usr/bin/env python3
"""C4's count and length through a RULED chain, beside the numeric path (GPU, one device).  After tools/chain_bench.py,
whose line, plant, batch and legs it shares.

One PMKID line, planted PSK 73019412, a scan of 16,777,216 slots.  The ruled chain is list 00..99 under the 100 rules
$0$0 .. $9$9, then mask ?d?d?d?d: 10^8 candidates of 8 bytes, all kept -- the set load_numeric's 8-digit keyspace
holds, in another order: the ruled part is rule-major, so candidate i is word + rule digits + mask digits with
word = i // 10^4 % 100, rule = i // 10^6.  Three legs of equal step count run one after the other in one child process
under one time limit:

  1. numeric       load_numeric + run
  2. chain_rules   set_chain + set_chain_rules once, load_chain + run   (k_prep_chain_rules)
  3. numeric       again

and the three legs' hits must be equal as (line, PSK, PMK).  Then, recorded as a number only and with no pass mark, a
fourth leg whose LAST part is a ruled list of 3 words (list 00..99, mask ?d?d?d?d, words 0 1 2 under 33 one-byte
appends and prepends: 9.9 * 10^7 candidates of 8 bytes): a wave then holds some 22 distinct rules, which it runs one
after the other -- what rule divergence costs.  Then, in a second child, one dwpa_crack_chain_rules call (list and
rules as files) until the plant is found: rc, wall time, candidates.

  python3 tools/chain_rules_bench.py [--steps 6] [--out profiles/chain_rules/chain_rules_bench.jsonl]

Every result is one JSON line on stdout and in --out; the last line is the verdict.  --trace-leg KIND runs one leg
alone: the form to put behind a kernel tracer (`rocprofv3 --kernel-trace --stats -- python3 tools/chain_rules_bench.py
--trace-leg chain_rules --steps 1 --warmup 0`; no counters in that run).  --judge TRACE_DIR holds the ruled leg to
DESIGN.md 4.9's rule against the NUMERIC legs with the kernel times of TRACE_DIR/numeric_kernel_stats.csv and
TRACE_DIR/chain_rules_kernel_stats.csv, and appends its line to --out:

  chain_rules >= lower numeric leg x (1 - numeric spread - prep share),
  prep share = (k_prep_chain_rules time - k_prep_numeric time) / the step's PBKDF2 launch time.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import chain_bench as CB  # noqa: E402

PLANT, K, BATCH, NC = CB.PLANT, CB.K, CB.BATCH, CB.NC
LEGS = ("numeric", "chain_rules", "numeric")
RULES = ["$%d$%d" % (a, b) for a in range(10) for b in range(10)]
# the divergence leg: 3 words under 33 rules behind 10^6 choices
WORDS3 = [b"0", b"1", b"2"]
RULES3 = ["$%d" % d for d in range(10)] + ["^%d" % d for d in range(10)] + ["$" + chr(c) for c in range(97, 110)]
K3 = 100 * 10**4 * len(WORDS3) * len(RULES3)


def psk_of(i):
    """The PSK of raw index i of the ruled chain."""
    choice, mask = divmod(i, 10**4)
    rule, word = divmod(choice, 100)
    return "%02d%02d%04d" % (word, rule, mask)


def index_of(psk):
    return (int(psk[2:4]) * 100 + int(psk[:2])) * 10**4 + int(psk[4:])


def leg(kind, steps, warmup):
    import dwpa_amd
    from dwpa_amd import _lib as L
    from dwpa_amd import m22000 as M
    from dwpa_amd.device import Dictionary
    lib = L.load()
    M.init(host_max_pmks=-1, allow_cpu_fallback=-1)
    line, essid = CB.the_line()
    sc = dwpa_amd.Scan([line], nc=NC, nc_mode=0, batch=BATCH)
    hs = ctypes.c_void_p()
    L.check(lib.dwpa_stream_create(0, ctypes.byref(hs)), "stream_create")
    ev = []
    for _ in range(2 * steps):
        e = ctypes.c_void_p()
        L.check(lib.dwpa_event_create(0, ctypes.byref(e)), "event_create")
        ev.append(e)
    keep, k = [], K
    if kind == "chain_rules":
        d = Dictionary.from_words(CB.the_words())
        keep.append(d)
        assert sc.set_chain([(L.DWPA_CHAIN_LIST, d.off.ptr, d.data.ptr, 100), (L.DWPA_CHAIN_MASK, b"?d?d?d?d")]) == 10**6
        assert sc.set_chain_rules(0, "\n".join(RULES)) == K and sc.chain_nrules == 100
    elif kind == "chain_rules_3":
        d, d3 = Dictionary.from_words(CB.the_words()), Dictionary.from_words(WORDS3)
        keep += [d, d3]
        sc.set_chain([(L.DWPA_CHAIN_LIST, d.off.ptr, d.data.ptr, 100), (L.DWPA_CHAIN_MASK, b"?d?d?d?d"),
                      (L.DWPA_CHAIN_LIST, d3.off.ptr, d3.data.ptr, 3)])
        assert sc.set_chain_rules(2, "\n".join(RULES3)) == K3 and sc.chain_nrules == len(RULES3)
        k = K3
    nb = (k + BATCH - 1) // BATCH

    def step(i, e0=None, e1=None):
        first = (i % nb) * BATCH
        count = min(BATCH, k - first)
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
    name = (lambda i: "%08d" % i) if kind == "numeric" else psk_of if kind == "chain_rules" else str
    return {"leg": kind, "steps": steps, "warmup": warmup, "batch": BATCH, "candidates": cands, "seconds": round(wall, 4),
            "pmk_per_s": round(cands / wall, 1), "load_device_ms": load_ms, "kernels": sorted(L.pbkdf2_kernels()),
            "ids": [h["cand"] for h in hits], "hits": [[h["line"], name(h["cand"]), h["pmk"].hex()] for h in hits]}


def crack():
    import dwpa_amd
    from dwpa_amd import _lib as L
    from dwpa_amd import m22000 as M
    line, essid = CB.the_line()
    with tempfile.TemporaryDirectory() as tmp:
        hf, out, lf, rf = (os.path.join(tmp, n) for n in ("c4.hash", "c4.key", "list.txt", "append.rule"))
        with open(hf, "wb") as f:
            f.write(line + b"\n")
        with open(lf, "wb") as f:
            f.write(b"".join(w + b"\n" for w in CB.the_words()))
        with open(rf, "w") as f:
            f.write("\n".join(RULES) + "\n")
        parts = [(L.DWPA_CHAIN_LIST, lf), (L.DWPA_CHAIN_MASK, "?d?d?d?d")]
        t0 = time.perf_counter()
        rc, st = dwpa_amd.crack_chain(hf, parts, nonce_error_corrections=NC, out_file=out, batch=BATCH, rules=[rf, None])
        wall = time.perf_counter() - t0
        rec = open(out, "rb").read().decode("latin-1").strip() if os.path.exists(out) else ""
    cs = M.crack_stats()
    return {"leg": "crack_chain_rules", "rc": rc, "part_status": st, "seconds": round(wall, 3),
            "candidates": cs["candidates"], "words": cs["words"], "rules": cs["rules"], "cracked": cs["cracked"],
            "pmk_per_s": round(cs["candidates"] / wall, 1), "psk": rec.rsplit(":", 1)[-1],
            "workers": M.crack_worker_stats()}


def judge(out_path, trace_dir):
    rows = [json.loads(ln) for ln in open(out_path) if ln.strip()]
    legs = [r for r in rows if r.get("leg") in ("numeric", "chain_rules")]
    n1, ch, n2 = legs[:3]
    assert (n1["leg"], ch["leg"], n2["leg"]) == LEGS
    num, cha = (os.path.join(trace_dir, k + "_kernel_stats.csv") for k in ("numeric", "chain_rules"))
    prep_chain, prep_numeric = CB.kernel_ns(cha, "k_prep_chain_rules"), CB.kernel_ns(num, "k_prep_numeric")
    pbkdf2 = CB.kernel_ns(cha, "k_pbkdf2")
    lo, hi = sorted((n1["pmk_per_s"], n2["pmk_per_s"]))
    spread = (hi - lo) / ((lo + hi) / 2)
    share = (prep_chain - prep_numeric) / pbkdf2
    bound = lo * (1 - spread - share)
    row = {"rule": "chain_rules >= lower numeric x (1 - numeric spread - prep share)",
           "k_prep_chain_rules_ms": round(prep_chain / 1e6, 4), "k_prep_numeric_ms": round(prep_numeric / 1e6, 4),
           "pbkdf2_launch_ms": round(pbkdf2 / 1e6, 3), "prep_share": round(share, 6), "numeric_spread": round(spread, 6),
           "lower_numeric_pmk_per_s": lo, "bound_pmk_per_s": round(bound, 1), "chain_rules_pmk_per_s": ch["pmk_per_s"],
           "margin_pmk_per_s": round(ch["pmk_per_s"] - bound, 1), "rule_met": ch["pmk_per_s"] >= bound}
    three = os.path.join(trace_dir, "chain_rules_3_kernel_stats.csv")
    if os.path.exists(three):  # a number only
        row["k_prep_chain_rules_ms_3_words"] = round(CB.kernel_ns(three, "k_prep_chain_rules") / 1e6, 4)
    print(json.dumps(row))
    with open(out_path, "a") as f:
        f.write(json.dumps(row) + "\n")
    return 0 if row["rule_met"] else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=6, help="timed steps per leg (6 = one pass over the keyspace)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_rules", "chain_rules_bench.jsonl"))
    ap.add_argument("--trace-leg", choices=["numeric", "chain_rules", "chain_rules_3"],
                    help="run this one leg alone in this process and print its line")
    ap.add_argument("--judge", metavar="TRACE_DIR", help="hold the legs of --out to the rule with TRACE_DIR's kernel times")
    ap.add_argument("--child", choices=["legs", "crack_chain_rules"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.judge:
        return judge(a.out, a.judge)
    if a.trace_leg:
        print(json.dumps(leg(a.trace_leg, a.steps, a.warmup)))
        return 0
    if a.child == "legs":
        for kind in LEGS + ("chain_rules_3",):
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
        for kind, n in (("legs", len(LEGS) + 1), ("crack_chain_rules", 1)):
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--steps", str(a.steps),
                                    "--warmup", str(a.warmup)], capture_output=True, text=True,
                                   timeout=120 if kind == "crack_chain_rules" else limit)
            except subprocess.TimeoutExpired:
                emit({"verdict": "failed", "why": kind + " ran into its time limit"})
                return 1
            if r.returncode != 0:
                emit({"verdict": "failed", "why": "%s exited with %d" % (kind, r.returncode),
                      "stderr": r.stderr[-1500:]})
                return 1
            for ln in r.stdout.strip().splitlines()[-n:]:
                emit(json.loads(ln))
        n1, ch, n2, three, c = rows
        lo, hi = sorted((n1["pmk_per_s"], n2["pmk_per_s"]))
        mean = (lo + hi) / 2
        line, essid = CB.the_line()
        from tests import synth as S
        nb = (K + BATCH - 1) // BATCH
        times = a.steps // nb + (a.steps % nb > PLANT // BATCH)           # the numeric legs meet the plant at its value
        times_ch = a.steps // nb + (a.steps % nb > index_of("%08d" % PLANT) // BATCH)  # the chain at its index
        want = [0, "%08d" % PLANT, S.pmk(b"%08d" % PLANT, essid).hex()]
        ok_hits = n1["hits"] == n2["hits"] == [want] * times and ch["hits"] == [want] * times_ch
        ok_ids = ch["ids"] == [index_of("%08d" % PLANT)] * times_ch
        ok_crack = c["rc"] == 0 and c["psk"] == "%08d" % PLANT and c["words"] == 100 and c["rules"] == 100
        ok = ok_hits and ok_ids and ok_crack and times_ch > 0
        emit({"verdict": "accepted" if ok else "refused", "numeric_pmk_per_s": [n1["pmk_per_s"], n2["pmk_per_s"]],
              "numeric_spread": round((hi - lo) / mean, 6), "chain_rules_pmk_per_s": ch["pmk_per_s"],
              "chain_rules_vs_numeric_mean": round(ch["pmk_per_s"] / mean, 5),
              "chain_rules_at_least_lower_numeric": ch["pmk_per_s"] >= lo,
              "chain_rules_3_words_pmk_per_s": three["pmk_per_s"],
              "chain_rules_3_words_vs_numeric_mean": round(three["pmk_per_s"] / mean, 5),
              "hits_equal": ok_hits, "ids_exact": ok_ids, "crack_chain_rules_ok": ok_crack})
        return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
