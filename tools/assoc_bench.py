#!/usr/bin/env python3
"""The association attack beside the only way to do its work without it (GPU, one device).

1,000 nets with distinct ESSIDs and MACs, one PMKID line each, 20 words per net and 100 rules: 2 x 10^6 (net, candidate)
pairs, every one inside 8..63 bytes, 50 of them planted (one net in twenty, at an index that moves through the words and
the rules).  Three legs, each in a child process of its own under its own time limit:

  1. check   dwpa_check_batch over the same pairs expanded on the host: one job per net with its 2,000 keys.  Code the
             association attack does not touch, and the only way to ask "these keys for that net" without it.
  2. assoc   set_assoc once, then load_assoc + run over the keyspace in batches of 2^20.
  3. check   again.

Then one dwpa_crack_assoc call over files of the same nets, words and rules.  Each leg reports PMK/s (pairs of the timed
passes / their wall time, the result read-back included; building the jobs, set_assoc and the upload of the entries are
timed apart) and its hits as (line, PSK, PMK) -- the assoc leg's PSK rebuilt from the hit's index on the host.

  python3 tools/assoc_bench.py [--passes 2] [--out profiles/assoc/assoc_bench.jsonl]

Every result is one JSON line on stdout and in --out; the last line is the verdict.  Exit status 0: the three legs
report the same hits, they are the plants, and the crack call found every plant.  PMK/s is reported, not judged.
--trace-leg KIND (check, assoc) runs one leg alone in this process: the form to put behind a kernel tracer.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NETS, WORDS, PLANTS = 1000, 20, 50
RULES = [":"] + ["$%s" % c for c in "0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"] + \
        ["^%s" % c for c in "0123456789abcdefghijklmnopqrstuvwxyzA"]
BATCH = 1 << 20
NC = 8
LEGS = ("check", "assoc", "check")
K = NETS * WORDS * len(RULES)


def word(n, w):
    return b"bench-%04d-%02d" % (n, w)


def apply(rule, w):
    return w if rule == ":" else w + rule[1:].encode() if rule[0] == "$" else rule[1:].encode() + w


def candidate(i):
    """(net, PSK) of index i: net-major, within a net rule-major with the word fastest."""
    n, sub = divmod(i, WORDS * len(RULES))
    r, w = divmod(sub, WORDS)
    return n, apply(RULES[r], word(n, w))


def plant_index(p):
    """Plant p stands in net 20 p + 7, at a word and a rule that move with p."""
    n = 20 * p + 7
    return n * WORDS * len(RULES) + (p * 37 % len(RULES)) * WORDS + p * 7 % WORDS


def fixture():
    from tests import synth as S
    assert len(RULES) == 100 and len(set(RULES)) == 100
    planted = dict(candidate(plant_index(p)) for p in range(PLANTS))
    nets, lines = [], []
    for n in range(NETS):
        essid, mac = b"bench-essid-%04d" % n, b"\x02\xbe" + n.to_bytes(4, "big")
        nets.append((essid, mac))
        lines.append(S.pmkid_line(planted.get(n, b"nobody-tries-%04d" % n), essid, mac, b"\x02\xc1" + n.to_bytes(4, "big")))
    want = sorted([n, planted[n].decode(), S.pmk(planted[n], nets[n][0]).hex()] for n in planted)
    return nets, lines, want


def leg_check(passes):
    from dwpa_amd import m22000 as M
    M.init(host_max_pmks=-1, allow_cpu_fallback=-1)
    nets, lines, _ = fixture()
    t0 = time.perf_counter()
    per = WORDS * len(RULES)
    jobs = M.BatchJobs((lines[n], [candidate(n * per + s)[1] for s in range(per)], False, NC) for n in range(NETS))
    build_s = time.perf_counter() - t0
    jobs.run()  # warm-up
    t0 = time.perf_counter()
    for _ in range(passes):
        jobs.run()
        res = jobs.results()
    wall = time.perf_counter() - t0
    hits = sorted([n, r[0].decode(), r[3].hex()] for n, r in enumerate(res) if r)
    return {"leg": "check", "passes": passes, "pairs": K * passes, "seconds": round(wall, 4),
            "pmk_per_s": round(K * passes / wall, 1), "build_jobs_s": round(build_s, 3), "stats": M.check_stats(),
            "hits": hits}


def leg_assoc(passes):
    import dwpa_amd
    from dwpa_amd import _lib as L
    from dwpa_amd import m22000 as M
    M.init(host_max_pmks=-1, allow_cpu_fallback=-1)
    nets, lines, _ = fixture()
    sc = dwpa_amd.Scan(lines, nc=NC, nc_mode=0, batch=BATCH)
    assert sc.nets == NETS
    t0 = time.perf_counter()
    k = sc.set_assoc([word(n, w) for n in range(NETS) for w in range(WORDS)],
                     [n for n in range(NETS) for _ in range(WORDS)], "\n".join(RULES))
    set_s = time.perf_counter() - t0
    assert k == K

    def one_pass():
        hits, loaded = [], 0
        for first in range(0, K, BATCH):
            sc.load_assoc(first, min(BATCH, K - first))
            sc.run()
            loaded += sc.loaded()
            hits += sc.hits()
        return hits, loaded

    one_pass()  # warm-up
    L.pbkdf2_kernels(reset=True)
    L.assoc_work(reset=True)
    t0 = time.perf_counter()
    for _ in range(passes):
        hits, loaded = one_pass()
    wall = time.perf_counter() - t0
    assert loaded == K
    out = sorted([h["line"], candidate(h["cand"])[1].decode(), h["pmk"].hex()] for h in hits)
    assert all(candidate(h["cand"])[0] == h["line"] for h in hits)  # one line per net, in net order
    sc.close()
    return {"leg": "assoc", "passes": passes, "pairs": K * passes, "seconds": round(wall, 4),
            "pmk_per_s": round(K * passes / wall, 1), "set_assoc_s": round(set_s, 3), "batch": BATCH,
            "kernels": sorted(L.pbkdf2_kernels()), "work": L.assoc_work(), "hits": out}


def crack():
    import dwpa_amd
    from dwpa_amd import m22000 as M
    nets, lines, want = fixture()
    with tempfile.TemporaryDirectory() as tmp:
        hf, af, rf, out = (os.path.join(tmp, n) for n in ("b.hash", "b.assoc", "b.rule", "b.key"))
        with open(hf, "wb") as f:
            f.write(b"\n".join(lines) + b"\n")
        with open(af, "wb") as f:
            f.write(b"".join(nets[n][1].hex().encode() + b":" + word(n, w) + b"\n" for n in range(NETS)
                             for w in range(WORDS)))
        with open(rf, "w") as f:
            f.write("".join(r + "\n" for r in RULES))
        t0 = time.perf_counter()
        rc = dwpa_amd.crack_assoc(hf, af, rules_file=rf, nonce_error_corrections=NC, out_file=out, batch=BATCH)
        wall = time.perf_counter() - t0
        recs = open(out, "rb").read().decode("latin-1").split("\n")[:-1] if os.path.exists(out) else []
    cs = M.crack_stats()
    return {"leg": "crack_assoc", "rc": rc, "seconds": round(wall, 3), "candidates": cs["candidates"],
            "words": cs["words"], "rules": cs["rules"], "cracked": cs["cracked"],
            "pmk_per_s": round(cs["candidates"] / wall, 1), "psks": sorted(r.rsplit(":", 1)[-1] for r in recs)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--passes", type=int, default=2, help="timed passes over the 2 x 10^6 pairs per leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assoc", "assoc_bench.jsonl"))
    ap.add_argument("--trace-leg", choices=["check", "assoc"], help="run this one leg alone in this process")
    ap.add_argument("--child", choices=["check", "assoc", "crack_assoc"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    kind = a.trace_leg or a.child
    if kind:
        print(json.dumps(leg_check(a.passes) if kind == "check" else leg_assoc(a.passes) if kind == "assoc" else crack()))
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

        # a pass is ~0.5 s at 4-5 M PMK/s; the fixture, the jobs' 2 x 10^6 key buffers and start-up take far longer
        limit = 120 + 10 * a.passes
        for kind in LEGS + ("crack_assoc",):
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--passes", str(a.passes)],
                                   capture_output=True, text=True, timeout=limit)
            except subprocess.TimeoutExpired:
                emit({"verdict": "failed", "why": kind + " ran into its time limit"})
                return 1
            if r.returncode != 0:
                emit({"verdict": "failed", "why": "%s exited with %d" % (kind, r.returncode), "stderr": r.stderr[-1500:]})
                return 1
            emit(json.loads(r.stdout.strip().splitlines()[-1]))
        c1, asc, c3, c = rows
        want = fixture()[2]
        ok_hits = c1["hits"] == asc["hits"] == c3["hits"] == want
        ok_crack = c["rc"] == 1 and c["cracked"] == PLANTS and c["psks"] == sorted(w[1] for w in want)
        lo = min(c1["pmk_per_s"], c3["pmk_per_s"])
        emit({"verdict": "accepted" if ok_hits and ok_crack else "refused",
              "check_pmk_per_s": [c1["pmk_per_s"], c3["pmk_per_s"]], "assoc_pmk_per_s": asc["pmk_per_s"],
              "assoc_vs_lower_check": round(asc["pmk_per_s"] / lo, 4), "crack_assoc_pmk_per_s": c["pmk_per_s"],
              "hits_equal": ok_hits, "crack_assoc_ok": ok_crack})
        return 0 if ok_hits and ok_crack else 1


if __name__ == "__main__":
    sys.exit(main())
