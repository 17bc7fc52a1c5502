"""Child process of tests/test_gpu_check_recall.py: DWPA_FIRST_KEY_EXIT and the dwpa_init batch are fixed once per
process, so a run with the early exit off, or with the call cut into small chunks, gets a process of its own (started
fresh by the parent, with its environment plus the switch).

  check_recall_child.py PLANS.pkl BATCH NAME...

PLANS.pkl holds the parent's plans (tests/check_recall.py) by name; BATCH > 0 is passed to dwpa_init.  Prints one JSON
line: per plan the jobs that differ from the plan (count and description), the verify kernels that ran, the call's
stats and the hit records the device wrote."""
import ctypes
import json
import os
import pickle
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dwpa_amd import _lib as L  # noqa: E402
from dwpa_amd import m22000 as M  # noqa: E402
from tests import check_recall as C  # noqa: E402


def main():
    with open(sys.argv[1], "rb") as f:
        plans = pickle.load(f)
    batch = int(sys.argv[2])
    if batch:
        cfg = L.Config(ctypes.sizeof(L.Config), 0, batch, 0)
        L.check(L.load().dwpa_init(ctypes.byref(cfg)), "init")
    out = {"exit": os.environ.get("DWPA_FIRST_KEY_EXIT", "1"), "batch": batch, "plans": {}}
    for name in sys.argv[3:]:
        p = plans[name]
        L.verify_kernels(reset=True)
        L.check_hit_records(reset=True)
        t = time.perf_counter()
        got, key_index = C.run_batch(p)
        dt = time.perf_counter() - t
        st = M.check_stats()
        bad = C.mismatches(p, got, key_index)
        out["plans"][name] = {"jobs": len(p["jobs"]), "nbad": len(bad), "bad": repr(C.describe(p, bad)) if bad else "",
                              "kernels": sorted(L.verify_kernels()), "records": L.check_hit_records(),
                              "stats": {k: st[k] for k in ("jobs", "slots", "pmks", "hits", "backend")},
                              "call_s": round(dt, 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
