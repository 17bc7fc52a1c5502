"""GPU precision: a target that is almost right must never be reported.

The recall tests pin "every true PSK is found" on every path; their lines are all genuine, so a verifier that compared
three of the four target words, 15 of 16 bytes or a word in the wrong byte order would pass them.  The fixtures of
tests/precision_plan.py put, next to each true line, the 128 lines that differ from it in one bit of the PMKID / MIC,
four with one target word byte-swapped, an over-long target that is right and one that is wrong in its 16th byte, and
lines made from the all-zero PMK, which every idle lane of the key-parallel verifier computes.  They go through every
comparison site of the device: the inline four-word compare of k_verify's PMKID branch and mic_match() in the
key-parallel classes (check path at nc 8, scan path per group and multi-group) and in the attempt-parallel classes
(check path at nc 128), and through the crack calls above them.  Expected results are the plan's model, which
tests/test_precision_plan.py ties to the C oracle line by line; the same file shows that a comparer blind to any one
bit, byte or word fails these comparisons.

Every test resets and then asserts the verify kernels that ran (dwpa_debug_verify_kernels), and the check-path tests
the hit records the device wrote (dwpa_debug_check_hit_records): the host's pick of the first key must not mask a
false record.  Each test prints its time (pytest -s shows it).
"""
import json
import os
import pickle
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

import dwpa_amd  # noqa: E402
from dwpa_amd import _lib as L  # noqa: E402
from dwpa_amd import m22000 as M  # noqa: E402
from dwpa_amd.device import Dictionary  # noqa: E402
from tests import check_recall as C  # noqa: E402
from tests import precision_plan as P  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = 192  # the smallest scan batch (a multiple of 64) of at least 192: three waves, the third with 2 of 64 lanes
KEY_PARALLEL = {"k_verify<pmkid>", "k_verify<kv1>", "k_verify<kv2>", "k_verify<kv3>"}
ATT_PARALLEL = {"k_verify<pmkid>", "k_verify_att<kv1|kv2>", "k_verify_att<kv3>"}


@pytest.fixture(autouse=True)
def _one_worker(monkeypatch):
    monkeypatch.delenv("DWPA_CRACK_SHARDS_PER_DEVICE", raising=False)
    monkeypatch.delenv("DWPA_FIRST_KEY_EXIT", raising=False)


@pytest.fixture(scope="module")
def dictionary():
    assert dwpa_amd.device_count() >= 1
    return Dictionary.from_words(P.dictionary())


# ---------------------------------------------------------------------------------------------------------------
# a, b, c: the check path
# ---------------------------------------------------------------------------------------------------------------
def _check(p, kernels):
    """One dwpa_check_batch over the plan's jobs on the device: results and key_index equal the plan, the kernels are
    `kernels`, and the device wrote one hit record per expected hit -- none for a near-miss."""
    L.verify_kernels(reset=True)
    L.check_hit_records(reset=True)
    t = time.perf_counter()
    got, key_index = C.run_batch(p)
    dt = time.perf_counter() - t
    st = M.check_stats()
    ran, records = L.verify_kernels(), L.check_hit_records()
    nhit = sum(1 for e in p["exp"] if e)
    print("%s: %d jobs, %d hits, %d hit records, %s, call %.3f s" % (p["name"], len(p["jobs"]), st["hits"], records,
                                                                      sorted(ran), dt))
    assert st["backend"] == L.DWPA_BACKEND_DEVICE
    bad = C.mismatches(p, got, key_index)
    assert not bad, C.describe(p, bad)
    assert st["jobs"] == len(p["jobs"]) and st["hits"] == nhit
    assert ran == kernels
    assert records == nhit


def test_check_path_key_parallel():
    """a. nc = 8, 21 attempts: k_verify of the four classes over every line of the fixture, derived and caller PMKs."""
    p = P.check_plan(P.fixture("single"))
    assert len(p["jobs"]) == 593 and sum(1 for e in p["exp"] if e) == 57
    _check(p, KEY_PARALLEL)


def test_check_path_attempt_parallel():
    """b. nc = 128, 261 attempts, the true correction at +-30 / +-65: the EAPOL lines go to k_verify_att (keyver 1 and
    2 in the combined class, keyver 3 in its own), the PMKID lines stay key-parallel.  The early exit is on."""
    p = P.check_plan(P.fixture("wide"))
    assert len(p["jobs"]) == 593
    _check(p, ATT_PARALLEL)


@pytest.mark.parametrize("keyver", [1, 2])
def test_check_path_attempt_parallel_one_keyver(keyver):
    """b. The combined keyver 1|2 class with lines of one key version only."""
    p = P.check_plan(P.fixture("wide"), kinds=(keyver,))
    assert len(p["jobs"]) == 16 + 128 + 4 + 3 + 1
    _check(p, {"k_verify_att<kv1|kv2>"})


def test_check_path_attempt_parallel_early_exit_off(tmp_path):
    """b. DWPA_FIRST_KEY_EXIT=0 (read once per process: a child, tests/check_recall_child.py): every key of a job is
    verified and the host picks among all the records.  Still one record per expected hit."""
    p = P.check_plan(P.fixture("wide"))
    name = p["name"]
    fxp = tmp_path / "plans.pkl"
    with open(fxp, "wb") as f:
        pickle.dump({name: p}, f)
    env = dict(os.environ, DWPA_FIRST_KEY_EXIT="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "check_recall_child.py"), str(fxp), "0", name],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    o = res["plans"][name]
    print(name, "early exit off", {k: o[k] for k in ("jobs", "records", "kernels", "stats", "call_s")})
    assert res["exit"] == "0" and o["jobs"] == len(p["jobs"])
    assert o["nbad"] == 0, o["bad"]
    nhit = sum(1 for e in p["exp"] if e)
    assert o["kernels"] == sorted(ATT_PARALLEL)
    assert o["stats"]["backend"] == L.DWPA_BACKEND_DEVICE and o["stats"]["hits"] == nhit
    assert o["records"] == nhit


@pytest.mark.host_routing
@pytest.mark.parametrize("name", ["single", "wide"])
def test_host_equals_device(name):
    """c. The same jobs once with every derive on the host backend and once with the host backend off: both lists
    equal the plan."""
    fx = P.fixture(name)
    js = P.jobs(fx)
    exp, _ = P.job_results(fx, js)
    L.verify_kernels(reset=True)
    try:
        M.init(host_max_pmks=1 << 30)
        host = dwpa_amd.check_batch(js)
        assert M.check_stats()["backend"] == L.DWPA_BACKEND_HOST_SMALL
        assert L.verify_kernels() == set()
        M.init(host_max_pmks=-1)
        dev = dwpa_amd.check_batch(js)
        assert M.check_stats()["backend"] == L.DWPA_BACKEND_DEVICE
    finally:
        M.init()
    bad = [i for i, (h, e) in enumerate(zip(host, exp)) if h != e]
    assert not bad, ("host", P.describe(fx, bad[:5]))
    bad = [i for i, (d, e) in enumerate(zip(dev, exp)) if d != e]
    assert not bad, ("device", P.describe(fx, bad[:5]))
    assert L.verify_kernels() == (KEY_PARALLEL if name == "single" else ATT_PARALLEL)


# ---------------------------------------------------------------------------------------------------------------
# d, e, f: the scan path
# ---------------------------------------------------------------------------------------------------------------
def _hitset(hits):
    got = [(h["line"], h["cand"], h["nc"], h["endian"], h["pmk"]) for h in hits]
    assert len(set(got)) == len(got), "a hit was reported twice"
    return set(got)


def _describe_hits(fx, rows, got, exp):
    def show(h):
        r = fx["rows"][rows[h[0]]]
        return (r["kind"], r["tag"], r["plant"], r["frame"]) + h[1:4]
    missing, extra = sorted(exp - got), sorted(got - exp)
    return ("missing %d" % len(missing), [show(h) for h in missing[:5]], "extra %d" % len(extra),
            [show(h) for h in extra[:5]])


def _scan(fx, rows, d, nc_mode, mode, loads=(P.NWORDS,)):
    """One Scan of the lines of `rows`: per load of the dictionary's first n words, the hits are exactly the plan's."""
    lines = [fx["rows"][i]["line"] for i in rows]
    t = time.perf_counter()
    L.verify_kernels(reset=True)
    sc = dwpa_amd.Scan(lines, nc=8, nc_mode=nc_mode, batch=BATCH)
    try:
        assert sc.batch == BATCH and sc.groups == len(fx["essids"])
        assert all(sc.line_status(i) >= 0 for i in range(len(lines)))
        for n in loads:
            sc.load_dict(d.off.ptr, d.data.ptr, 0, n)
            assert sc.loaded() == n
            if mode == "run":
                sc.run()
            else:
                for g in range(sc.groups):
                    sc.pbkdf2(g)
                    sc.verify(g)
            got, exp = _hitset(sc.hits(cap=4096)), P.scan_hits(fx, rows, n)
            assert got == exp, (mode, nc_mode, n) + _describe_hits(fx, rows, got, exp)
    finally:
        sc.close()
    ran = L.verify_kernels()
    print("scan %s %s mode %d: %d lines, loads %s, %s: %.3f s" % (fx["name"], mode, nc_mode, len(lines), loads,
                                                                  sorted(ran), time.perf_counter() - t))
    return ran


@pytest.mark.parametrize("nc_mode", [L.DWPA_NC_PHP, L.DWPA_NC_HASHCAT])
def test_scan_one_group(dictionary, nc_mode):
    """d. Every line of the one-ESSID fixture in one Scan, the 130 words in a batch of 192 (the PSK in lanes 0 and 63
    of the first wave, lane 0 of the second and lane 1 of the third, 62 lanes of which are idle), pbkdf2(0) and
    verify(0): the hits are the controls and long-target hits x the four copies, with the oracle's (nc, endian, pmk),
    in PHP's and in hashcat's attempt order."""
    fx = P.fixture("single")
    assert len(P.scan_hits(fx)) == 4 * 57
    assert _scan(fx, range(len(fx["rows"])), dictionary, nc_mode, "per_group") == KEY_PARALLEL


@pytest.mark.parametrize("nc_mode", [L.DWPA_NC_PHP, L.DWPA_NC_HASHCAT])
def test_scan_multi_group(dictionary, nc_mode):
    """e. The same families spread over the 1-, 13- and 52-byte ESSIDs through run(): the line_list / line_poff launch
    of one k_verify per class."""
    fx = P.fixture("multi")
    assert fx["essids"] == P.ESSIDS_MULTI and [len(e) for e in fx["essids"]] == [1, 13, 52]
    assert _scan(fx, range(len(fx["rows"])), dictionary, nc_mode, "run") == KEY_PARALLEL


@pytest.mark.parametrize("mode", ["per_group", "run"])
def test_idle_lanes_and_the_zero_pmk(dictionary, mode):
    """f. Loads of 1, 65 and 130 words leave 63, 63 and 62 idle lanes in the last wave; each of them computes the
    PMKID / MIC of the all-zero PMK.  The twelve zero-PMK lines (four kinds x three ESSIDs) are never reported, per
    group and through run(); the controls beside them are, once per copy of the PSK loaded."""
    fx = P.fixture("multi")
    rows = [i for i, r in enumerate(fx["rows"]) if r["tag"] in ("control", "zero")]
    assert sum(1 for i in rows if fx["rows"][i]["tag"] == "zero") == 12
    assert _scan(fx, rows, dictionary, L.DWPA_NC_PHP, mode, loads=(1, 65, 130)) == KEY_PARALLEL


def test_zero_pmk_lines_are_hits_with_the_zero_pmk():
    """f, the positive control: the same zero-PMK lines through the check path with the zero PMK handed over (the
    goldens' zero-pmk-* shape) are hits -- the lines are sound, the scans above did not miss them for another
    reason."""
    fx = P.fixture("multi")
    js, exp = P.zero_jobs(fx)
    assert len(js) == 12
    L.verify_kernels(reset=True)
    L.check_hit_records(reset=True)
    assert dwpa_amd.check_batch(js) == exp
    assert M.check_stats()["backend"] == L.DWPA_BACKEND_DEVICE
    assert L.verify_kernels() == KEY_PARALLEL and L.check_hit_records() == 12


# ---------------------------------------------------------------------------------------------------------------
# g: through a crack call
# ---------------------------------------------------------------------------------------------------------------
def _crack(tmp_path, fx, call):
    hf, out = tmp_path / "h.hash", tmp_path / "o.key"
    hf.write_bytes(b"\n".join(fx["lines"]) + b"\n")
    L.verify_kernels(reset=True)
    t = time.perf_counter()
    rc = call(str(hf), str(out))
    dt = time.perf_counter() - t
    ran, st = L.verify_kernels(), M.crack_stats()
    recs = out.read_bytes().split(b"\n") if out.exists() else [b""]
    assert recs.pop() == b""
    exp = P.records(fx)
    print("crack %s: rc %d, %d records, %s, %s: %.3f s" % (fx["name"], rc, len(recs), st, sorted(ran), dt))
    missing, extra = sorted(set(exp) - set(recs)), sorted(set(recs) - set(exp))
    assert not missing and not extra, ("missing %d" % len(missing), missing[:3], "extra %d" % len(extra), extra[:3])
    assert sorted(recs) == exp  # one record per hit line (the hit lines of one frame share a record's text)
    assert rc == 1  # exhausted: the near-misses and the zero lines stay
    assert st["hashes"] == len(fx["lines"]) and st["cracked"] == sum(r["hit"] for r in fx["rows"]) == 57
    assert ran == KEY_PARALLEL


def test_crack_files(tmp_path):
    """g. The one-ESSID fixture's hash file through dwpa_crack_files, the dictionary as a file: rc 1, one record per
    control and long-target hit, no near-miss retired."""
    fx = P.fixture("single")
    df = tmp_path / "d.txt"
    df.write_bytes(b"".join(w + b"\n" for w in fx["words"]))
    _crack(tmp_path, fx, lambda hf, out: dwpa_amd.crack_files(hf, [str(df)], None, 8, out, device_mask=1,
                                                              batch=BATCH))
    assert M.crack_stats()["words"] == P.NWORDS


def test_crack_mask_window(tmp_path):
    """g. The eight-digit fixture through dwpa_crack_mask on a window of 4,096 indices of ?d x 8 around its PSK."""
    fx = P.fixture("digits")
    at = int(fx["psk"])
    assert M.mask_candidate(P.MASK_DIGITS, at) == fx["psk"] == P.PSK_DIGITS
    skip, limit = at - 1500, 4096
    _crack(tmp_path, fx, lambda hf, out: dwpa_amd.crack_mask(hf, P.MASK_DIGITS, (), skip=skip, limit=limit,
                                                             nonce_error_corrections=8, out_file=out, device_mask=1,
                                                             batch=512))
    assert M.crack_stats()["candidates"] == limit
