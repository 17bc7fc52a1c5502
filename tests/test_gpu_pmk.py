"""GPU: the PMK differential.  Every PBKDF2 kernel a scan can launch writes its PMKs where the verifier reads them; the
tests below read them back (dwpa_debug_scan_pmks: copies only) and compare all eight words of every slot, bit for bit.

A scan otherwise shows its PMKs only through hits, and a wrong PMK at a slot nobody planted a line for is reported by
nothing.  Here nothing is planted at all: every line is a PMKID line of a PSK no candidate equals, so hits() stays empty
and nothing retires, and what is compared is the buffer itself --

* with the CPU oracle's PMKs (tests/pmk_plan.py, OpenSSL): every slot of the small launches, and 1,024 / 512 per group
  sampled slots of the large ones (every structural position, then seeded filler);
* for the large launches, every slot with a re-derivation of the same candidates through k_pbkdf2 in loads of at most
  one wave per SIMD -- the kernel case a compares slot by slot with the oracle;
* past the loaded count, with the words the buffer held before the derive: a lane past the count must not write.  Before
  a partial load the scan loads a full batch of other candidates and does not derive them, so that the midstates past
  the count are not the ones their stale PMKs came from: a lane that did write would write something else.

Batch sizes that select a kernel come from the device's CU count (tests/test_gpu_recall.py sizes); every test asserts
the exact set of PBKDF2 kernels that ran, and the last test the set the whole file reached.
"""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import dwpa_amd  # noqa: E402
from dwpa_amd import _lib as L  # noqa: E402
from dwpa_amd import m22000 as M  # noqa: E402
from tests import assoc_plan as A  # noqa: E402
from tests import pmk_plan as P  # noqa: E402
from tests import synth as S  # noqa: E402
from tests import test_gpu_recall as R  # noqa: E402
from tests.test_gpu_recall import sizes  # noqa: E402,F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC = 8
CHILD = bool(os.environ.get(P.FIXTURE_ENV))  # a forced-build child: cases a-d only
REACHED = set()   # PBKDF2 kernels the file's tests (and their children) saw run
CASES = set()     # which cases ran in this process
TALLY = {}        # case -> [PMKs read back and compared, of them against the oracle, of them against a re-derivation]


def _ran(expected, case):
    ran = L.pbkdf2_kernels()
    assert ran == set(expected), (case, sorted(ran))
    REACHED.update(ran)
    CASES.add(case)


def _tally(case, read=0, oracle=0, rederived=0):
    t = TALLY.setdefault(case, [0, 0, 0])
    t[0] += read
    t[1] += oracle
    t[2] += rederived


def _ms_kernel():
    return "k_pbkdf2_gfx950_ms_p" if R._env_flag("DWPA_PBKDF2_ISSUE") and not R._env_flag("DWPA_PBKDF2_PLAIN") \
        else "k_pbkdf2_ms"


@pytest.fixture(scope="module")
def cus():
    assert dwpa_amd.device_count() >= 1
    return R._cu_count()


@pytest.fixture(scope="module")
def tb(cus, sizes):  # noqa: F811
    assert P.sizes(cus) == sizes
    t = P.tables(cus)
    if not CHILD:
        print("oracle: %d PMKs in %.2f s (%.0f PMK/s)" % (len(t.pmk), t.seconds, len(t.pmk) / t.seconds))
    return t


def _loads():
    """(first, count) of the loads of cases a and b: the full batch, then the partial ones, each one value later."""
    return [(P.SLOTS_FIRST + k, c) for k, c in enumerate((P.SLOTS,) + P.COUNTS)]


def _load(sc, first, count, poison):
    """load_numeric of [first, first + count); ahead of a partial load, a full batch of `poison` values that nothing
    derives, so the midstates past the count belong to no PMK the buffer holds."""
    if count < sc.batch:
        sc.load_numeric(poison, sc.batch, P.DIGITS)
    sc.load_numeric(first, count, P.DIGITS)
    assert sc.loaded() == count


# ---------------------------------------------------------------------------------------------------------------
# a, b: every slot of a 1,088-slot batch, and the stale tail
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("essid", P.SLOT_ESSIDS, ids=["essid1", "essid32"])
def test_every_slot_per_group(tb, essid):
    """a. pbkdf2(0) at batch 1,088 (four workgroups and a wave): all 1,088 slots, then loads of 1,087 ... 1 candidates,
    each starting one value later than the one before, so no slot derives what it derived last time.  Slots below the
    count are the oracle's; slots at or above it hold what the load before left."""
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan([P.scan_line(essid)], nc=NC, batch=P.SLOTS)
    try:
        assert sc.groups == 1 and sc.batch == P.SLOTS
        held = L.scan_pmks(sc)
        for k, (first, count) in enumerate(_loads()):
            _load(sc, first, count, P.SLOTS_POISON + 4096 * k)
            before = L.scan_pmks(sc)
            assert (before == held).all(), "a load wrote PMK words"
            sc.pbkdf2(0)
            got = L.scan_pmks(sc)
            want = held.copy()
            want[:, :count] = tb.numeric(essid, range(first, first + count))
            msg = P.compare(got, want, [(j, first + j) for j in range(P.SLOTS)], prev=before)
            assert not msg, (count, msg)
            _tally("a", P.SLOTS, count)
            sc.verify(0)
            held = got
        assert sc.hits() == []
    finally:
        sc.close()
    _ran({R.expected_kernel("one", "plain")}, "a")


def test_every_slot_run(tb):
    """b. The same through run(): the two ESSIDs as two groups of one k_pbkdf2_mg launch, each group's column block
    read back, the stale tail held per group."""
    essids = P.group_order(P.SLOT_ESSIDS)
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan([P.scan_line(e, k) for k, e in enumerate(essids)], nc=NC, batch=P.SLOTS)
    try:
        assert sc.groups == 2
        with pytest.raises(L.DwpaError) as err:  # no run() yet: no launch holds the group
            L.scan_pmks(sc, 0, run=True)
        assert err.value.code == L.DWPA_E_ARG
        held = None
        for k, (first, count) in enumerate(_loads()):
            _load(sc, first, count, P.SLOTS_POISON + 4096 * k)
            sc.run()
            got = [L.scan_pmks(sc, g, run=True) for g in range(2)]
            for g, e in enumerate(essids):
                want = got[g].copy() if held is None else held[g].copy()
                want[:, :count] = tb.numeric(e, range(first, first + count))
                msg = P.compare(got[g], want, [(g, j, first + j) for j in range(P.SLOTS)],
                                prev=None if held is None else held[g])
                assert not msg, (count, len(e), msg)
                _tally("b", P.SLOTS, count)
            held = got
        assert sc.hits() == []
        with pytest.raises(L.DwpaError):
            L.scan_pmks(sc, 2, run=True)
    finally:
        sc.close()
    _ran({R.expected_kernel("mg", "plain")}, "b")


# ---------------------------------------------------------------------------------------------------------------
# c: the salt sweep
# ---------------------------------------------------------------------------------------------------------------
def test_salt_sweep(tb):
    """c. One scan over every ESSID of the plan (lengths 1..33, 51 | 52, 115 | 116: one, two and three salt blocks;
    NUL, LF and 0xff among the bytes), 64 candidates: pbkdf2(g) for every group, then, after a fresh load, one run()
    whose launch holds groups of one, two and three blocks side by side.  The line with the empty ESSID, which the
    oracle refuses, is refused here too and makes no group."""
    order = P.group_order(P.ESSIDS)
    assert {P.nsalt(e) for e in order} == {1, 2, 3}
    lines = [P.scan_line(e, k) for k, e in enumerate(P.ESSIDS)] + [P.scan_line(e, 99) for e in P.REFUSED]
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(lines, nc=NC, batch=P.SWEEP)
    try:
        assert sc.groups == len(order) == 37 and sc.batch == P.SWEEP
        assert [sc.line_status(i) for i in range(len(lines))] == [0] * 37 + [L.DWPA_E_HEX] * len(P.REFUSED)
        first = P.SWEEP_FIRST
        sc.load_numeric(first, P.SWEEP, P.DIGITS)
        assert sc.loaded() == P.SWEEP
        for g, e in enumerate(order):
            sc.pbkdf2(g)
            msg = P.compare(L.scan_pmks(sc), tb.numeric(e, range(first, first + P.SWEEP)),
                            [(g, j, first + j) for j in range(P.SWEEP)])
            assert not msg, ("pbkdf2(g)", len(e), P.nsalt(e), msg)
            sc.verify(g)
            _tally("c", P.SWEEP, P.SWEEP)
        _ran({R.expected_kernel("one", "plain")}, "c")
        L.pbkdf2_kernels(reset=True)
        L.scan_work(reset=True)
        first += 1
        sc.load_numeric(first, P.SWEEP, P.DIGITS)
        sc.run()
        work = L.scan_work()
        assert (work["pbkdf2_launches"], work["groups_derived"]) == (1, 37), work
        for g, e in enumerate(order):
            msg = P.compare(L.scan_pmks(sc, g, run=True), tb.numeric(e, range(first, first + P.SWEEP)),
                            [(g, j, first + j) for j in range(P.SWEEP)])
            assert not msg, ("run()", len(e), P.nsalt(e), msg)
            _tally("c", P.SWEEP, P.SWEEP)
        assert sc.hits() == []
    finally:
        sc.close()
    _ran({R.expected_kernel("mg", "plain")}, "c")


# ---------------------------------------------------------------------------------------------------------------
# d: the association, mixed salts in a wave
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rules", [False, True], ids=["plain", "rule"])
def test_assoc_mixed_salts(tb, rules):
    """d. 40 nets whose ESSIDs cycle through 1, 51, 52, 115, 116 and 32 bytes, one to three words each: neighbouring
    lanes of a wave read different salt entries, and the trip count of their salt loop differs.  PMK[slot] is the
    oracle's for the slot's candidate under its own net's ESSID; the slots past the count are not written."""
    ac = P.assoc_case(rules)
    plan = ac["plan"]
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(ac["lines"], nc=NC, batch=128)
    try:
        assert sc.nets == len(ac["nets"]) and sc.batch == 128 > plan.k > 64
        assert sc.set_assoc(*plan.flat(), P.ASSOC_RULE if rules else "") == plan.k
        sc.load_assoc(0, plan.k)
        assert sc.loaded() == plan.k
        before = L.scan_pmks(sc)
        sc.run()
        prep = L.scan_prepared(sc, sref=True)
        ids = [int(i) for i in prep["ids"]]
        assert prep["count"] == plan.k and sorted(ids) == list(range(plan.k))
        essids = [ac["essid_of"][i] for i in ids]
        ns = [P.nsalt(e) for e in essids]
        assert any(set(ns[w:w + 64]) == {1, 2, 3} for w in range(0, plan.k, 64))
        assert sum(a != b for a, b in zip(ns, ns[1:])) >= 10  # lanes next to each other differ in their trip count
        assert len(set(zip(prep["sref"].tolist(), essids))) == len(set(essids)) == len(P.ASSOC_LENGTHS)
        got = L.scan_pmks(sc)
        want = before.copy()
        for j, i in enumerate(ids):
            want[:, j] = tb.words(essids[j], [ac["cands"][i]])[:, 0]
        msg = P.compare(got, want, [(j, ids[j], len(essids[j])) if j < plan.k else j for j in range(128)],
                        prev=before)
        assert not msg, msg
        _tally("d", 128, plan.k)
        assert sc.hits() == []
    finally:
        sc.close()
    _ran({_ms_kernel()}, "d")


# ---------------------------------------------------------------------------------------------------------------
# e: a-d with the kernel choice forced
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch", ["DWPA_PBKDF2_ISSUE", "DWPA_PBKDF2_PLAIN"])
def test_forced_builds(tb, tmp_path, switch):
    """e. Cases a-d in a fresh child process (the switches are read once per process) with the issue-pass kernels
    forced -- k_pbkdf2_gfx950_p, _mg_p and _ms_p at sizes that otherwise run the plain schedule -- and with the plain
    kernels forced.  The child reads the oracle's tables from this process's pickle and leaves the kernels it reached."""
    fxp, rp = tmp_path / "tables.pkl", tmp_path / "reached.txt"
    with open(fxp, "wb") as f:
        pickle.dump(tb, f)
    env = {k: v for k, v in os.environ.items() if k not in ("DWPA_PBKDF2_PLAIN", "DWPA_PBKDF2_ISSUE")}
    env.update({switch: "1", P.FIXTURE_ENV: str(fxp), P.REACHED_ENV: str(rp)})
    sel = "every_slot_per_group or every_slot_run or salt_sweep or assoc_mixed or kernels_reached"
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        os.path.abspath(__file__), "-k", sel], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "7 passed" in r.stdout, r.stdout[-500:]
    got = set(rp.read_text().split())
    want = {"k_pbkdf2", "k_pbkdf2_mg", "k_pbkdf2_ms"} if switch == "DWPA_PBKDF2_PLAIN" \
        else {"k_pbkdf2_gfx950_p", "k_pbkdf2_gfx950_mg_p", "k_pbkdf2_gfx950_ms_p"}
    assert got == want, sorted(got)
    REACHED.update(got)
    CASES.add("e")


# ---------------------------------------------------------------------------------------------------------------
# f-h: the large launches
# ---------------------------------------------------------------------------------------------------------------
def _rederive(essids, first, n, step):
    """PMKs of candidates [first, first + n) under each ESSID, through a second scan in loads of at most `step`
    (<= one wave per SIMD: k_pbkdf2, or what the process's switches make of such a launch; under DWPA_PBKDF2_ISSUE that
    is k_pbkdf2_gfx950_p, which the forced child of case a holds to the oracle slot by slot): [uint32[8][n] per
    group]."""
    L.pbkdf2_kernels(reset=True)
    out = [np.zeros((8, n), dtype=np.uint32) for _ in essids]
    sc = dwpa_amd.Scan([P.scan_line(e, 50 + k) for k, e in enumerate(essids)], nc=NC, batch=step)
    try:
        assert sc.groups == len(essids) and sc.batch == step
        for b in range(0, n, step):
            c = min(step, n - b)
            sc.load_numeric(first + b, c, P.DIGITS)
            for g in range(len(essids)):
                sc.pbkdf2(g)
                out[g][:, b:b + c] = L.scan_pmks(sc)[:, :c]
    finally:
        sc.close()
    ran = L.pbkdf2_kernels()
    assert ran == {R.expected_kernel("one", "plain")}, ran
    return out


def _oracle_at(tb, got, prev, essid, first, pos):
    """compare() of the sampled slots with the oracle's PMKs."""
    pos = np.asarray(pos)
    return P.compare(got[:, pos], tb.numeric(essid, [first + int(s) for s in pos]), [int(s) for s in pos],
                     prev=None if prev is None else prev[:, pos])


def test_queue_kernel_every_slot(tb, cus, sizes):  # noqa: F811
    """f. k_pbkdf2_gfx950_q: Q + 193 candidates under the 32-byte ESSID (Q: one resident round, so waves take second
    items and the last item is a partial wave).  All slots are read; the oracle checks the 1,024 sampled ones, a
    re-derivation through k_pbkdf2 every one; the slots past the count keep the words the buffer had.  A second load of
    Q + 1 candidates that starts 7 values later must give the first load's PMKs 7 slots to the left, and leave slots
    [Q + 1, n) as the first load wrote them."""
    qc = P.queue_case(cus)
    q, n, essid, first = qc["q"], qc["n"], qc["essid"], qc["first"]
    assert q == 4 * sizes["level_lanes"] and n == q + 193
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan([P.scan_line(essid)], nc=NC, batch=n)
    try:
        cap = sc.batch
        assert sc.groups == 1 and cap == (n + 63) // 64 * 64
        before = L.scan_pmks(sc)
        sc.load_numeric(first, n, P.DIGITS)
        assert sc.loaded() == n
        sc.pbkdf2(0)
        sc.verify(0)
        got = L.scan_pmks(sc)
        _ran({R.expected_kernel("one", "q")}, "f")
        sampled = _oracle_at(tb, got, before, essid, first, qc["sample"])
        want = before.copy()
        want[:, :n] = _rederive([essid], first, n, sizes["one"]["plain"])[0]
        msg = P.compare(got, want, range(cap), prev=before)
        assert not msg and not sampled, ("first load", "every slot: " + msg, "oracle sample: " + sampled)
        _tally("f", cap, len(qc["sample"]), n)
        # the second load
        L.pbkdf2_kernels(reset=True)
        _load(sc, first + P.QUEUE_SHIFT, q + 1, P.QUEUE_POISON)
        sc.pbkdf2(0)
        sc.verify(0)
        got2 = L.scan_pmks(sc)
        assert q + 1 + P.QUEUE_SHIFT <= n
        want = got.copy()
        want[:, :q + 1] = got[:, P.QUEUE_SHIFT:q + 1 + P.QUEUE_SHIFT]
        msg = P.compare(got2, want, range(cap), prev=got)
        assert not msg, ("second load", msg)
        _tally("f", cap, 0, q + 1)
        assert sc.hits() == []
    finally:
        sc.close()
    _ran({R.expected_kernel("one", "q")}, "f")


def _group_run(tb, case, batch, n, poison, kernel, sizes_, what):  # noqa: F811
    """A run() of three groups at `batch` with n candidates loaded: every column block read, the oracle at the case's
    sample, every slot against the re-derivation, the slots past n as a first run() of other candidates left them."""
    essids, first = case["essids"], case["first"]
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan([P.scan_line(e, k) for k, e in enumerate(essids)], nc=NC, batch=batch)
    try:
        assert sc.groups == 3 and sc.batch == batch
        before = None
        if n < batch:
            sc.load_numeric(poison[0], batch, P.DIGITS)
            sc.run()
            before = [L.scan_pmks(sc, g, run=True) for g in range(3)]
            _load(sc, first, n, poison[1])
        else:
            sc.load_numeric(first, n, P.DIGITS)
        sc.run()
        got = [L.scan_pmks(sc, g, run=True) for g in range(3)]
        assert sc.hits() == []
    finally:
        sc.close()
    _ran({kernel}, what)
    ref = _rederive(essids, first, n, sizes_["one"]["plain"])
    for g, e in enumerate(essids):
        sampled = _oracle_at(tb, got[g], before and before[g], e, first, case["sample"][g])
        want = got[g].copy() if before is None else before[g].copy()
        want[:, :n] = ref[g]
        msg = P.compare(got[g], want, range(batch), prev=before and before[g])
        assert not msg and not sampled, (what, g, len(e), "every slot: " + msg, "oracle sample: " + sampled)
        _tally(what, batch, len(case["sample"][g]), n)


def test_group_queue_kernel_every_slot(tb, cus, sizes):  # noqa: F811
    """g. k_pbkdf2_gfx950_mg_q: ESSIDs of 1, 52 and 116 bytes (one, two, three salt blocks) at the smallest batch whose
    three groups exceed one resident round, batch - 37 candidates loaded.  The oracle checks 512 positions per group,
    the re-derivation every slot, and the last 37 slots of every group stay as an earlier run() left them."""
    gc = P.group_case(cus)
    assert gc["batch"] == sizes["mg"]["q"] and 3 * gc["batch"] > gc["q"]
    _group_run(tb, gc, gc["batch"], gc["n"], P.GROUP_POISON, R.expected_kernel("mg", "q"), sizes, "g")


def test_priority_kernels_at_full_load(tb, cus, sizes):  # noqa: F811
    """h. The smallest k_pbkdf2_gfx950_p and k_pbkdf2_gfx950_mg_p batches with every slot loaded: every slot against
    the re-derivation, the structural positions against the oracle."""
    pc = P.prio_cases(cus)
    one = pc["one"]
    batch, essid, first = one["batch"], one["essid"], one["first"]
    assert batch == sizes["one"]["p"]
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan([P.scan_line(essid)], nc=NC, batch=batch)
    try:
        before = L.scan_pmks(sc)
        sc.load_numeric(first, batch, P.DIGITS)
        assert sc.loaded() == batch == sc.batch
        sc.pbkdf2(0)
        sc.verify(0)
        got = L.scan_pmks(sc)
        assert sc.hits() == []
    finally:
        sc.close()
    _ran({R.expected_kernel("one", "p")}, "h")
    sampled = _oracle_at(tb, got, before, essid, first, one["sample"])
    msg = P.compare(got, _rederive([essid], first, batch, sizes["one"]["plain"])[0], range(batch), prev=before)
    assert not msg and not sampled, ("h one", "every slot: " + msg, "oracle sample: " + sampled)
    _tally("h", batch, len(one["sample"]), batch)
    mg = pc["mg"]
    assert mg["batch"] == sizes["mg"]["p"]
    _group_run(tb, mg, mg["batch"], mg["batch"], None, R.expected_kernel("mg", "p"), sizes, "h")


# ---------------------------------------------------------------------------------------------------------------
# i: the check path
# ---------------------------------------------------------------------------------------------------------------
def test_check_path_mixed_salts(tb):
    """i. One dwpa_check_batch of 192 PMKID jobs, one key each, ESSIDs of 1, 51, 52 and 116 bytes in turn: neighbouring
    slots of the per-slot-salt kernel differ in their salt's block count.  Every job hits with the oracle's PMK, and
    the device derived all 192."""
    jobs, exp = [], []
    for j, (e, k) in enumerate(P.check_case()):
        pmk = tb.pmk[(e, k)]
        line = S.pmkid_line(k, e, A.mac(0x920000 + j), b"\x02\x5c" + j.to_bytes(4, "big"), the_pmk=pmk)
        jobs.append((line, [k], False, NC))
        exp.append([k, None, None, pmk])
    L.pbkdf2_kernels(reset=True)
    got = dwpa_amd.check_batch(jobs)
    st = M.check_stats()
    assert st["backend"] == L.DWPA_BACKEND_DEVICE and st["pmks"] == P.CHECK_JOBS and st["hits"] == P.CHECK_JOBS, st
    bad = [(j, len(jobs[j][1][0]), g and g[3].hex()) for j, (g, x) in enumerate(zip(got, exp)) if g != x]
    assert not bad, (len(bad), bad[:4])
    _tally("i", P.CHECK_JOBS, P.CHECK_JOBS)
    # no tail at this size: a call below two wave units (CUs x 128 PMKs each) is all head (engine.cpp head_pmks)
    _ran({_ms_kernel()}, "i")


# ---------------------------------------------------------------------------------------------------------------
# which kernels the file reached
# ---------------------------------------------------------------------------------------------------------------
# Never launched by a scan: dwpa_scan_pbkdf2 and dwpa_scan_run always pass a work counter, so a launch that is too
# large for the priority kernel runs as a work queue (pbkdf2_module.cpp), never as the plain-priority grid kernel.
UNREACHABLE_FROM_A_SCAN = {"k_pbkdf2_gfx950", "k_pbkdf2_gfx950_mg"}
# Check-path kernels this file does not size a call for: the head of a call above one priority round, and the tail
# beside it.  tests/test_gpu_recall.py::test_check_path_non_priority_kernel compares every PMK of both.
CHECK_PATH_ONLY = {"k_pbkdf2_gfx950_ms", "k_pbkdf2_ms_tail"}


def test_kernels_reached():
    """Of the twelve PBKDF2 kernel names the file and its children ran eight -- every kernel a scan call can launch,
    the association's per-slot-salt kernels among them -- and the other four are listed above with the reason."""
    assert UNREACHABLE_FROM_A_SCAN | CHECK_PATH_ONLY <= set(L.PBKDF2_KERNEL_NAMES)
    if CHILD:  # cases a-d under a forced choice: leave the set for the parent
        assert CASES == {"a", "b", "c", "d"}, CASES
        with open(os.environ[P.REACHED_ENV], "w") as f:
            f.write(" ".join(sorted(REACHED)))
        return
    for case, (read, oracle, rederived) in sorted(TALLY.items()):
        print("%s: %d PMKs read back, %d compared with the oracle, %d with a re-derivation" %
              (case, read, oracle, rederived))
    assert not REACHED & UNREACHABLE_FROM_A_SCAN, sorted(REACHED)
    forced = R._env_flag("DWPA_PBKDF2_PLAIN") or R._env_flag("DWPA_PBKDF2_ISSUE")
    if CASES >= set("abcdefghi") and not forced:
        print("kernels reached: the whole file ran, the exact set is asserted: %s" % sorted(REACHED))
        assert REACHED == set(L.PBKDF2_KERNEL_NAMES) - UNREACHABLE_FROM_A_SCAN - CHECK_PATH_ONLY, sorted(REACHED)
    else:  # a selection of the file's tests, or a forced kernel choice: nothing outside the expected set
        print("kernels reached: WEAKER CHECK, subset only -- cases run %s of a..i, kernel choice %s: %s" %
              (sorted(CASES), "forced" if forced else "free", sorted(REACHED)))
        assert REACHED <= set(L.PBKDF2_KERNEL_NAMES) - UNREACHABLE_FROM_A_SCAN - CHECK_PATH_ONLY, sorted(REACHED)
