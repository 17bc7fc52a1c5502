"""GPU recall and precision of the association attack: k_prep_assoc through the scan API (set_assoc / load_assoc / run)
and dwpa_crack_assoc through its command line.

The all-plants method of tests/test_gpu_table.py: EVERY candidate of every loaded window is the PSK of exactly one line
of its own net, the expected set comes from the CPU oracle, and the hits must equal it as a set of (line, id, nc, endian,
PMK) -- none missing, none extra, none twice.  The candidates come from the reference of tests/assoc_plan.py, which
tests/test_assoc_plan.py checks on the CPU.  No scan loads the same `first` twice, so no slot holds a candidate it held
before and a stale PMK cannot stand in for one the kernel skipped.
"""
import os
import random
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

import dwpa_amd  # noqa: E402
from dwpa_amd import _lib as L  # noqa: E402
from tests import assoc_plan as A  # noqa: E402
from tests import test_gpu_recall as R  # noqa: E402
from tests.test_gpu_recall import sizes  # noqa: E402,F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC = A.NC
MS_FAMILY = {"k_pbkdf2_ms", "k_pbkdf2_gfx950_ms", "k_pbkdf2_gfx950_ms_p"}
KEY_PARALLEL = {"k_verify<pmkid>", "k_verify<kv1>", "k_verify<kv2>", "k_verify<kv3>"}


def essid_of(n):
    """Distinct ESSIDs of 1..32 bytes: the salt's length moves with the net."""
    return (b"net%04d-" % n + b"abcdefghijklmnopqrstuvwx")[:1 + (n * 7) % 32] if n % 5 else b"N%d" % n


def make_nets(count, base=0):
    nets = [(essid_of(base + n), A.mac(base + n)) for n in range(count)]
    assert len(set(nets)) == count
    return nets


class Fixture:
    """Nets, their words and rules; lines planted for the candidates of `windows`; the expected hits."""

    def __init__(self, nets, words, rules, windows, seed, kinds=(0, 1, 2, 3), extra_psks=None):
        self.plan = plan = A.Plan(None, rules=rules, nets=nets, words=words)
        assert plan.dropped == 0
        ids = sorted({i for first, count in windows for i in range(first, first + count)})
        assert ids and ids[-1] < plan.k
        by_psk, psks = {}, [[] for _ in nets]
        for i in ids:
            c = plan.candidate(i)
            if c is None:
                continue
            n = plan.net_of(i)
            assert not c.endswith(b"\0")
            if (n, c) not in by_psk:
                psks[n].append(c)
            by_psk.setdefault((n, c), []).append(i)
        for n, more in (extra_psks or {}).items():  # lines whose PSK their own net never tries
            psks[n] += more
        self.lines, self.owner, pmks, found = A.plant(nets, psks, random.Random(seed), kinds)
        self.exp = {(ln, i, found[ln][0], found[ln][1], pmks[ln]) for ln, (n, psk) in enumerate(self.owner)
                    for i in by_psk.get((n, psk), [])}
        self.kept = {i for v in by_psk.values() for i in v}
        self.rules_text = "\n".join(rules) if rules else ""

    def scan(self, batch):
        sc = dwpa_amd.Scan(self.lines, nc=NC, batch=batch)
        assert sc.nets == len(self.plan.nets)
        assert [sc.net_of_line(ln) for ln in range(len(self.lines))] == [n for n, _ in self.owner]
        assert sc.set_assoc(*self.plan.flat(), self.rules_text) == self.plan.k
        return sc

    def window(self, sc, held, first, count, what):
        assert first not in held, "a slot would hold a candidate it held before"
        held.add(first)
        sc.load_assoc(first, count)
        assert sc.loaded() == sum(1 for i in range(first, first + count) if i in self.kept), (what, first, count)
        sc.run()
        R._assert_same(R._hitset(sc.hits(cap=1 << 16)), {p for p in self.exp if first <= p[1] < first + count},
                       (what, first, count))

    def recall(self, windows, batch, what):
        L.pbkdf2_kernels(reset=True)
        sc = self.scan(batch)
        try:
            held = set()
            for first, count in windows:
                self.window(sc, held, first, count, what)
        finally:
            sc.close()
        ran = L.pbkdf2_kernels()
        assert ran and ran <= MS_FAMILY, ran  # per-slot salt only: no one-ESSID and no _mg kernel
        return ran


# ---------------------------------------------------------------------------------------------------------------
# the index: where a lane finds its net
# ---------------------------------------------------------------------------------------------------------------
def test_sixty_four_nets_per_wave():
    """200 nets of one index each: every lane of a wave stands in a net of its own, every segment holds one lane, the
    last wave is partial, and windows start in the middle of a wave's nets."""
    nets = make_nets(200)
    words = [[b"own-word-%06d" % n] for n in range(200)]
    windows = [(0, 200), (1, 64), (37, 130), (63, 2), (199, 1)]
    Fixture(nets, words, None, windows, 0xa1).recall(windows, 512, "ones")


WIDE_W, WIDE_R = 33, 35
WIDE_RULES = [":"] + ["$%s" % c for c in "abcdefghijklmnopqrstuvwxyz01234567"]  # 35 rules, 35 distinct results


def test_one_net_over_waves_and_blocks():
    """One net of 33 words x 35 rules = 1155 indices, no power of two: five blocks that all find the same net, windows
    that start and end inside it; rule-major, so a wave holds two or three rules."""
    assert len(WIDE_RULES) == WIDE_R
    nets = make_nets(1)
    words = [A.counter_words(b"wide", WIDE_W)]
    windows = [(0, 1155), (100, 300), (1154, 1), (640, 515)]
    fx = Fixture(nets, words, WIDE_RULES, windows, 0xa2)
    assert fx.plan.k == 1155 and len(fx.kept) == 1155
    fx.recall(windows, 1216, "wide")


def test_rejecting_and_length_changing_rules():
    """W = 7 under the rules of tests/test_gpu_recall.py: rejects, results below 8 and above 63 bytes, two rules with
    one result.  loaded() is the reference's kept count, and a PSK that two indices give is hit by both."""
    lens = (5, 7, 8, 9, 30, 56, 63)
    words = [[((b"rj%d" if k == 3 else b"Rj%d") % k + b"abcdefghijklmnopqrstuvwxyzabcdefghijklmnopqrstuvwxyzabcdefghij")[:n - 2]
              + b"-%d" % k for k, n in enumerate(lens)]]  # word 3 is lower case: ':' and 'l' give one PSK
    assert [len(w) for w in words[0]] == list(lens)
    k = 7 * len(R.RULES)
    windows = [(0, k), (3, 20), (k - 9, 9)]
    fx = Fixture(make_nets(1, 300), words, R.RULES, windows, 0xa3)
    cands = [fx.plan.candidate(i) for i in range(k)]
    assert None in cands and 0 < len(fx.kept) < k and len({c for c in cands if c}) < len(fx.kept)
    fx.recall(windows, 256, "rules")


MIXED = ["e"] + ["1"] * 35 + ["e"] + ["1"] * 35 + ["e", "W", "e"] + ["1"] * 30 + ["e"] + ["1"] * 40 + ["e"]
MIXED_SMALL = ["1"] * 10 + ["e", "W", "e"] + ["1"] * 10 + ["e", "1"]


def mixed_fixture(layout, base, wide_words):
    """Nets after a layout: "1" a net of one word, "W" the wide net, "e" a net that owns nothing (W = 0)."""
    nets = make_nets(len(layout), base)
    words = [[] if what == "e" else wide_words if what == "W" else [b"mx-%06d" % n] for n, what in enumerate(layout)]
    return nets, words, layout.index("W")


def test_mixed_nets_and_empty_nets():
    """A wave's first id lies in one net and its last in another; `first` and `first + count` fall inside the wide net;
    nets with W = 0 between the others own nothing."""
    nets, words, wide = mixed_fixture(MIXED, 400, A.counter_words(b"mixed-wide", 1155))  # 1155 words, R = 1
    windows = [(0, 100), (60, 200), (500, 300), (1000, 295), (69, 2), (1224, 2), (7, 1288)]
    fx = Fixture(nets, words, None, windows, 0xa4)
    assert fx.plan.k == 70 + 1155 + 70 and fx.plan.start[wide] == 70
    fx.recall(windows, 1344, "mixed")


def test_mixed_nets_under_rules():
    """The same shape with R = 35 everywhere: the one-word nets own 35 indices each, the wide net 33 x 35."""
    nets, words, wide = mixed_fixture(MIXED_SMALL, 560, A.counter_words(b"mixed-wide", WIDE_W))
    k = 21 * 35 + 1155
    windows = [(0, k), (300, 700), (k - 40, 40), (419, 2)]
    fx = Fixture(nets, words, WIDE_RULES, windows, 0xa5)
    assert fx.plan.k == k
    fx.recall(windows, 1920, "mixed+rules")


def test_four_classes():
    """One net with lines of PMKID and keyver 1, 2 and 3, four of each: every line is found by its own candidate, and
    the four key-parallel classes each ran once per load."""
    nets = make_nets(1, 600)
    words = [A.counter_words(b"class", 16)]
    fx = Fixture(nets, words, None, [(0, 16)], 0xa6)
    assert len(fx.lines) == 16 and len(fx.exp) == 16
    L.verify_kernels(reset=True)
    ran = fx.recall([(0, 16), (5, 7)], 64, "classes")
    assert L.verify_kernels() == KEY_PARALLEL
    assert ran == ({"k_pbkdf2_ms"} if not R._env_flag("DWPA_PBKDF2_ISSUE") or R._env_flag("DWPA_PBKDF2_PLAIN")
                   else {"k_pbkdf2_gfx950_ms_p"})


# ---------------------------------------------------------------------------------------------------------------
# precision: the association holds
# ---------------------------------------------------------------------------------------------------------------
def test_association_holds():
    """Nets A and B share an ESSID and differ in MAC_AP; C and D share a MAC_AP and differ in ESSID.  A and C own the
    word x, B and D do not.  Lines of B and D whose PSK is x are never reported -- B's would accept A's PMK -- and A's
    and C's are, with the owning net's index."""
    x = b"shared-psk-x-000000"
    nets = [(b"one-essid", A.mac(701)), (b"one-essid", A.mac(702)), (b"essid-C", A.mac(703)), (b"essid-D", A.mac(703))]
    words = [[b"a-own-000001", x, b"a-own-000002"], [b"b-own-000001", b"b-own-000002"],
             [x, b"c-own-000001"], [b"d-own-000001"]]
    fx = Fixture(nets, words, None, [(0, 8)], 0xa7, extra_psks={1: [x], 3: [x]})
    assert len(fx.lines) == 8 + 2 and len(fx.exp) == 8
    silent = [ln for ln, (n, psk) in enumerate(fx.owner) if n in (1, 3) and psk == x]
    assert len(silent) == 2 and not {p for p in fx.exp if p[0] in silent}
    assert {p[1] for p in fx.exp if fx.owner[p[0]][1] == x} == {1, 5}  # x at A's index 1 and C's index 5 only
    fx.recall([(0, 8), (1, 5), (4, 4)], 64, "precision")


# ---------------------------------------------------------------------------------------------------------------
# the issue-pass kernels and segment growth
# ---------------------------------------------------------------------------------------------------------------
def test_issue_pass_kernels(sizes):
    """One filler net with one line and enough indices that a load's kept count selects k_pbkdf2_gfx950_ms_p (above one
    wave per SIMD: 2 x slots > level_lanes) and another's k_pbkdf2_gfx950_ms (above one round: 2 x slots > 8 x
    level_lanes), as pbkdf2_module.cpp states the thresholds.  150 two-word nets before the filler and 150 after it
    are planted: exactly the plants are reported."""
    ll = sizes["level_lanes"]
    fill = (4 * ll // 64 + 1) * 64 + ll // 2 + 1024
    nets = make_nets(301, 800)
    words = [[b"ip-%04d-a" % n, b"ip-%04d-b" % n] for n in range(150)] + [A.counter_words(b"filler", fill)] + \
            [[b"ip-%04d-a" % n, b"ip-%04d-b" % n] for n in range(151, 301)]
    k = 300 + fill + 300
    w1 = (0, 300 + ll // 2 + 64)
    w2 = (w1[1], k - w1[1])
    assert 2 * w1[1] > ll and 2 * w1[1] <= 8 * ll and 2 * w2[1] > 8 * ll
    fx = Fixture(nets, words, None, [(0, 300), (k - 300, 300)], 0xa8)
    assert fx.plan.k == k and len(fx.exp) == 600
    fx.kept = set(range(k))  # the filler's candidates are kept too; its one line has a PSK nobody tries
    sc = fx.scan((w2[1] + 63) // 64 * 64)
    try:
        held = set()
        for w, kernel in ((w1, "k_pbkdf2_gfx950_ms_p"), (w2, "k_pbkdf2_gfx950_ms")):
            L.pbkdf2_kernels(reset=True)
            fx.window(sc, held, *w, "issue pass")
            assert L.pbkdf2_kernels() == {"k_pbkdf2_ms" if R._env_flag("DWPA_PBKDF2_PLAIN") else kernel}
    finally:
        sc.close()


def test_segment_lists_grow():
    """With segment lists of one record, a load whose classes need hundreds of segments -- the 1155 lines of the wide
    net against every run of its lanes -- returns the same hits as with the default capacity."""
    nets, words, wide = mixed_fixture(MIXED, 400, A.counter_words(b"mixed-wide", 1155))
    windows = [(0, 1295), (64, 640)]
    fx = Fixture(nets, words, None, windows, 0xa9)
    L.assoc_work(reset=True)
    fx.recall(windows, 1344, "default capacity")
    base = L.assoc_work(reset=True)
    assert base["slots_derived"] == 1295 + 640 and base["segments"] > 4 * 100
    assert L.assoc_segcap(1) == 0
    try:
        fx.recall([(1, 1294), (65, 639)], 1344, "capacity 1")
    finally:
        assert L.assoc_segcap(0) == 1
    grown = L.assoc_work(reset=True)
    assert grown["slots_derived"] == 1294 + 639 and grown["segments"] > 4 * 100


def test_refusals_on_a_live_scan():
    """A load before any association, first + count > K (also when the sum wraps), count above the batch, per-group
    calls while an association is loaded, and bad set calls, which leave the association that was set in force."""
    fx = Fixture(make_nets(3, 900), [[b"refuse-%06d" % n] for n in range(3)], None, [(0, 3)], 0xaa)
    sc = dwpa_amd.Scan(fx.lines, nc=NC, batch=64)

    def refused(fn, *a, **kw):
        with pytest.raises(L.DwpaError) as e:
            fn(*a, **kw)
        assert e.value.code == L.DWPA_E_ARG, a

    try:
        refused(sc.load_assoc, 0, 1)
        words, nets = fx.plan.flat()
        assert sc.set_assoc(words, nets) == 3
        for first, count in ((0, 4), (3, 1), (4, 0), (2**64 - 1, 2), (0, 128)):
            refused(sc.load_assoc, first, count)
        sc.load_assoc(3, 0)
        assert sc.loaded() == 0
        sc.load_assoc(0, 3)
        refused(sc.pbkdf2, 0)
        refused(sc.verify, 0)
        refused(sc.set_assoc, words, [0, 2, 1])          # net numbers decrease
        refused(sc.set_assoc, words, [0, 1, 3])          # no such net
        refused(sc.set_assoc, [b"", b"x", b"y"], nets)   # an empty word
        refused(sc.set_assoc, [b"L" * 257, b"x", b"y"], nets)
        with pytest.raises(L.DwpaError) as e:
            sc.set_assoc(words, nets, "not a rule at all")
        assert e.value.code == L.DWPA_E_RULE
        fx.window(sc, set(), 0, 3, "after the refusals")
        sc.load_numeric(0, 64)  # another kind of load: the per-group calls work again
        sc.pbkdf2(0)
        sc.verify(0)
        assert sc.hits() == []
    finally:
        sc.close()


# ---------------------------------------------------------------------------------------------------------------
# dwpa_crack_assoc
# ---------------------------------------------------------------------------------------------------------------
CRACK_RULES = [":", "u", "$1", "c $!", "^x"]


@pytest.fixture(scope="module")
def cfiles(tmp_path_factory):
    """40 nets, an association file of three words per net (one MAC under two ESSIDs), --single and five rules.  Every
    line's PSK is a candidate of its own net, at an index that moves through the net's words and rules."""
    d = tmp_path_factory.mktemp("gpu_assoc")
    nets = make_nets(40, 1000)
    nets[7] = (b"twin-of-six", nets[6][1])
    assoc = [m.hex().encode() + b":" + w for n, (e, m) in enumerate(nets) if n != 7
             for w in A.counter_words(b"crack%02d" % n, 3)]
    assoc += [b"0a0b0c0d0e0f:nobody-has-this-mac", b"not an association line"]
    pre = A.Plan(None, assoc, True, CRACK_RULES, nets=nets)
    rng = random.Random(0xab)
    psks, ids = [[] for _ in nets], {}
    for n in range(len(nets)):
        for _ in range(1 + n % 2):  # one or two lines per net
            while True:
                i = rng.randrange(pre.start[n], pre.start[n + 1])
                c = pre.candidate(i)
                if c is not None and c not in psks[n]:
                    break
            psks[n].append(c)
    lines, owner, pmks, found = A.plant(nets, psks, rng)
    plan = A.Plan(lines, assoc, True, CRACK_RULES)
    assert plan.info() == pre.info() and plan.unmatched == 1 and plan.malformed == 1
    (d / "h.hash").write_bytes(b"\n".join(lines) + b"\n")
    A.write_assoc(d / "a.txt", assoc)
    (d / "r.rule").write_text("".join(r + "\n" for r in CRACK_RULES))
    return {"dir": d, "plan": plan, "lines": lines, "owner": owner, "hash": str(d / "h.hash"), "afile": str(d / "a.txt"),
            "rules": str(d / "r.rule")}


def _expected_records(cf, first, count):
    """The records of the lines whose PSK their own net tries inside [first, first + count)."""
    plan = cf["plan"]
    tried = {}
    for i in range(first, first + count):
        c = plan.candidate(i)
        if c is not None:
            tried.setdefault(plan.net_of(i), set()).add(c)
    hit = [ln for ln, (n, psk) in enumerate(cf["owner"]) if psk in tried.get(n, ())]
    return sorted(R._records([cf["lines"][ln] for ln in hit], [cf["owner"][ln][1] for ln in hit])), len(hit)


def _assoc_cli(cf, out, *extra, env=None):
    argv = [sys.executable, "-m", "dwpa_amd.assoc", cf["hash"], cf["afile"], "--single", "-r", cf["rules"], "--batch",
            "512", "--nonce-error-corrections", str(NC), "-o", str(out), *extra]
    r = subprocess.run(argv, cwd=ROOT, capture_output=True, timeout=120, env=dict(os.environ, **(env or {})))
    recs = out.read_bytes().split(b"\n") if out.exists() else [b""]
    assert recs.pop() == b""
    return r, recs


def test_crack_every_line(cfiles, tmp_path):
    """The whole keyspace in loads of 512: exit 0, every line once with its PSK, the counts on stderr."""
    exp, n = _expected_records(cfiles, 0, cfiles["plan"].k)
    assert n == len(cfiles["lines"]) == 60 and cfiles["plan"].k > 4 * 512
    r, recs = _assoc_cli(cfiles, tmp_path / "o.key")
    assert r.returncode == 0 and r.stdout == b"", r.stderr[-2000:]
    assert sorted(recs) == exp
    assert b"40 nets, %d entries, 5 rules" % cfiles["plan"].entries in r.stderr
    assert b"1 unmatched, 1 malformed" in r.stderr and b"60/60 hashlines cracked" in r.stderr


def test_crack_window_and_shards(cfiles, tmp_path):
    """-s / -l: exit 1 and exactly the lines whose PSK the window tries; then everything with two shards per device."""
    plan = cfiles["plan"]
    s, l = plan.start[5] + 3, plan.start[23] - plan.start[5]
    exp, n = _expected_records(cfiles, s, l)
    assert 0 < n < 60
    r, recs = _assoc_cli(cfiles, tmp_path / "w.key", "-s", str(s), "-l", str(l))
    assert r.returncode == 1 and sorted(recs) == exp, r.stderr[-2000:]
    exp, n = _expected_records(cfiles, 0, plan.k)
    r, recs = _assoc_cli(cfiles, tmp_path / "s.key", env={"DWPA_CRACK_SHARDS_PER_DEVICE": "2"})
    assert r.returncode == 0 and sorted(recs) == exp, r.stderr[-2000:]
    r, recs = _assoc_cli(cfiles, tmp_path / "e.key", "-s", str(plan.k))
    assert r.returncode == 255 and not (tmp_path / "e.key").exists()


def test_a_retired_net_costs_nothing(tmp_path):
    """Net 0 owns 2,000 indices and its only line falls to its first candidate; net 1 is never cracked.  In loads of
    512 the first derives 512 slots of net 0; after it net 0 is retired and none of its later 1,488 slots is derived."""
    nets = make_nets(2, 1100)
    words = [A.counter_words(b"retire", 2000), A.counter_words(b"other", 100)]
    pre = A.Plan(None, nets=nets, words=words)
    lines, owner, _, _ = A.plant(nets, [[pre.candidate(0)], [b"nobody-tries-this"]], random.Random(0xac))
    hf, af, out = tmp_path / "h.hash", tmp_path / "a.txt", tmp_path / "o.key"
    hf.write_bytes(b"\n".join(lines) + b"\n")
    A.write_assoc(af, [m.hex().encode() + b":" + w for (e, m), ws in zip(nets, words) for w in ws])
    L.assoc_work(reset=True)
    L.pbkdf2_kernels(reset=True)
    rc = dwpa_amd.crack_assoc(str(hf), str(af), nonce_error_corrections=NC, out_file=str(out), batch=512)
    work = L.assoc_work(reset=True)
    assert rc == 1
    assert out.read_bytes().split(b"\n") == R._records(lines[:1], [pre.candidate(0)]) + [b""]
    assert work["slots_derived"] == 512 + 100, work
    assert work["segments"] == 512 // 64 + 2, work  # eight waves of net 0, net 1's 100 lanes in two waves' runs
    assert L.pbkdf2_kernels() <= MS_FAMILY
    st = dwpa_amd.m22000.crack_stats()
    assert st["candidates"] == 512 + 100 and st["cracked"] == 1 and st["hashes"] == 2
