"""GPU recall of rules on chain list parts: k_prep_chain_rules through the scan API (set_chain / set_chain_rules /
load_chain) and dwpa_crack_chain_rules through the command line.

The all-plants method of tests/test_gpu_chain.py: EVERY kept candidate of a load is the PSK of one line per ESSID,
the expected set comes from tests/chain_rules_plan.RuledChain (rule-major choices, oracle/rules.py's pieces, the
63-byte limit on a ruled part's RESULT), and the hits must equal it -- none missing, none extra, none twice, ids and
PMKs equal -- while loaded() must equal the kept count.  tests/test_chain_rules_plan.py checks, without a GPU, that
the fixtures can be planted and show every drop reason.  Batch sizes follow from the device's CU count as in
test_gpu_recall, and every scan test asserts which PBKDF2 kernel ran.
"""
import json
import os
import random
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

import dwpa_amd  # noqa: E402
from dwpa_amd import _lib as L  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import chain_rules_plan as P  # noqa: E402
from tests import test_gpu_chain as G  # noqa: E402
from tests import test_gpu_recall as R  # noqa: E402
from tests.test_gpu_chain import plant  # noqa: E402
from tests.test_gpu_recall import sizes  # noqa: E402,F401  (the fixture)

ROOT = G.ROOT
NC = R.NC
ONE = (b"chain-rules",)


@pytest.fixture(scope="module")
def fx():
    """Every fixture of the plan planted once under one ESSID, and [ruled list, mask] under the three ESSIDs of
    test_gpu_recall too (one of 52 bytes)."""
    out = {}
    for k, (name, (ch, windows, reasons)) in enumerate(sorted(P.fixtures().items())):
        if name.startswith("crack"):
            continue
        kept = P.planted(ch, windows)
        lines, exp, psks = plant(kept, ONE, 0x70 + k)
        out[name] = {"chain": ch, "windows": windows, "kept": kept, "lines": lines, "exp": exp}
    f = out["RM"]
    lines, exp, psks = plant(f["kept"], R.ESSIDS, 0x6f)
    out["RM3"] = dict(f, lines=lines, exp=exp)
    return out


def set_ruled(sc, dev, ch):
    """set_chain, then the rules part by part: K grows from the un-ruled product to the chain's."""
    assert sc.set_chain(dev.parts, ch.custom) == ch.unruled().k
    k = ch.unruled().k
    for p, part in enumerate(ch.given):
        if isinstance(part, tuple):
            k = sc.set_chain_rules(p, P.rules_text(part[1]))
            assert sc.chain_nrules == len(part[1])
    assert k == ch.k == sc.chain_keyspace
    return k


def recall(lines, exp, chain, loads, batch, how, kernel):
    """The chain and its rules set once, then every load: loaded() == the kept count and the hits are exactly the
    load's plants."""
    dev = G.Device(chain)
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(lines, nc=NC, batch=batch)
    held = set()
    try:
        set_ruled(sc, dev, chain)
        for first, count in loads:
            ids = [i for i, psk in chain.kept(first, count)]
            slots = set(enumerate(ids))
            assert not slots & held, "a slot would hold a candidate it held before"
            held |= slots
            sc.load_chain(first, count)
            assert sc.loaded() == len(ids), (first, count)
            R._scan_all(sc, how)
            R._assert_same(R._hitset(sc.hits(cap=8192)), {p for p in exp if p[1] in set(ids)}, (how, first, count))
    finally:
        sc.close()
    assert L.pbkdf2_kernels() == {kernel}


def _hits_of(sc, load, count):
    load()
    assert sc.loaded() == count
    R._scan_all(sc, "per_group")
    return R._hitset(sc.hits(cap=8192))


# ---------------------------------------------------------------------------------------------------------------
# 1, 2: equal to the paths that exist
# ---------------------------------------------------------------------------------------------------------------
def test_equal_to_the_rules_path(fx, sizes):
    """1. One ruled list alone gives what Scan.set_rules + load_rules give on the same words and rules: the same
    PSKs and PMKs, the ids renamed from word * R + rule to rule * nwords + word."""
    f = fx["alone"]
    ch = f["chain"]
    nw, nr = len(P.LE), len(P.RSA)
    assert ch.k == nw * nr and 40 <= len(f["kept"]) < ch.k
    dev = G.Device(ch)
    d = dev.dicts[0]
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(f["lines"], nc=NC, batch=sizes["one"]["p"])
    try:
        set_ruled(sc, dev, ch)
        by_chain = _hits_of(sc, lambda: sc.load_chain(0, ch.k), len(f["kept"]))
        assert sc.set_rules(P.rules_text(P.RSA)) == nr
        by_rules = _hits_of(sc, lambda: sc.load_rules(d.off.ptr, d.data.ptr, 0, nw), len(f["kept"]))
        again = _hits_of(sc, lambda: sc.load_chain(0, ch.k), len(f["kept"]))  # set_rules left the chain's rules alone
    finally:
        sc.close()
    R._assert_same(by_chain, f["exp"], "chain")
    assert by_chain == again == {(ln, (i % nr) * nw + i // nr, nc, en, pmk) for ln, i, nc, en, pmk in by_rules}
    assert L.pbkdf2_kernels() == {R.expected_kernel("one", "p")}


def test_colon_on_every_list_equals_the_unruled_chain(fx, sizes):
    """2. ':' on every list part gives the hit set of the same chain without rules, under the same ids (no list of
    it holds an empty word, which ':' rejects and an un-ruled part keeps)."""
    f = fx["colon"]
    ch = f["chain"]
    assert ch.unruled().kept(0, ch.k) == f["kept"] and ch.unruled().k == ch.k and len(f["kept"]) >= 30
    dev = G.Device(ch)
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(f["lines"], nc=NC, batch=sizes["one"]["p"])
    try:
        assert sc.set_chain(dev.parts, ch.custom) == ch.k
        plain = _hits_of(sc, lambda: sc.load_chain(0, ch.k), len(f["kept"]))
        set_ruled(sc, dev, ch)
        ruled = _hits_of(sc, lambda: sc.load_chain(0, ch.k), len(f["kept"]))
    finally:
        sc.close()
    R._assert_same(ruled, f["exp"], "ruled")
    assert plain == ruled
    assert L.pbkdf2_kernels() == {R.expected_kernel("one", "p")}


# ---------------------------------------------------------------------------------------------------------------
# 3, 4, 5, 6: shapes, the distinct-rule loop, carries, run()
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", P.SHAPES)
def test_whole_key_space(fx, sizes, name):
    """3. Ruled list + mask, mask + ruled list, two ruled lists under different rule sets, and un-ruled + ruled + mask
    + ruled: the whole key space in one load."""
    f = fx[name]
    assert f["chain"].k <= 4000 and 200 <= len(f["kept"]) <= 1000
    recall(f["lines"], f["exp"], f["chain"], [(0, f["chain"].k)], sizes["one"]["p"], "per_group",
           R.expected_kernel("one", "p"))


@pytest.mark.parametrize("nwords", P.LOOP_NWORDS)
def test_distinct_rule_loop(fx, sizes, nwords):
    """4. The last part ruled with 1, 3, 63, 64 and 65 words under 72 rules: a wave holds 64, 22, 2, 1-2 and 1-2
    distinct rules.  Windows whose `first` is no multiple of 64, that cross a rule boundary inside a wave, of 1, 63, 65
    and 200 raw indices (a partial last wave), and up to K (tests/test_chain_rules_plan.py checks all that)."""
    f = fx["loop%d" % nwords]
    recall(f["lines"], f["exp"], f["chain"], f["windows"], sizes["one"]["p"], "per_group",
           R.expected_kernel("one", "p"))


@pytest.mark.parametrize("name", P.SHAPES)
def test_carries(fx, sizes, name):
    """5. Windows that wrap a ruled part into the part before it, every part into the one before it, and the first
    part into nothing (the end of K)."""
    f = fx[name]
    recall(f["lines"], f["exp"], f["chain"], P.carry_windows(f["chain"]), sizes["one"]["p"], "per_group",
           R.expected_kernel("one", "p"))


def test_run_over_three_essids(fx, sizes):
    """6. [ruled list, mask] through run() over three ESSIDs, one of them 52 bytes long: the whole key space and a
    window."""
    f = fx["RM3"]
    ch = f["chain"]
    recall(f["lines"], f["exp"], ch, [(0, ch.k), (ch.k // 3 + 1, 200)], sizes["mg"]["p"], "run",
           R.expected_kernel("mg", "p"))


# ---------------------------------------------------------------------------------------------------------------
# 7: argument errors on a live scan
# ---------------------------------------------------------------------------------------------------------------
def test_set_chain_rules_errors_leave_the_scan_usable(fx, sizes):
    f = fx["RM"]
    ch = f["chain"]
    un = ch.unruled()
    dev = G.Device(ch)
    la, m = dev.parts
    nw = len(P.LA)
    text = P.rules_text(P.RSA)
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(f["lines"], nc=NC, batch=sizes["one"]["p"])

    def refused(call, code=L.DWPA_E_ARG):
        with pytest.raises(L.DwpaError) as e:
            call()
        assert e.value.code == code

    def good(chain, exp_ids=None):
        """A load of the whole key space of `chain` (what the scan must still hold) gives its hits."""
        kept = [i for i, psk in chain.kept(0, chain.k)]
        sc.load_chain(0, chain.k)
        assert sc.loaded() == len(kept)
        R._scan_all(sc, "per_group")
        want = {p for p in f["exp"] if p[1] in set(kept if exp_ids is None else exp_ids)}
        R._assert_same(R._hitset(sc.hits(cap=8192)), want, "after a refusal")

    # rule 0 of the ruled chain is ':', so the un-ruled chain's kept candidates are its first ones, under the same ids
    assert P.RSA[0] == ":" and [c for c in ch.kept(0, un.k)] == un.kept(0, un.k) and un.kept(0, un.k)
    try:
        refused(lambda: sc.set_chain_rules(0, text))                    # no chain
        assert sc.set_chain(dev.parts, ch.custom) == un.k
        assert sc.set_chain_rules(0, text) == ch.k and sc.chain_nrules == len(P.RSA)
        for part in (1, 2, 7, 2**32 - 1):                               # a mask part; part >= nparts
            refused(lambda: sc.set_chain_rules(part, text))
            good(ch)
        refused(lambda: sc.set_chain_rules(0, "no such rule\n# nothing\n"), L.DWPA_E_RULE)  # no valid rule
        good(ch)
        refused(lambda: sc.set_chain_rules(1, "no such rule\n"))        # what is wrong with the call comes first
        # the rules come off and go on again
        assert sc.set_chain_rules(0, b"") == un.k and sc.chain_nrules == 0
        good(un)
        assert sc.set_chain_rules(0, text) == ch.k
        good(ch)
        # set_chain again clears the rules: K falls back to the un-ruled product
        assert sc.set_chain(dev.parts, ch.custom) == un.k
        good(un)
        # nwords = 2^31 claimed with two rules is 2^32 choices: refused before anything is read, and the chain as set
        # -- whose first words are the list's -- stays
        assert sc.set_chain([(L.DWPA_CHAIN_LIST, la[1], la[2], 2**31), m], ch.custom) == 2**31 * 6
        refused(lambda: sc.set_chain_rules(0, ":\nc\n"))
        sc.load_chain(0, un.k)
        assert sc.loaded() == len(un.kept(0, un.k))
        R._scan_all(sc, "per_group")
        R._assert_same(R._hitset(sc.hits(cap=8192)), {p for p in f["exp"] if p[1] in {i for i, c in un.kept(0, un.k)}},
                       "after the 2^31 claim")
        assert sc.set_chain_rules(0, ":\n") == 2**31 * 6                 # one rule fits
        # K above 2^64 - 1: (2^31 - 1) x 2^32 x 2 fits, twice that does not
        big = [(L.DWPA_CHAIN_LIST, la[1], la[2], 2**31 - 1), (L.DWPA_CHAIN_MASK, b"?b?b?b?b"), (L.DWPA_CHAIN_MASK, b"?1")]
        assert sc.set_chain(big, ch.custom) == (2**31 - 1) * 2**33
        refused(lambda: sc.set_chain_rules(0, ":\nc\n"))
        assert sc.chain_keyspace == (2**31 - 1) * 2**33
        # and a good chain with rules after all of it
        set_ruled(sc, dev, ch)
        good(ch)
    finally:
        sc.close()
    assert L.pbkdf2_kernels() == {R.expected_kernel("one", "p")}


# ---------------------------------------------------------------------------------------------------------------
# 8: dwpa_crack_chain_rules through the command line
# ---------------------------------------------------------------------------------------------------------------
_CRACK_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
from dwpa_amd import chain as CLI
from dwpa_amd import m22000 as M
res = []
for argv in json.load(open(sys.argv[2])):
    rc = CLI.main(argv)
    res.append({"rc": rc, "stats": M.crack_stats(), "workers": M.crack_worker_stats()})
print(json.dumps(res))
"""


def _child(tmp_path, name, runs, **env):
    jp = tmp_path / (name + ".json")
    jp.write_text(json.dumps(runs))
    e = {k: v for k, v in os.environ.items() if k != "DWPA_RULE_MODE"}
    e.update(env, DWPA_CRACK_SHARDS_PER_DEVICE="2")
    r = subprocess.run([sys.executable, "-c", _CRACK_CHILD, ROOT, str(jp)], env=e, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _records(path):
    recs = open(path, "rb").read().split(b"\n")
    assert recs.pop() == b""
    return sorted(recs)


def test_crack_chain_rules(tmp_path):
    """8. [list A under a rules file, list B, ?d?1] at batch 64 with two workers on one device, in child processes.
    The file's last rule uses a reject function: hashcat's -r loader (the default) skips it, DWPA_RULE_MODE=full runs
    it, so R -- and with it K and every id -- differs by that line, and rules_skipped says so.
    Plants at the lowest and the highest kept id and inside a -s/-l window: rc 0 and the outfile PSKs are the ruled
    strings; the window alone cracks only its plant; an exhausted run gives rc 1 with candidates = the reference's
    kept count; an inline rule:c works."""
    hc, full = P.crack_chain(False), P.crack_chain(True)
    assert len(hc.rules[0]) == 3 and len(full.rules[0]) == 4 and full.k == hc.k // 3 * 4
    kept = dict(hc.kept(0, hc.k))
    ids = sorted(kept)
    mid = ids[len(ids) // 2]
    planted = [ids[0], mid, ids[-1]]
    assert 100 < len(kept) < hc.k and len({hc.split(0, hc.digits(i)[0])[0] for i in planted}) == 3  # every rule
    lines, exp, psks = plant([(i, kept[i]) for i in planted], ONE, 0x90)
    # under the fourth rule only: '>6 $#' on a 9-byte word
    fkept = dict(full.kept(0, full.k))
    only_full = [i for i in sorted(fkept) if full.split(0, full.digits(i)[0])[0] == 3]
    assert only_full and fkept[only_full[-1]] not in kept.values()
    flines, fexp, fpsks = plant([(only_full[-1], fkept[only_full[-1]])], ONE, 0x91)
    # rule:c alone
    inline = P.RuledChain([(P.CRACK_A, ["c"]), P.CRACK_B, P.CRACK_MASK], P.CRACK_CUSTOM)
    ikept = inline.kept(0, inline.k)
    ilines, iexp, ipsks = plant(ikept[-1:], ONE, 0x92)
    rng = random.Random(0x93)
    outside = b"no-chain-gives-this"
    extra = R._line(0, 0, "LE", outside, ONE[0], O.c_pbkdf2(outside, ONE[0]), rng)

    pa, pb, pr = tmp_path / "a.txt", tmp_path / "b.txt", tmp_path / "a.rule"
    pa.write_bytes(b"".join(w + b"\n" for w in P.CRACK_A))
    pb.write_bytes(b"\n".join(P.CRACK_B))
    pr.write_text("# capitalise, append\n" + "\n".join(P.CRACK_RULES) + "\n")
    hashes = {}
    for name, ls in (("all", lines), ("extra", lines + [extra]), ("full", flines + [extra]), ("inline", ilines)):
        hashes[name] = tmp_path / (name + ".hash")
        hashes[name].write_bytes(b"\n".join(ls) + b"\n")
    out = {k: str(tmp_path / (k + ".key")) for k in ("whole", "window", "exhausted", "inline", "full")}
    chain = ["list:" + str(pa), "rules:" + str(pr), "list:" + str(pb), "mask:" + P.CRACK_MASK.decode()]
    common = ["-1", "ab", "--batch", "64", "--nonce-error-corrections", str(NC)]
    runs = [[str(hashes["all"]), *chain, *common, "-o", out["whole"]],
            [str(hashes["all"]), *chain, *common, "-o", out["window"], "-s", str(mid - 70), "-l", "150"],
            [str(hashes["extra"]), *chain, *common, "-o", out["exhausted"]],
            [str(hashes["inline"]), chain[0], "rule:c", *chain[2:], *common, "-o", out["inline"]]]
    whole, window, exhausted, inl = _child(tmp_path, "hashcat", runs)
    every = sorted(R._records(lines, psks))
    assert whole["rc"] == 0 and _records(out["whole"]) == every
    assert len(whole["workers"]) == 2 and len({w["device"] for w in whole["workers"]}) == 1
    assert whole["stats"]["rules"] == 3 and whole["stats"]["rules_skipped"] == 1 == whole["stats"]["rules_rejmem"]
    assert whole["stats"]["words"] == len(P.CRACK_A) + len(P.CRACK_B) and whole["stats"]["cracked"] == 3
    # the window holds the middle plant alone
    assert ids[0] < mid - 70 and mid + 80 < ids[-1]
    assert window["rc"] == 1 and _records(out["window"]) == [R._records(lines, psks)[[p[1] for p in sorted(exp)].index(mid)]]
    assert window["stats"]["candidates"] == len(hc.kept(mid - 70, 150)) and window["stats"]["cracked"] == 1
    # exhausted: every raw index was loaded once, the kept ones derived
    assert exhausted["rc"] == 1 and _records(out["exhausted"]) == every
    assert exhausted["stats"]["candidates"] == len(kept) and exhausted["stats"]["hashes"] == 4
    assert sum(w["items"] for w in exhausted["workers"]) == (hc.k + 63) // 64
    assert inl["rc"] == 0 and _records(out["inline"]) == sorted(R._records(ilines, ipsks))
    assert inl["stats"]["rules"] == 1 and inl["stats"]["rules_skipped"] == 0
    # DWPA_RULE_MODE=full: the fourth rule runs
    (fullrun,) = _child(tmp_path, "full", [[str(hashes["full"]), *chain, *common, "-o", out["full"]]],
                        DWPA_RULE_MODE="full")
    assert fullrun["rc"] == 1 and _records(out["full"]) == sorted(R._records(flines, fpsks))
    assert fullrun["stats"]["rules"] == 4 and fullrun["stats"]["rules_skipped"] == 0 == fullrun["stats"]["rules_rejmem"]
    assert fullrun["stats"]["candidates"] == len(fkept) > len(kept)
    assert sum(w["items"] for w in fullrun["workers"]) == (full.k + 63) // 64
