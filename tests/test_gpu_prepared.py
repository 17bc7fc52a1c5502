"""GPU: the prepared-candidate differential.  Every candidate generator of the scan path -- k_prep_dict,
k_prep_numeric, k_rules_prep, k_prep_mask, k_prep_markov, k_prep_hybrid, k_prep_combinator, k_prep_chain,
k_prep_chain_rules, k_prep_table and both instantiations of k_prep_assoc -- loads the windows of the seeded random
specifications of tests/prepared_plan.py, and the batch it leaves is read back (dwpa_debug_scan_prepared) and compared
with the model: the raw kept counter, loaded(), the set of ids with none twice, and per id the ten HMAC-SHA1 key
midstate words, bit for bit; for the association also each slot's salt reference.  No PBKDF2 and no verify kernel
runs, so tens of thousands of candidates cost well under a second of device time; the numpy model is the cost.

The midstates are an exact witness of the candidate's bytes up to one thing, which this file cannot see and does not
work round: a candidate and the same candidate followed by NUL bytes are one HMAC key and have one midstate (the
all-plants recall tests have the same blind spot and assert it away).

A specification the library refuses fails its test.  A load that keeps more than the batch cannot be made through the
scan API (tests/prepared_plan.py says why); each list loads windows of exactly the batch instead.
"""
import random

import pytest

pytestmark = pytest.mark.gpu

import dwpa_amd  # noqa: E402
from dwpa_amd import _lib as L  # noqa: E402
from dwpa_amd.device import Dictionary  # noqa: E402
from tests import prepared_plan as P  # noqa: E402
from tests import synth as S  # noqa: E402
from tests import test_gpu_chain as G  # noqa: E402

LINE = S.pmkid_line(b"", b"prepared", bytes.fromhex("02a500000001"), bytes.fromhex("02a5000000fe"), the_pmk=bytes(32))


def cases(name):
    return pytest.mark.parametrize("case", range(len(P.specs(name))), ids=[s["name"] for s in P.specs(name)])


def check(sc, name, spec, win, sref=None):
    """The load has been issued: read the batch back and hold it to the model."""
    a = P.ATTACKS[name]
    m = P.model(a, spec, win)
    prep = L.scan_prepared(sc, sref=sref is not None)
    expect = None if sref is None else P.assoc_srefs(spec, a.plan(spec), m)
    try:
        P.compare(m, prep, batch=sc.batch, loaded=sc.loaded(), sref=expect)
    except AssertionError as e:
        raise AssertionError("%s %s window %r: %s" % (a.kernel, spec["name"], win, e)) from None


def scan(lines=(LINE,)):
    sc = dwpa_amd.Scan(list(lines), batch=P.BATCH)
    assert sc.batch == P.BATCH
    return sc


@cases("mask")
def test_prep_mask(case):
    spec = P.specs("mask")[case]
    sc = scan()
    try:
        assert sc.set_mask(spec["mask"], spec["custom"]) == P.ATTACKS["mask"].keyspace(spec)
        for first, count in spec["windows"]:
            sc.load_mask(first, count)
            check(sc, "mask", spec, (first, count))
    finally:
        sc.close()


@cases("markov")
def test_prep_markov(case):
    spec = P.specs("markov")[case]
    sc = scan()
    try:
        k = sc.set_mask(spec["mask"], spec["custom"], markov=P.markov_model()[1], threshold=spec["threshold"])
        assert k == P.ATTACKS["markov"].keyspace(spec)
        for first, count in spec["windows"]:
            sc.load_mask(first, count)
            check(sc, "markov", spec, (first, count))
    finally:
        sc.close()


@cases("numeric")
def test_prep_numeric(case):
    spec = P.specs("numeric")[case]
    sc = scan()
    try:
        for first, count in spec["windows"]:
            sc.load_numeric(first, count, spec["digits"])
            check(sc, "numeric", spec, (first, count))
    finally:
        sc.close()


@cases("dict")
def test_prep_dict(case):
    spec = P.specs("dict")[case]
    d = Dictionary.from_words(spec["words"])
    sc = scan()
    try:
        for first, count in spec["windows"]:
            sc.load_dict(d.off.ptr, d.data.ptr, first, count)
            check(sc, "dict", spec, (first, count))
    finally:
        sc.close()


@cases("rules")
def test_rules_prep(case):
    spec = P.specs("rules")[case]
    d = Dictionary.from_words(spec["words"])
    sc = scan()
    try:
        assert sc.set_rules(P.rules_bytes(spec["rules"])) == len(spec["rules"])
        for first, nwords in spec["windows"]:
            sc.load_rules(d.off.ptr, d.data.ptr, first, nwords)
            check(sc, "rules", spec, (first, nwords))
    finally:
        sc.close()


@cases("hybrid")
def test_prep_hybrid(case):
    spec = P.specs("hybrid")[case]
    d = Dictionary.from_words(spec["words"])
    sc = scan()
    try:
        assert sc.set_mask(spec["mask"], spec["custom"]) * len(spec["words"]) == P.ATTACKS["hybrid"].keyspace(spec)
        for fw, nw, mf, mc in spec["windows"]:
            sc.load_hybrid(d.off.ptr, d.data.ptr, fw, nw, mf, mc, spec["mode"])
            check(sc, "hybrid", spec, (fw, nw, mf, mc))
    finally:
        sc.close()


@cases("combinator")
def test_prep_combinator(case):
    spec = P.specs("combinator")[case]
    db, da = Dictionary.from_words(spec["base"]), Dictionary.from_words(spec["amp"])
    sc = scan()
    try:
        for fb, nb, af, ac in spec["windows"]:
            sc.load_combinator(db.off.ptr, db.data.ptr, fb, nb, da.off.ptr, da.data.ptr, len(spec["amp"]), af, ac,
                               spec["side"])
            check(sc, "combinator", spec, (fb, nb, af, ac))
    finally:
        sc.close()


@cases("chain")
def test_prep_chain(case):
    spec = P.specs("chain")[case]
    ch = P.ATTACKS["chain"].chain(spec)
    dev = G.Device(ch)
    sc = scan()
    try:
        assert sc.set_chain(dev.parts, spec["custom"]) == ch.k
        for first, count in spec["windows"]:
            sc.load_chain(first, count)
            check(sc, "chain", spec, (first, count))
    finally:
        sc.close()


@cases("chain_rules")
def test_prep_chain_rules(case):
    spec = P.specs("chain_rules")[case]
    ch = P.ATTACKS["chain_rules"].chain(spec)
    dev = G.Device(ch)
    sc = scan()
    try:
        k = sc.set_chain(dev.parts, spec["custom"])
        for p, part in enumerate(spec["parts"]):
            if isinstance(part, tuple):
                k = sc.set_chain_rules(p, P.rules_bytes(part[1]))
                assert sc.chain_nrules == len(part[1])
        assert k == ch.k
        for first, count in spec["windows"]:
            sc.load_chain(first, count)
            check(sc, "chain_rules", spec, (first, count))
    finally:
        sc.close()


@cases("table")
def test_prep_table(case):
    spec = P.specs("table")[case]
    plan = P.ATTACKS["table"].plan(spec)
    d = Dictionary.from_words(plan.words)
    sc = scan()
    try:
        got = sc.set_table(d.off.ptr, d.data.ptr, len(plan.words), plan.table, plan.minlen, plan.maxlen, plan.word_max)
        assert got == (plan.k, plan.kept())
        for first, count in spec["windows"]:
            sc.load_table(first, count)
            check(sc, "table", spec, (first, count))
    finally:
        sc.close()


def _assoc(name, case):
    spec = P.specs(name)[case]
    plan = P.ATTACKS[name].plan(spec)
    rng = random.Random(case)
    lines = [S.pmkid_line(b"", e, m, rng.randbytes(6), the_pmk=rng.randbytes(32)) for e, m in spec["nets"]]
    sc = scan(lines)
    try:
        assert sc.nets == len(spec["nets"]) and [sc.net_of_line(i) for i in range(len(lines))] == list(range(len(lines)))
        words, nets = plan.flat()
        rules = P.rules_bytes(spec["rules"]) if spec["rules"] is not None else b""
        assert sc.set_assoc(words, nets, rules) == plan.k
        for first, count in spec["windows"]:
            sc.load_assoc(first, count)
            check(sc, name, spec, (first, count), sref=True)
    finally:
        sc.close()


@cases("assoc_plain")
def test_prep_assoc_without_rules(case):
    _assoc("assoc_plain", case)


@cases("assoc_rules")
def test_prep_assoc_with_rules(case):
    _assoc("assoc_rules", case)
