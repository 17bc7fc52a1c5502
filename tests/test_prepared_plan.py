"""CPU: tests/prepared_plan.py is what tests/test_gpu_prepared.py takes it for.  The SHA-1 of the midstate model is
right (against hashlib / hmac); the committed spec lists cover what they claim to, counted from the lists, so that a
later edit of a seed cannot lose a case unseen; and compare(), the comparison the GPU tests make, catches each of a
handful of deliberately wrong models on every list the slip can touch."""
import hashlib
import hmac
import random

import numpy as np
import pytest

from tests import prepared_plan as P
from tests import table_plan as T
from tests import test_markov as MK

NAMES = tuple(P.ATTACKS)
FILTERING = tuple(n for n in NAMES if P.ATTACKS[n].compacts)
# what the limits rule out, and for a dictionary's ids across 2^32 the cost (tests/prepared_plan.py's docstring has
# the reasons)
NO_2_32 = ("dict", "assoc_plain")
NO_2_63 = NO_2_32 + ("rules", "assoc_rules", "combinator", "table")
NO_DUPLICATES = ("mask", "markov", "numeric")


# ---------------------------------------------------------------------------------------------------------------
# the midstate model
# ---------------------------------------------------------------------------------------------------------------
def test_sha1_is_hashlibs():
    rng = random.Random(0x51)
    for n in [0, 1, 3, 54, 55, 56, 57, 63, 64, 65, 119, 120, 128, 1000] + [rng.randrange(300) for _ in range(40)]:
        data = rng.randbytes(n)
        assert P.sha1(data) == hashlib.sha1(data).digest(), n


def test_midstates_finish_to_hmac_sha1():
    """Keys of every length 0..64 (and random ones, trailing NULs among them), random messages: HMAC-SHA1 finished from
    the model's ten words is hmac's.  One vectorised call gives what single calls give."""
    rng = random.Random(0x52)
    keys = [rng.randbytes(n) for n in range(65)] + [rng.randbytes(rng.randrange(65)) for _ in range(200)]
    keys += [b"key\0", b"key", b"\xff" * 64, bytes(64), b""]
    mid = P.midstates(keys)
    assert mid.shape == (10, len(keys)) and mid.dtype == np.uint32
    for j, k in enumerate(keys):
        msg = rng.randbytes(rng.choice((0, 1, 20, 55, 56, 64, 100, 200)))
        assert P.hmac_sha1_from_mid(mid[:, j], msg) == hmac.new(k, msg, hashlib.sha1).digest(), (j, k)
    assert (P.midstates(keys[7:8]) == mid[:, 7:8]).all()
    # rows 0..4 are the inner (0x36) state: the device's order, prep_dev.hpp store_mid
    inner = P.sha1_compress(P._iv(1), P._blocks(bytes(c ^ 0x36 for c in keys[64]))[0].reshape(16, 1))
    assert (mid[:5, 64:65] == inner).all()
    # the one blind spot: a key and the same key with trailing NULs are one HMAC key
    assert (mid[:, keys.index(b"key\0")] == mid[:, keys.index(b"key")]).all()


def test_the_remembered_markov_rows_are_ref_markov():
    a, n = P.ATTACKS["markov"], P.markov_model()[0]
    rng = random.Random(0x53)
    for s in P.specs("markov"):
        r = a._r(s)
        for i in [0, r["k"] - 1] + [rng.randrange(r["k"]) for _ in range(6)]:
            assert a.cand(s, i) == MK.ref_markov(n, r["sets"], s["threshold"], i), (s["name"], i)


# ---------------------------------------------------------------------------------------------------------------
# the comparison itself
# ---------------------------------------------------------------------------------------------------------------
def _fails(model, prep, **kw):
    try:
        P.compare(model, prep, **kw)
    except AssertionError:
        return True
    return False


def test_compare_rules():
    m = {100 + i: b"candidate-%04d" % i for i in range(300)}
    good = P.simulate(m)
    P.compare(m, good, loaded=300)
    assert _fails(m, good, loaded=299)
    # slot order is the compaction's business
    perm = np.random.default_rng(1).permutation(300)
    P.compare(m, {"count": 300, "ids": good["ids"][perm], "mid": good["mid"][:, perm], "sref": None})
    assert _fails(m, {"count": 300, "ids": good["ids"][perm], "mid": good["mid"], "sref": None})  # ids moved alone
    assert _fails(m, dict(good, count=301)) and _fails(m, dict(good, count=299))
    twice = good["ids"].copy()
    twice[5] = twice[4]
    assert _fails(m, dict(good, ids=twice))
    flipped = good["mid"].copy()
    flipped[9, 299] ^= 1
    assert _fails(m, dict(good, mid=flipped))
    assert _fails({**m, 99: b"one-more"}, good) and _fails({k: v for k, v in m.items() if k != 100}, good)
    # overflow: the counter is the model's count, the batch holds distinct ids of the model, whichever
    P.compare(m, P.simulate(m, batch=256), batch=256, loaded=256)
    late = sorted(m)[-256:]
    P.compare(m, {"count": 300, "ids": np.array(late, dtype=np.uint64), "mid": P.midstates(m[i] for i in late),
                  "sref": None}, batch=256)
    assert _fails(m, dict(P.simulate(m, batch=256), count=256), batch=256)
    assert _fails(m, P.simulate(m, batch=255), batch=256)
    # salt references
    sref = {i: i % 7 for i in m}
    P.compare(m, dict(good, sref=np.array([i % 7 for i in sorted(m)], dtype=np.uint32)), sref=sref)
    assert _fails(m, dict(good, sref=np.array([(i + 1) % 7 for i in sorted(m)], dtype=np.uint32)), sref=sref)


def test_salt_refs():
    """One entry of 1 + 2 x 16 x blocks words per ESSID in byte order; ESSID || INT(i) takes a second block from 52
    bytes on."""
    ref = P.salt_refs([b"b", b"a" * 32, b"a", b"c" * 51, b"d" * 52, b"e"])
    assert ref == {b"a": 0, b"a" * 32: 33, b"b": 66, b"c" * 51: 99, b"d" * 52: 132, b"e": 132 + 65}


# ---------------------------------------------------------------------------------------------------------------
# coverage, counted from the lists
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models():
    """{attack: [(spec, window, model)]} of the committed lists."""
    return {n: [(s, w, P.model(P.ATTACKS[n], s, w)) for s in P.specs(n) for w in s["windows"]] for n in NAMES}


def _ids(name, s, w):
    return P.ATTACKS[name].ids(s, w)


@pytest.mark.parametrize("name", NAMES)
def test_windows_fit_the_keyspace_and_the_batch(name, models):
    a = P.ATTACKS[name]
    assert len(P.specs(name)) >= 4
    for s, w, m in models[name]:
        ids = _ids(name, s, w)
        assert 1 <= len(ids) == P.raw_count(name, s, w) <= P.BATCH, (s["name"], w)
        assert 0 <= min(ids) and max(ids) < a.keyspace(s) <= P.U64, (s["name"], w)
        if not a.compacts:
            assert len(m) == len(ids)  # nothing is filtered: the counter is the count


def test_the_lists_sizes(models):
    """What the GPU tests compare, counted here: per kernel (specs, windows, raw candidates loaded, candidates kept and
    compared).  CHANGELOG.md quotes these figures."""
    sizes = {P.ATTACKS[n].kernel: (len(P.specs(n)), len(models[n]), sum(P.raw_count(n, s, w) for s, w, m in models[n]),
                                   sum(len(m) for s, w, m in models[n])) for n in NAMES}
    print("\n".join("%s %r" % kv for kv in sizes.items()))
    assert len(sizes) == 12 and all(raw >= 10000 and kept >= 3000 for _, _, raw, kept in sizes.values()), sizes
    assert sum(raw for _, _, raw, _ in sizes.values()) >= 300000


@pytest.mark.parametrize("name", NAMES)
def test_every_count_and_every_kind_of_start(name, models):
    a = P.ATTACKS[name]
    counts = {P.raw_count(name, s, w) for s, w, m in models[name]}
    assert set(P.COUNTS) <= counts, sorted(set(P.COUNTS) - counts)
    spans = [(min(_ids(name, s, w)), max(_ids(name, s, w)), a.keyspace(s)) for s, w, m in models[name]]
    assert any(lo == 0 for lo, hi, k in spans) and any(hi == k - 1 for lo, hi, k in spans)
    assert any(0 < lo and hi < k - 1 for lo, hi, k in spans)
    if name not in NO_2_32:
        assert any(lo < P.U32 <= hi for lo, hi, k in spans), "no window across 2^32"
    else:
        assert all(k < P.U32 for lo, hi, k in spans)
    if name not in NO_2_63:
        assert any(k > 2**63 for lo, hi, k in spans), "no keyspace above 2^63"
        assert any(lo > 2**63 for lo, hi, k in spans), "no window above 2^63"


@pytest.mark.parametrize("name", NAMES)
def test_duplicates_inside_a_window(name, models):
    dup = any(len(set(m.values())) < len(m) for s, w, m in models[name])
    assert dup == (name not in NO_DUPLICATES)


@pytest.mark.parametrize("name", FILTERING)
def test_lengths_at_the_filter(name, models):
    """8 and 63 bytes kept, 7 and 64 bytes dropped, and both outcomes inside one window."""
    a = P.ATTACKS[name]
    kept, dropped, mixed = set(), set(), False
    for s, w, m in models[name]:
        kept |= {len(c) for c in m.values()}
        out = [a.cand(s, i, 0, 1000) for i in _ids(name, s, w) if i not in m]
        dropped |= {len(c) for c in out if c is not None}
        mixed = mixed or (bool(m) and len(m) < len(_ids(name, s, w)))
    assert {8, 63} <= kept and min(kept) == 8 and max(kept) == 63, sorted(kept)
    assert {7, 64} <= dropped, sorted(dropped)
    assert mixed


def test_unfiltered_lengths():
    """A mask, Markov or numeric load keeps every length; the lists hold 1, 8 and 63 positions (8 and 20 digits), and
    the table list drops words of 7 and 64 bytes, and for word_max, when the table is set."""
    for name in ("mask", "markov"):
        a = P.ATTACKS[name]
        assert {1, 7, 8, 9, 10, 11, 63} <= {len(a.cand(s, 0)) for s in P.specs(name)}
    assert {s["digits"] for s in P.specs("numeric")} == set(range(8, 21))
    why = set()
    for s in P.specs("table"):
        p = P.ATTACKS["table"].plan(s)
        why |= {(len(w) if y == T.DROP_LEN else 0, y) for w, y in zip(p.words, p.why)}
        assert {len(p.words[j]) for j in p.kword} >= {8, 63} or s["name"] == "big"
    assert {(7, T.DROP_LEN), (64, T.DROP_LEN), (0, T.DROP_MAX), (0, T.KEPT)} <= why


def test_mask_lists():
    lanes, sizes, members = set(), set(), set()
    for name in ("mask", "markov"):
        for s in P.specs(name):
            sets = MK.mk_sets(s["mask"], s["custom"])
            lanes |= {p % 4 for p, x in enumerate(sets) if len(x) == 1}
            sizes |= {len(x) for x in sets}
            members |= {c for x in sets if len(x) > 1 for c in x}
    assert lanes == {0, 1, 2, 3} and {1, 2, 256} <= sizes and len(sizes) >= 12
    assert set(P.EDGE_BYTES) <= members
    ts = {(s["threshold"], max(len(x) for x in MK.mk_sets(s["mask"], s["custom"]))) for s in P.specs("markov")}
    assert any(t == 1 for t, n in ts) and any(t > n > 1 for t, n in ts) and any(1 < t < n for t, n in ts)
    assert any(t == 0 for t, n in ts)


def test_hybrid_and_combinator_sides():
    assert {s["mode"] for s in P.specs("hybrid")} == {6, 7}
    assert {s["side"] for s in P.specs("combinator")} == {P.COMBI_AMP_RIGHT, P.COMBI_AMP_LEFT}
    for name, key in (("hybrid", "mode"), ("combinator", "side")):
        for v in {s[key] for s in P.specs(name)}:  # each side across 2^32 on its own
            assert any(min(_ids(name, s, w)) < P.U32 <= max(_ids(name, s, w))
                       for s in P.specs(name) if s[key] == v for w in s["windows"]), (name, v)


@pytest.mark.parametrize("name", ["chain", "chain_rules"])
def test_chain_shapes(name):
    shapes = set()
    for s in P.specs(name):
        ch = P.ATTACKS[name].chain(s)
        shapes.add("".join("M" if x is not None else "R" if name == "chain_rules" and ch.rules[p] else "L"
                           for p, x in enumerate(ch.sets)))
        assert 1 in ch.radix or s["name"] != "ones"
    assert {len(x) for x in shapes} == {2, 3, 4}
    assert any("M" in x and ("L" in x or "R" in x) for x in shapes)
    assert any(1 in P.ATTACKS[name].chain(s).radix for s in P.specs(name))
    if name == "chain_rules":
        assert all("R" in x for x in shapes) and any(x.count("R") > 1 for x in shapes)
        assert any("L" in x and "R" in x for x in shapes)


def test_rules_reject():
    """The rule lists hold rejecting and memory functions, and some candidate is dropped by a rule, not for its length."""
    from oracle import rules as OR
    for name in ("rules", "assoc_rules"):
        a = P.ATTACKS[name]
        lines = [r for s in P.specs(name) for r in s["rules"]]
        assert any(not OR.hashcat_loads(r) for r in lines)
        assert any(a.cand(s, i, 0, 1000) is None for s in P.specs(name) for w in s["windows"][:2]
                   for i in list(_ids(name, s, w))[:400])
    ruled = [p[1] for s in P.specs("chain_rules") for p in s["parts"] if isinstance(p, tuple)]
    assert any(not OR.hashcat_loads(r) for rs in ruled for r in rs)


def test_table_lists():
    sizes, own = set(), False
    for s in P.specs("table"):
        p = P.ATTACKS["table"].plan(s)
        sizes |= {len(a) for a in p.alt}
        own = own or any(len(a) > 1 and c in a for c, a in enumerate(p.alt))
        # a window that starts inside a word
        assert any(w[0] not in p.start for w in s["windows"])
    assert {1, 2, 3, 5, 8, 16} <= sizes and own


@pytest.mark.parametrize("name", ["assoc_plain", "assoc_rules"])
def test_assoc_lists(name):
    sizes = set()
    for s in P.specs(name):
        p = P.ATTACKS[name].plan(s)
        sizes |= {len(ws) for ws in p.words}
        assert any(w[0] not in p.start for w in s["windows"])  # a window that starts inside a net
        assert len({e for e, m in s["nets"]}) < len(s["nets"])  # two nets under one ESSID
    assert {0, 1} <= sizes and max(sizes) > 1000
    assert all((s["rules"] is not None) == (name == "assoc_rules") for s in P.specs(name))


def test_dictionary_offsets():
    for name, key in (("dict", "words"), ("rules", "words"), ("hybrid", "words"), ("combinator", "base"),
                      ("combinator", "amp")):
        for s in P.specs(name):
            if s["name"] in ("all-kept", "wide", "wide-right", "wide-left") or s["name"].startswith("top"):
                continue
            off, pairs = 0, set()
            for w in s[key]:
                if 1 <= len(w) <= 63:
                    pairs.add((len(w) % 4, off % 4))
                off += len(w)
            assert len(pairs) == 16, (name, s["name"])
    assert {len(w) for s in P.specs("dict") for w in s["words"]} >= set(range(71))


# ---------------------------------------------------------------------------------------------------------------
# teeth
# ---------------------------------------------------------------------------------------------------------------
# where a slip cannot change anything: ids below 2^32; an id that is no numeral; loads that filter no length
# (and without rules a net's numeral has one digit: nothing to reverse)
BLIND = {"first32": set(NO_2_32), "reversed": {"dict", "assoc_plain"}, "radix": {"dict"},
         "maxlen64": {"mask", "markov", "numeric", "table"}, "lastbyte": set()}


@pytest.mark.parametrize("slip", P.SLIPS)
@pytest.mark.parametrize("name", NAMES)
def test_a_wrong_model_is_caught(name, slip, models):
    """A generator with the slip (its batch simulated from the wrong model) fails compare() against the right model on
    some window of the attack's list."""
    a = P.ATTACKS[name]
    caught = any(_fails(m, P.simulate(P.model(a, s, w, slip))) for s, w, m in models[name])
    assert caught == (name not in BLIND[slip]), (name, slip)


def test_no_list_passes_a_slip_it_could_see():
    assert all(len(BLIND[slip]) < len(NAMES) for slip in P.SLIPS)
    assert all(sum(name not in BLIND[slip] for slip in P.SLIPS) >= 2 for name in NAMES)


# ---------------------------------------------------------------------------------------------------------------
# the hook
# ---------------------------------------------------------------------------------------------------------------
def test_the_hook_is_outside_the_abi():
    """dwpa_debug_scan_prepared: exported, outside the public header, the PHP cdef and the ABI version, and
    DWPA_E_ARG for null arguments before anything touches a device."""
    import ctypes
    import os
    from dwpa_amd import _lib as L
    lib = L.load()
    hook = "dwpa_debug_scan_prepared"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    php = open(os.path.join(root, "php", "dwpa22000.php")).read()
    assert hasattr(lib, hook) and hook in L.SIGNATURES
    assert hook not in open(L.HEADER).read() and hook not in php
    assert lib.dwpa_abi_version() == 4
    ids, mid, n = (ctypes.c_uint64 * 4)(), (ctypes.c_uint32 * 40)(), ctypes.c_uint32(7)
    fake = ctypes.c_void_p(1)  # never dereferenced: a null argument is refused first
    for scan, i, m, c in ((None, ids, mid, ctypes.byref(n)), (fake, None, mid, ctypes.byref(n)),
                          (fake, ids, None, ctypes.byref(n)), (fake, ids, mid, None)):
        assert lib.dwpa_debug_scan_prepared(scan, i, m, 4, c, None, None) == L.DWPA_E_ARG
    assert n.value == 7
