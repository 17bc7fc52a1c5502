"""GPU recall across the hashcat nonce window: every attempt of a DWPA_NC_HASHCAT scan must be found.

Every dwpa_crack_* entry point and the benchmark's headline line verify in hashcat nonce mode: the stored ANONCE,
then +-1..+-N in little and big endian, cut down by the line's message-pair bits.  The other scan tests that assert
the (nc, endian) of a hit run PHP's order with a handful of offsets.  Here the plans of tests/nonce_plan.py plant a
hit at every attempt index of the 33- and the 65-attempt window (the latter one past ATT_PARALLEL_MIN: scans verify
key-parallel at any length), at the ends and the 64-attempt marks of the 257-attempt one, at every index of the 1- and
5-attempt ones, at and one past the window's edge, under every message-pair mask, over stored tails that carry, wrap
or make two attempts one value, and in lines with a short ANONCE -- for keyver 1, 2 and 3 and both nonce orders, which
decide the words and blocks of the PRF message an attempt patches.  The hits of a scan must be exactly the plan's
(line, cand, nc, endian, pmk): none missing, none extra, none twice; the model and the C oracle decided them.

Each pass asserts the verify kernels that ran (the library's dwpa_debug_verify_kernels hook): the key-parallel
k_verify of the classes present and no k_verify_att.
"""
import time

import pytest

pytestmark = pytest.mark.gpu

import dwpa_amd  # noqa: E402
from dwpa_amd import _lib as L  # noqa: E402
from dwpa_amd import m22000 as M  # noqa: E402
from dwpa_amd.device import Dictionary  # noqa: E402
from tests import nonce_plan as N  # noqa: E402

BATCH = 256  # which PBKDF2 kernel derives is not the subject here


def expected_kernels(p):
    """scan_verify / scan_run launch one key-parallel kernel per verify class present: PMKID, keyver 1, 2, 3."""
    out = {"k_verify<pmkid>"} | {"k_verify<kv%d>" % kv for kv in p["classes"]}
    assert out <= set(L.VERIFY_KERNEL_NAMES) and not any(n.startswith("k_verify_att") for n in out)
    return out


@pytest.fixture(scope="module")
def dictionary():
    assert dwpa_amd.device_count() >= 1
    return Dictionary.from_words(N.dictionary()["words"])


def _hitset(hits):
    got = [(h["line"], h["cand"], h["nc"], h["endian"], h["pmk"]) for h in hits]
    assert len(set(got)) == len(got), "a hit was reported twice"
    return set(got)


def _pass(sc, d, p, count, nkept, mode):
    """One load of the dictionary's first `count` words and one scan; the hits must be the plan's for those words."""
    L.verify_kernels(reset=True)
    sc.load_dict(d.off.ptr, d.data.ptr, 0, count)
    assert sc.loaded() == nkept
    if mode == "run":
        sc.run()
    else:
        for g in range(sc.groups):
            sc.pbkdf2(g)
            sc.verify(g)
    got = _hitset(sc.hits(cap=4096))
    assert got == N.hits_within(p, nkept), (mode,) + N.describe(dict(p, hits=N.hits_within(p, nkept)), got)
    assert L.verify_kernels() == expected_kernels(p), mode


@pytest.mark.parametrize("name", N.PLANS)
def test_every_planted_attempt_is_found(dictionary, name):
    """One Scan per plan: the 130 kept words loaded, once through pbkdf2(g) / verify(g) per ESSID group, and after a
    fresh load once through run(), a multi-group launch of both ESSIDs."""
    p = N.plan(name)
    t = time.perf_counter()
    sc = dwpa_amd.Scan(p["lines"], nc=p["nec"], nc_mode=L.DWPA_NC_HASHCAT, batch=BATCH)
    try:
        assert sc.groups == 2
        for mode in ("per_group", "run"):
            _pass(sc, dictionary, p, len(p["words"]), 130, mode)
    finally:
        sc.close()
    print("%s: %d lines, %d hits, nec %d: %.3f s" % (name, len(p["lines"]), len(p["hits"]), p["nec"],
                                                    time.perf_counter() - t))


@pytest.mark.parametrize("mode", ["per_group", "run"])
def test_early_wave_alone(dictionary, mode):
    """every_8 with the first 64 kept words only, in a fresh Scan (no PMK of an earlier load can stand in): the rows
    whose PSK is kept word 0 or 63 are found, those of words 64, 127, 128 and 129 are absent."""
    p = N.plan("every_8")
    early = N.hits_within(p, 64)
    assert len(early) == sum(1 for r in p["rows"] if r["pos"] in (0, 63)) + 1 and 60 < len(early) < 80
    sc = dwpa_amd.Scan(p["lines"], nc=p["nec"], nc_mode=L.DWPA_NC_HASHCAT, batch=BATCH)
    try:
        _pass(sc, dictionary, p, p["kept"][63] + 1, 64, mode)
    finally:
        sc.close()


def test_crack_files_edges_and_message_pairs(tmp_path):
    """dwpa_crack_files (hashcat nonce mode is its default) at nonce_error_corrections = 8 over the lines of edges_8,
    edges_16 and message_pair, the dictionary as a file: the outfile holds exactly the rows the model finds at +-8 and
    the PMKID controls, each once; rc 1, because the misses stay."""
    lines, psks, want = [], [], []
    for name in ("edges_8", "edges_16", "message_pair"):
        p = N.plan(name)
        found = set(N.model_hits(p["rows"], 8))
        for i, r in enumerate(p["rows"]):
            lines.append(r["line"])
            psks.append(r["psk"])
            want.append(i in found)
        for k, pos in p["controls"]:
            lines.append(p["lines"][k])
            psks.append(p["words"][p["kept"][pos]])
            want.append(True)
    assert len(set(lines)) == len(lines) and 0 < sum(want) < len(want)
    exp = [N.record(ln, psk) for ln, psk, w in zip(lines, psks, want) if w]
    assert len(set(exp)) == len(exp)
    hf, out, df = tmp_path / "h.hash", tmp_path / "o.key", tmp_path / "d.txt"
    hf.write_bytes(b"\n".join(lines) + b"\n")
    df.write_bytes(b"".join(w + b"\n" for w in N.dictionary()["words"]))
    L.verify_kernels(reset=True)
    rc = dwpa_amd.crack_files(str(hf), [str(df)], None, nonce_error_corrections=8, out_file=str(out), batch=BATCH)
    ran = L.verify_kernels()
    recs = out.read_bytes().split(b"\n")
    assert recs.pop() == b""
    assert len(set(recs)) == len(recs), "a record was written twice"
    missing, extra = set(exp) - set(recs), set(recs) - set(exp)
    assert not missing and not extra, ("missing %d" % len(missing), sorted(missing)[:3], "extra %d" % len(extra),
                                       sorted(extra)[:3])
    assert rc == 1
    assert M.crack_stats()["cracked"] == len(exp)
    assert ran == {"k_verify<pmkid>", "k_verify<kv1>", "k_verify<kv2>", "k_verify<kv3>"}
