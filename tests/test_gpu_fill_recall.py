"""GPU recall across the crack loop's load sizing.

dwpa_crack_files, dwpa_crack_hybrid and dwpa_crack_combinator size every device load from a running estimate of the
kept share (scan_shard, csrc/crack.cpp): a load that keeps more than a batch is repeated with fewer words before
anything is derived, one that keeps nothing is skipped, and a hit's id is mapped back to its word after either.  The
recall tests below this loop pin the kernels; the crack tests above it run one or two loads with a kept share that
never moves.  Here the fixtures of tests/fill_plan.py swing the share (tests/test_fill_plan.py proves on the CPU that
they reach the overflow path for every plausible cut into items), every kept candidate is the PSK of one PMKID line,
and each case asserts rc 1, exactly the planned records, dwpa_crack_stats.candidates equal to the model's kept
candidates -- a repeated load must not count twice, a dropped one must not be missing -- and, from the library's
dwpa_debug_crack_loads hook, that the path in question was taken.

Each case prints its hook counts and its time (pytest -s shows them).
"""
import gzip
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

import dwpa_amd  # noqa: E402
from dwpa_amd import _lib as L  # noqa: E402
from dwpa_amd import m22000 as M  # noqa: E402
from tests import fill_plan as P  # noqa: E402
from tests import test_gpu_recall as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC = P.NC


@pytest.fixture(autouse=True)
def _one_worker(monkeypatch):
    monkeypatch.delenv("DWPA_CRACK_SHARDS_PER_DEVICE", raising=False)


def _write_words(path, words):
    path.write_bytes(b"".join(w + b"\n" for w in words))
    return path


def _read_records(out):
    recs = out.read_bytes().split(b"\n") if out.exists() else [b""]
    assert recs.pop() == b""
    return recs


def _assert_records(recs, lines, psks, what):
    """Exactly the planned records, each once: every line but the last (whose PSK is no candidate) with its PSK."""
    assert len(lines) == len(psks) + 1
    exp = R._records(lines[:-1], psks)
    assert len(set(recs)) == len(recs), (what, "a record was written twice")
    missing, extra = set(exp) - set(recs), set(recs) - set(exp)
    assert not missing and not extra, (what, "missing %d of %d" % (len(missing), len(exp)), sorted(missing)[:3],
                                       "extra %d" % len(extra), sorted(extra)[:3])


def _run(tmp_path, what, lines, psks, nwords, ncands, call):
    """One call of a product entry point: call(hash file, outfile) -> rc.  Returns the hook's counts."""
    hf, out = tmp_path / "h.hash", tmp_path / "o.key"
    hf.write_bytes(b"\n".join(lines) + b"\n")
    L.pbkdf2_kernels(reset=True)
    L.crack_loads(reset=True)
    t = time.monotonic()
    rc = call(str(hf), str(out))
    took = time.monotonic() - t
    loads, ran = L.crack_loads(), L.pbkdf2_kernels()
    st = M.crack_stats()
    print("FILL %s: rc %d, %s, candidates %d of %d, %.2f s" % (what, rc, loads, st["candidates"], ncands, took))
    _assert_records(_read_records(out), lines, psks, what)
    assert rc == 1, what
    assert (st["cracked"], st["hashes"]) == (len(psks), len(psks) + 1), (what, st)
    assert st["words"] == nwords, (what, st["words"], nwords)
    assert st["candidates"] == ncands, (what, st["candidates"], ncands)
    ws = M.crack_worker_stats()
    assert len(ws) == 1 and ws[0]["candidates"] == ncands and ws[0]["words"] == nwords, (what, ws)
    assert ran and ran <= R.MG_KERNELS, (what, ran)
    assert loads["loads"] == loads["overflowed"] + loads["empty"] + loads["scanned"], (what, loads)
    return loads


def _files(d, batch, rules=None):
    kw = {"rule_mode": L.DWPA_RULES_FULL} if rules else {}
    return lambda hf, out: dwpa_amd.crack_files(hf, [str(d)], rules and str(rules), NC, out, device_mask=1,
                                                batch=batch, nc_mode=L.DWPA_NC_HASHCAT, **kw)


# ---------------------------------------------------------------------------------------------------------------
# a, b, h: the dictionary path
# ---------------------------------------------------------------------------------------------------------------
def _swing_gz(f, path):
    """The swing dictionary as a .gz with CRLF endings in its first half and three $HEX[] entries."""
    words = list(f["words"])
    kept = [i for i, k in enumerate(f["kept_per_word"]) if k]
    for i in (kept[0], kept[len(kept) // 2], kept[-1]):
        words[i] = b"$HEX[" + words[i].hex().encode() + b"]"
    half = len(words) // 2
    with gzip.open(path, "wb") as g:
        g.write(b"".join(w + b"\r\n" for w in words[:half]) + b"".join(w + b"\n" for w in words[half:]))
    return path


@pytest.mark.parametrize("batch,form", [(64, "plain"), (256, "plain"), (64, "gz")])
def test_swing(tmp_path, batch, form):
    """a. A kept share that swings between 1/8 and 1, then an all-junk tail: a dense stretch right after a sparse one
    overflows the load sized for the sparse one (repeated with fewer words), the tail's loads keep nothing; every kept
    word is found and counted once.  Also as a .gz with CRLF endings and $HEX[] entries."""
    f = P.swing()
    d = _swing_gz(f, tmp_path / "d.txt.gz") if form == "gz" else _write_words(tmp_path / "d.txt", f["words"])
    loads = _run(tmp_path, "swing/%d/%s" % (batch, form), f["lines"], f["psk"], len(f["words"]), f["candidates"],
                 _files(d, batch))
    assert loads["overflowed"] >= 1 and loads["empty"] >= 1, loads


def test_all_kept(tmp_path):
    """b. 5 x 64 + 1 words, nothing filtered, batch 64: the estimate stays 1, every load is exactly a batch and none
    overflows."""
    f = P.all_kept()
    d = _write_words(tmp_path / "d.txt", f["words"])
    loads = _run(tmp_path, "all_kept/64", f["lines"], f["psk"], len(f["words"]), f["candidates"], _files(d, 64))
    assert loads["overflowed"] == 0 and loads["empty"] == 0 and loads["scanned"] >= 6, loads


_SHARDS_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import dwpa_amd
from dwpa_amd import _lib as L
from dwpa_amd import m22000 as M
rc = dwpa_amd.crack_files(sys.argv[2], [sys.argv[4]], None, int(sys.argv[5]), sys.argv[3], device_mask=1, batch=64,
                          nc_mode=L.DWPA_NC_HASHCAT)
print(json.dumps({"rc": rc, "stats": M.crack_stats(), "workers": M.crack_worker_stats(), "loads": L.crack_loads()}))
"""


def test_swing_two_workers(tmp_path):
    """h. The swing dictionary with DWPA_CRACK_SHARDS_PER_DEVICE=2 (read per call; a child keeps this process's
    environment as it is): each worker carries its own estimate over the items it happens to take.  Every record
    once, rc 1, and the two workers' candidates sum to the kept words."""
    f = P.swing()
    hf, out = tmp_path / "h.hash", tmp_path / "o.key"
    hf.write_bytes(b"\n".join(f["lines"]) + b"\n")
    d = _write_words(tmp_path / "d.txt", f["words"])
    env = dict(os.environ, DWPA_CRACK_SHARDS_PER_DEVICE="2")
    r = subprocess.run([sys.executable, "-c", _SHARDS_CHILD, ROOT, str(hf), str(out), str(d), str(NC)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print("FILL swing/64/two workers: %s, %.2f s" % (res["loads"], res["stats"]["seconds"]))
    _assert_records(_read_records(out), f["lines"], f["psk"], "two workers")
    assert res["rc"] == 1
    assert len(res["workers"]) == 2 and len({w["device"] for w in res["workers"]}) == 1
    assert sum(w["candidates"] for w in res["workers"]) == res["stats"]["candidates"] == f["candidates"]


# ---------------------------------------------------------------------------------------------------------------
# c, g: the rules path
# ---------------------------------------------------------------------------------------------------------------
def test_rules_swing(tmp_path):
    """c. Eight rules that reject, shorten, lengthen and collide over runs of words that keep almost nothing and runs
    that keep almost everything, batch 64: every distinct kept result is found, candidates = the oracle's kept (word,
    rule) pairs, and at least one load overflowed and was repeated."""
    f = P.rules_swing()
    d = _write_words(tmp_path / "d.txt", f["words"])
    rf = tmp_path / "r.rule"
    rf.write_text("\n".join(f["rules"]) + "\n")
    loads = _run(tmp_path, "rules_swing/64", f["lines"], f["psk"], len(f["words"]), f["candidates"],
                 _files(d, 64, rf))
    assert M.crack_stats()["rules"] == len(f["rules"]) == 8
    assert loads["overflowed"] >= 1, loads


@pytest.mark.parametrize("nrules", [64, 65, 1025])
def test_rules_wide(tmp_path, nrules):
    """g. A rules file of exactly a batch of rules, of one more, and of 16 batches + 1, at batch 64: every plant is
    found and candidates = 6 words x nrules.  With more rules than the batch one word's results no longer fit a load:
    the sizing loop alone returned DWPA_E_OVERFLOW at 65 rules (rc -1, nothing cracked) and rules_load refused every
    load at 1,025 (DWPA_E_ARG); the library now goes one word at a time over rule ranges of a batch, which the hook
    does not count."""
    f = P.rules_wide(nrules)
    d = _write_words(tmp_path / "d.txt", f["words"])
    rf = tmp_path / "r.rule"
    rf.write_text("\n".join(f["rules"]) + "\n")
    loads = _run(tmp_path, "rules_wide/%d" % nrules, f["lines"], f["psk"], 6, 6 * nrules, _files(d, 64, rf))
    assert M.crack_stats()["rules"] == nrules
    exp = {"loads": 6, "overflowed": 0, "empty": 0, "scanned": 6} if nrules == 64 else dict.fromkeys(loads, 0)
    assert loads == exp, loads


# ---------------------------------------------------------------------------------------------------------------
# d, e: the hybrid path
# ---------------------------------------------------------------------------------------------------------------
def _hybrid(d, f, mode):
    def call(hf, out):
        rc, st = dwpa_amd.crack_hybrid(hf, [str(d)], f["mask"], f["custom"], mode, NC, out, device_mask=1, batch=64,
                                       nc_mode=L.DWPA_NC_HASHCAT)
        assert st == [L.DWPA_DICT_OK]
        return rc
    return call


@pytest.mark.parametrize("mode", [6, 7])
def test_hybrid_narrow(tmp_path, mode):
    """d. ?d (K = 10) at batch 64 over runs of words whose lengths the join drops and runs it keeps: every kept word x
    every digit is found, and at least one load overflowed and was repeated."""
    f = P.hybrid_narrow()
    d = _write_words(tmp_path / "d.txt", f["words"])
    loads = _run(tmp_path, "hybrid_narrow/%d" % mode, f[mode]["lines"], f[mode]["psk"], len(f["words"]),
                 f["candidates"], _hybrid(d, f, mode))
    assert loads["overflowed"] >= 1, loads


@pytest.mark.parametrize("mode", [6, 7])
@pytest.mark.parametrize("K", [64, 65])
def test_hybrid_edge(tmp_path, K, mode):
    """e. A mask of exactly the batch (K = 64: the sizing loop, one word per load) and of one more (K = 65: one word x
    mask ranges, which the hook does not count): plants at mask indices 0, 63 and K - 1 of three kept words among
    dropped ones, candidates = 3 x K."""
    f = P.hybrid_edge(K)
    d = _write_words(tmp_path / "d.txt", f["words"])
    loads = _run(tmp_path, "hybrid_edge/%d/%d" % (K, mode), f[mode]["lines"], f[mode]["psk"], len(f["words"]), 3 * K,
                 _hybrid(d, f, mode))
    n = len(f["words"])
    exp = {"loads": n, "overflowed": 0, "empty": n - 3, "scanned": 3} if K == 64 else dict.fromkeys(loads, 0)
    assert loads == exp, loads


# ---------------------------------------------------------------------------------------------------------------
# f: the combinator path
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [L.DWPA_COMBI_AMP_RIGHT, L.DWPA_COMBI_AMP_LEFT])
@pytest.mark.parametrize("A", [64, 63])
def test_combi_edge(tmp_path, A, side):
    """f. An amplifier of exactly the batch and of one less, either list as the amplifier: the loop sizes from the
    lengths, its running sum lands on exactly 64 and stops before 65, and its guard on the kernel's own count stays
    silent.  It has no adaptive state, so the loads are the model's exactly: none overflows, the scanned and the
    empty ones are counted."""
    f = P.combi_edge(A, side)
    base = _write_words(tmp_path / "base.txt", f["words"])
    amp = _write_words(tmp_path / "amp.txt", f["amp"])
    left, right = (amp, base) if side == L.DWPA_COMBI_AMP_LEFT else (base, amp)

    def call(hf, out):
        rc, st = dwpa_amd.crack_combinator(hf, str(left), str(right), side, NC, out, device_mask=1, batch=64,
                                           nc_mode=L.DWPA_NC_HASHCAT)
        assert st == [L.DWPA_DICT_OK] * 2
        return rc
    loads = _run(tmp_path, "combi_edge/%d/%d" % (A, side), f["lines"], f["psk"], len(f["words"]), f["candidates"],
                 call)
    model = f["loads"]
    exp = {"loads": len(model), "overflowed": 0, "empty": sum(1 for _, _, k in model if k == 0),
           "scanned": sum(1 for _, _, k in model if k)}
    assert loads == exp, (loads, exp)
