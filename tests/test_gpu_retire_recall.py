"""GPU recall across retirement, multi-launch runs and launch dimensions that come from the data.

The scan-path recall tests plant every candidate slot of ONE launch.  Between the launches of a crack run the library
retires what is cracked (scan_mark_cracked, then scan_mg_rebuild: the active ESSID groups, their spread over the
PBKDF2 launches, the per-class line lists, every line's PMK offset), and a mistake there loses genuine cracks in
silence.  The plans of tests/retire_plan.py walk one run through chosen retirement patterns; here the run's records
must be exactly the planned ones, each once, and -- with one worker -- the scan-work counters of the library's
dwpa_debug_scan_work hook must equal the plan's model: a retirement that never happens, or happens too little, cracks
everything all the same and shows only there.

The last two tests put more than 65,535 into a launch's grid.y: lines of one class of one ESSID group (scan_verify
passes the run's length on, scan_run cuts it into launches of 65,535), and rules (launch_rules_prep and
launch_rules_expand pass the rule count on).
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
from dwpa_amd import m22000 as M  # noqa: E402
from dwpa_amd.device import Dictionary  # noqa: E402
from oracle import oracle as O  # noqa: E402
from oracle import rules as OR  # noqa: E402
from tests import retire_plan as P  # noqa: E402
from tests import synth as S  # noqa: E402
from tests import test_gpu_recall as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC = P.NC


@pytest.fixture(autouse=True)
def _one_worker(monkeypatch):
    monkeypatch.delenv("DWPA_CRACK_SHARDS_PER_DEVICE", raising=False)


def _write_hashes(tmp_path, p):
    hf = tmp_path / "h.hash"
    hf.write_bytes(b"\n".join(p["lines"]) + b"\n")
    return hf, tmp_path / "o.key"


def _read_records(out):
    recs = out.read_bytes().split(b"\n")
    assert recs.pop() == b""
    return recs


def _assert_records(recs, p, in_order):
    """Exactly the planned records, each once; in_order: written in the order of their scheduled batches."""
    assert len(set(recs)) == len(recs), "a record was written twice"
    missing, extra = set(p["records"]) - set(recs), set(recs) - set(p["records"])
    assert not missing and not extra, (p["name"], "missing %d" % len(missing),
                                       sorted((p["record_batch"][r], r) for r in missing)[:4],
                                       "extra %d" % len(extra), sorted(extra)[:4])
    if in_order:
        at = [p["record_batch"][r] for r in recs]
        assert at == sorted(at), at


# ---------------------------------------------------------------------------------------------------------------
# a-d: plan A, one launch per batch
# ---------------------------------------------------------------------------------------------------------------
def test_plan_a_crack_mask(tmp_path):
    """a. Plan A through dwpa_crack_mask at batch 64: 16 batches, eight ESSID groups that retire front to back, back
    to front, inside out, a class at once, all at once in the first and in the last batch, a single line, and one
    that never finishes.  rc 1, the records, their order, the stats, and the three counters equal to the model."""
    p = P.plan("A")
    hf, out = _write_hashes(tmp_path, p)
    L.pbkdf2_kernels(reset=True)
    L.scan_work(reset=True)
    rc = dwpa_amd.crack_mask(str(hf), p["mask"], p["custom"], nonce_error_corrections=NC, out_file=str(out),
                             device_mask=1, batch=p["batch_size"])
    work, ran = L.scan_work(), L.pbkdf2_kernels()
    _assert_records(_read_records(out), p, in_order=True)
    assert rc == 1
    st = M.crack_stats()
    assert (st["cracked"], st["hashes"], st["candidates"]) == (p["crackable"], p["crackable"] + 1, 1024)
    ws = M.crack_worker_stats()
    assert len(ws) == 1 and ws[0]["items"] == p["nbatches"] == 16
    assert work == p["work"], (work, p["work"])
    assert ran and ran <= R.MG_KERNELS, ran


def test_plan_a_crack_files(tmp_path):
    """b. Plan A's lines through dwpa_crack_files: the 1,024 numerals in index order as a dictionary, a word outside
    the 8..63 filter between every two of them, batch 64, no rules.  The same records and rc.  The guided queue cuts
    the items, so the counters are not the model's; but with eight groups every scan makes exactly one PBKDF2 launch,
    so the launch counter IS the number of scans, and the groups derived must stay strictly below scans x the groups
    at the start: the sorted-first group leaves after the first batch."""
    p = P.plan("A")
    hf, out = _write_hashes(tmp_path, p)
    words = []
    for i in range(1024):
        words.append(P.a_candidate(i))
        words.append(b"j" * R.JUNK_LENGTHS[i % len(R.JUNK_LENGTHS)])
    assert {len(w) for w in words[1::2]} == set(R.JUNK_LENGTHS) and not any(8 <= len(w) <= 63 for w in words[1::2])
    d = tmp_path / "d.txt"
    d.write_bytes(b"".join(w + b"\n" for w in words))
    L.pbkdf2_kernels(reset=True)
    L.scan_work(reset=True)
    rc = dwpa_amd.crack_files(str(hf), [str(d)], None, NC, str(out), device_mask=1, batch=p["batch_size"],
                              nc_mode=L.DWPA_NC_HASHCAT)
    work, ran = L.scan_work(), L.pbkdf2_kernels()
    _assert_records(_read_records(out), p, in_order=False)
    assert rc == 1 and M.crack_stats()["cracked"] == p["crackable"]
    scans, at_start = work["pbkdf2_launches"], p["active"][0]
    assert at_start == 8 and scans >= p["nbatches"]
    assert work["groups_derived"] < scans * at_start, work
    assert work["line_rows"] < scans * p["uncracked"][0], work
    assert ran and ran <= R.MG_KERNELS, ran


_SHARDS_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import dwpa_amd
from dwpa_amd import m22000 as M
rc = dwpa_amd.crack_mask(sys.argv[2], "?1" * 10, (b"01",), nonce_error_corrections=int(sys.argv[4]),
                         out_file=sys.argv[3], device_mask=1, batch=64)
print(json.dumps({"rc": rc, "stats": M.crack_stats(), "workers": M.crack_worker_stats()}))
"""


def test_plan_a_two_workers(tmp_path):
    """d. Plan A through dwpa_crack_mask with DWPA_CRACK_SHARDS_PER_DEVICE=2 (read per call; a child keeps this
    process's environment as it is): a line cracked by one worker is retired on the other with a lag, so no counter
    is compared; every record once, rc 1, and the workers' candidates sum to the keyspace."""
    p = P.plan("A")
    assert (p["mask"], p["custom"], p["batch_size"]) == (b"?1" * 10, (b"01",), 64)
    hf, out = _write_hashes(tmp_path, p)
    env = dict(os.environ, DWPA_CRACK_SHARDS_PER_DEVICE="2")
    r = subprocess.run([sys.executable, "-c", _SHARDS_CHILD, ROOT, str(hf), str(out), str(NC)], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    _assert_records(_read_records(out), p, in_order=False)
    assert res["rc"] == 1
    assert len(res["workers"]) == 2 and len({w["device"] for w in res["workers"]}) == 1
    assert sum(w["candidates"] for w in res["workers"]) == res["stats"]["candidates"] == 1024
    assert res["stats"]["cracked"] == p["crackable"]


# ---------------------------------------------------------------------------------------------------------------
# c: plan B, launches that merge
# ---------------------------------------------------------------------------------------------------------------
def test_plan_b_crack_chain(tmp_path):
    """c. Plan B through dwpa_crack_chain with one worker: the chain [4,096 words, 2,048 words] at batch 2^20 keeps
    1,536 of every 2^20 raw candidates; 40 ESSID groups need 3 PBKDF2 launches (16 groups x 2^20 slots fill one), and
    as groups retire the active count goes 40, 33, 32, 17, 16, 15, 1, 1: launches of 14/13/13, 11/11/11, 16/16, 9/8,
    then one.  14 launches in all: a change of MG_SLOTS fails here instead of moving the run onto one launch."""
    p = P.plan("B")
    hf, out = _write_hashes(tmp_path, p)
    paths = []
    for name, ws in zip("ab", p["chain"]):
        paths.append(tmp_path / (name + ".txt"))
        paths[-1].write_bytes(b"".join(w + b"\n" for w in ws))
    L.pbkdf2_kernels(reset=True)
    L.scan_work(reset=True)
    rc, status = dwpa_amd.crack_chain(str(hf), [(L.DWPA_CHAIN_LIST, str(x)) for x in paths],
                                      nonce_error_corrections=NC, out_file=str(out), device_mask=1,
                                      batch=p["batch_size"])
    work, ran = L.scan_work(), L.pbkdf2_kernels()
    assert status == [L.DWPA_DICT_OK] * 2
    _assert_records(_read_records(out), p, in_order=True)
    assert rc == 1
    st = M.crack_stats()
    assert st["candidates"] == 8 * 1536 == p["nbatches"] * p["kept_per_batch"]
    assert (st["cracked"], st["hashes"]) == (p["crackable"], p["crackable"] + 1)
    assert work == p["work"] and work["pbkdf2_launches"] == 14, (work, p["work"])
    assert ran and ran <= R.MG_KERNELS, ran


# ---------------------------------------------------------------------------------------------------------------
# e: more than 65,535 lines of one class in one ESSID group
# ---------------------------------------------------------------------------------------------------------------
E_LINES = 65540
E_PLANTS = (0, 65534, 65535, 65536, 65539)  # positions inside the PMKID class, both sides of 65,535 and the last


@pytest.fixture(scope="module")
def many_lines():
    rng = random.Random(0xE65535)
    essid, psk = b"retire-many-lines", b"the-one-psk-of-65540"
    pmk = O.c_pbkdf2(psk, essid)
    lines = []
    for k in range(E_LINES):
        ap, sta = rng.randbytes(6), rng.randbytes(6)
        if k in E_PLANTS:
            lines.append(S.pmkid_line(psk, essid, ap, sta, the_pmk=pmk))
        else:  # 16 random bytes for a PMKID: no PBKDF2 and no HMAC on the CPU
            lines.append(b"WPA*01*%s*%s*%s*%s***" % (rng.randbytes(16).hex().encode(), ap.hex().encode(),
                                                     sta.hex().encode(), essid.hex().encode()))
    for kv in (1, 2, 3):  # three EAPOL lines behind them; keyver 2 is the PSK's, the other two some other PMK's
        lines.append(R._line(kv, -3, "BE", psk, essid, pmk if kv == 2 else rng.randbytes(32), rng))
    assert len(set(lines)) == len(lines) == E_LINES + 3
    words = [b"wrong-word-0", psk, b"wrong-word-2"]
    exp = set()
    for k in E_PLANTS + (E_LINES + 1,):
        o = O.c_check_key_m22000(lines[k], words, False, NC)
        assert o and o[0] == psk and o[3] == pmk, k
        exp.add((k, 1, o[1], o[2], pmk))
    assert (E_LINES + 1, 1, -3, "BE", pmk) in exp and len(exp) == 6
    for k in (1, 65533, E_LINES, E_LINES + 2):
        assert O.c_check_key_m22000(lines[k], words, False, NC) is False, k
    return {"lines": lines, "words": words, "exp": exp}


@pytest.mark.parametrize("mode", ["per_group", "run"])
def test_more_than_65535_lines_of_one_class(many_lines, mode):
    """e. 65,540 PMKID lines under one ESSID, the PSK's PMKID at class positions 0, 65,534, 65,535, 65,536 and 65,539,
    and three EAPOL lines behind them, one planted.  pbkdf2(0) + verify(0) puts the whole PMKID run into one launch's
    grid.y; run() cuts it at 65,535.  Both report exactly the six plants, and verify 65,543 line rows."""
    f = many_lines
    d = Dictionary.from_words(f["words"])
    L.scan_work(reset=True)
    sc = dwpa_amd.Scan(f["lines"], nc=NC, batch=64)
    try:
        assert sc.groups == 1
        sc.load_dict(d.off.ptr, d.data.ptr, 0, 3)
        assert sc.loaded() == 3
        R._scan_all(sc, mode)
        R._assert_same(R._hitset(sc.hits(cap=256)), f["exp"], mode)
    finally:
        sc.close()
    assert L.scan_work() == {"groups_derived": 1, "pbkdf2_launches": int(mode == "run"), "line_rows": E_LINES + 3}


# ---------------------------------------------------------------------------------------------------------------
# f: more than 65,535 rules
# ---------------------------------------------------------------------------------------------------------------
F_RULES = 70000
F_PLANTS = (0, 1, 65534, 65535, 65536, 65537, 69999)
F_WORDS = (b"rulew", b"rulewo", b"rulewor")  # 5, 6 and 7 bytes: every candidate is 8, 9 or 10 bytes and kept
_AL = b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz"


def _suffix(r):
    return bytes((_AL[r // 3844], _AL[r // 62 % 62], _AL[r % 62]))


@pytest.fixture(scope="module")
def many_rules():
    rng = random.Random(0xF65535)
    assert len(set(_AL)) == 62 and 62 ** 3 >= F_RULES
    rules = ["$%c $%c $%c" % tuple(_suffix(r)) for r in range(F_RULES)]
    assert len(set(rules)) == F_RULES and OR.apply(OR.parse(rules[65536]), b"w") == b"w" + _suffix(65536)
    essid = b"retire-many-rules"
    plants = [(w, r) for w in range(len(F_WORDS)) for r in F_PLANTS]
    psks = [F_WORDS[w] + _suffix(r) for w, r in plants]
    assert len(set(psks)) == len(psks) == 21
    raw = O.c_pbkdf2_many(psks, essid, threads=8)
    lines, exp = [], set()
    for k, ((w, r), psk) in enumerate(zip(plants, psks)):
        pmk = raw[32 * k:32 * k + 32]
        line = R._line(k % 4, R.OFFSETS[k % 8], ("LE", "BE")[k // 8 % 2], psk, essid, pmk, rng)
        o = O.c_check_key_m22000(line, [psk], False if k % 4 == 0 else pmk, NC)
        assert o and o[0] == psk and o[3] == pmk, k
        lines.append(line)
        exp.add((k, w * F_RULES + r, o[1], o[2], pmk))
    return {"text": "\n".join(rules) + "\n", "rules": rules, "lines": lines, "exp": exp}


def test_more_than_65535_rules(many_rules):
    """f. 70,000 rules `$x $y $z` x three words: launch_rules_prep gets the rule count as grid.y.  One line per (word,
    rule) for the rules on both sides of 65,535, the first two and the last: the hits are the 21 plants with ids
    word * 70000 + rule, and all 210,000 candidates are loaded."""
    f = many_rules
    d = Dictionary.from_words(list(F_WORDS))
    sc = dwpa_amd.Scan(f["lines"], nc=NC, batch=1 << 18)
    try:
        assert sc.set_rules(f["text"]) == F_RULES
        sc.load_rules(d.off.ptr, d.data.ptr, 0, len(F_WORDS))
        assert sc.loaded() == len(F_WORDS) * F_RULES == 210000
        sc.run()
        R._assert_same(R._hitset(sc.hits(cap=256)), f["exp"], "rules")
    finally:
        sc.close()


def test_rules_expand_more_than_65535_rules(many_rules):
    """f. dwpa_rules_expand of one word over the same rules (launch_rules_expand, the same grid) against the rule
    oracle: every one of the 70,000 candidates."""
    f = many_rules
    got = dwpa_amd.rules_expand(f["text"], [F_WORDS[1]])
    ref = OR.expand(f["rules"], [F_WORDS[1]])
    assert len(got) == 1 and len(got[0]) == F_RULES
    bad = [r for r in range(F_RULES) if got[0][r] != ref[0][r]]
    assert not bad, (len(bad), bad[:5], got[0][bad[0]], ref[0][bad[0]])
    assert got[0][65536] == F_WORDS[1] + _suffix(65536)
