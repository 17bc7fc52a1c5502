"""CPU: rules on chain list parts on the host -- python -m dwpa_amd.chain with rules:FILE / rule:TEXT (--keyspace,
--stdout and the refusals), chain_candidate(..., rules=), the no-device answers of dwpa_scan_set_chain_rules and
dwpa_crack_chain_rules, and what the crack call refuses before it touches a device.  The reference is
tests/chain_rules_plan.RuledChain: rule-major choices, oracle/rules.py's pieces, rejected choices omitted."""
import ctypes
import os
import subprocess
import sys

import pytest

import dwpa_amd
from dwpa_amd import _lib as L
from dwpa_amd import chain as CLI
from dwpa_amd import m22000 as M
from oracle import rules as OR
from tests import chain_rules_plan as P
from tests import synth as S
from tests.test_mask import NO_DEVICES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = ["-1", "ab", "-2", "cde"]  # P.CUSTOM
# rules files: a comment, an empty line and a line that does not parse around the rules; hashcat's -r loader (the
# default) also skips the lines with a reject or a memory function
FILE_A = ["# rules on the first list"] + P.RSA[:5] + ["", "no such rule"] + P.RSA[5:]
FILE_B = P.RSB


def _loaded(lines, full):
    return [r for r in lines if OR.parse(r) is not None and (full or OR.hashcat_loads(r))]


def _files(tmp_path):
    def put(name, words):
        (tmp_path / name).write_bytes(b"".join(w + b"\n" for w in words))
        return "list:" + str(tmp_path / name)
    paths = {"A": put("a.txt", P.LA), "B": put("b.txt", P.LB), "U": put("u.txt", P.LU)}
    (tmp_path / "a.rule").write_text("\n".join(FILE_A) + "\n")
    (tmp_path / "b.rule").write_text("\n".join(FILE_B))  # no newline after the last rule
    paths["ra"], paths["rb"] = "rules:" + str(tmp_path / "a.rule"), "rules:" + str(tmp_path / "b.rule")
    return paths


def _cli(capfdbinary, *argv):
    rc = CLI.main(list(argv))
    cap = capfdbinary.readouterr()
    return rc, cap.out, cap.err


def _lines(ch, skip=0, limit=0):
    """What --stdout prints: every candidate of the window, unfiltered, rejected choices omitted."""
    end = ch.k if not limit else min(ch.k, skip + limit)
    out = []
    for i in range(skip, end):
        ps = ch.pieces(i)
        if None not in ps:
            out.append(b"".join(ps) + b"\n")
    return b"".join(out)


@pytest.mark.parametrize("full", [False, True], ids=["hashcat", "full"])
def test_keyspace_and_stdout(capfdbinary, tmp_path, monkeypatch, full):
    """--keyspace is the product with nwords x R, --stdout the reference byte for byte, over whole spaces and over
    windows that cross a rule boundary and a part wrap; R follows the process's rule mode."""
    if full:
        monkeypatch.setenv("DWPA_RULE_MODE", "full")
    else:
        monkeypatch.delenv("DWPA_RULE_MODE", raising=False)
    paths = _files(tmp_path)
    ra, rb = _loaded(FILE_A, full), _loaded(FILE_B, full)
    assert len(ra) == (10 if full else 8) and len(rb) == 5
    shapes = [([paths["A"], paths["ra"], "mask:?1-?2"], P.RuledChain([(P.LA, ra), P.ML])),
              (["mask:?1-?2", paths["A"], paths["ra"]], P.RuledChain([P.ML, (P.LA, ra)])),
              ([paths["A"], paths["ra"], paths["B"], paths["rb"]], P.RuledChain([(P.LA, ra), (P.LB, rb)])),
              ([paths["U"], paths["B"], paths["rb"], "mask:?1?2", paths["B"], "rule:$1"],
               P.RuledChain([P.LU, (P.LB, rb), P.M6, (P.LB, ["$1"])])),
              ([paths["B"], "rule:^x $y"], P.RuledChain([(P.LB, ["^x $y"])]))]
    for argv, ch in shapes:
        rc, out, err = _cli(capfdbinary, "--keyspace", *SETS, *argv)
        assert (rc, out.split()) == (0, [b"%d" % ch.k]), err
        assert (b"no such rule" in err) == (paths["ra"] in argv)  # the skipped line is named
        rc, out, err = _cli(capfdbinary, "--stdout", *SETS, *argv)
        whole = _lines(ch)
        assert (rc, out) == (0, whole)
        assert 0 < whole.count(b"\n") < ch.k  # some choices are rejected, and they are omitted
        last = ch.radix[-1]
        nw = len(ch.parts[-1]) if ch.rules[-1] is not None else last
        windows = [(0, 1), (ch.k - 1, 0), (ch.k - 1, 5), (ch.k // 3, ch.k // 2),
                   (nw - 2, 5),                 # across a rule boundary of the last part (or its wrap)
                   (last - 3, 7),               # across a wrap of the last part
                   (ch.k - last - 2, last + 2)]
        for skip, limit in windows:
            if skip < 0:
                continue
            rc, out, err = _cli(capfdbinary, "--stdout", "-s", str(skip), "-l", str(limit), *SETS, *argv)
            assert (rc, out) == (0, _lines(ch, skip, limit)), (argv, skip, limit)


def test_stdout_as_a_module(tmp_path):
    paths = _files(tmp_path)
    ch = P.RuledChain([(P.LB, ["c", "$1"]), b"?d"], ())
    (tmp_path / "c.rule").write_text("c\n$1\n")
    r = subprocess.run([sys.executable, "-m", "dwpa_amd.chain", "--stdout", "-s", "7", "-l", "90", paths["B"],
                        "rules:" + str(tmp_path / "c.rule"), "mask:?d"], cwd=ROOT, capture_output=True, timeout=60)
    assert (r.returncode, r.stdout) == (0, _lines(ch, 7, 90)) and r.stdout


def test_chain_candidate_with_rules():
    """chain_candidate(..., rules=) is the reference, candidate by candidate, and None on a reject."""
    ch = P.shape("URMR")
    parts = [P.LU, P.LC, ("mask", P.M2), P.LD]
    rules = [None, P.rules_text(P.RSC), None, P.rules_text(P.RSB)]
    none = 0
    for i in list(range(0, ch.k, 7)) + [ch.k - 1]:
        ps = ch.pieces(i)
        exp = None if None in ps else b"".join(ps)
        assert M.chain_candidate(parts, i, P.CUSTOM, rules) == exp, i
        none += exp is None
    assert 0 < none < ch.k // 7
    with pytest.raises(L.DwpaError):
        M.chain_candidate(parts, ch.k, P.CUSTOM, rules)
    # rule-major: the word runs fastest inside the part
    ws = [b"aBc1", b"dEf2"]
    assert [M.chain_candidate([ws], i, (), ["u\nl\n"]) for i in range(4)] == [b"ABC1", b"DEF2", b"abc1", b"def2"]
    assert M.chain_candidate([ws], 1, (), [None]) == b"dEf2" == M.chain_candidate([ws], 1)
    # lines that do not parse are skipped; the interpreter takes reject functions
    assert [M.chain_candidate([ws + [b""]], i, (), ["bogus!!\n>9\n$x"]) for i in range(6)] == \
        [None, None, None, b"aBc1x", b"dEf2x", None]
    for bad, code in (([ws, ("mask", b"?d")], L.DWPA_E_ARG), ([ws], L.DWPA_E_RULE)):
        with pytest.raises(L.DwpaError) as e:
            M.chain_candidate(bad, 0, (), [None, ":"] if len(bad) == 2 else ["no such rule"])
        assert e.value.code == code
    with pytest.raises(L.DwpaError):
        M.chain_candidate([ws], 0, (), [":", ":"])


def test_refusals(capfdbinary, tmp_path):
    """Exit 255, nothing on stdout, a message on stderr."""
    paths = _files(tmp_path)
    (tmp_path / "none.rule").write_text("# nothing\nno such rule\n")
    (tmp_path / "reject.rule").write_text(">6 $#\n")
    bad = [["--keyspace", paths["ra"], paths["A"]],                              # a modifier that comes first
           ["--keyspace", "rule:c"],
           ["--keyspace", paths["A"], "mask:?d", paths["ra"]],                    # after a mask
           ["--stdout", "mask:?d", "rule:c", paths["A"]],
           ["--keyspace", paths["A"], paths["ra"], "rule:c"],                     # two modifiers on one part
           ["--keyspace", paths["A"], "rule:c", "rule:u", "mask:?d"],
           ["--keyspace", paths["A"], "rules:" + str(tmp_path / "missing.rule")],  # a missing rules file
           ["--keyspace", paths["A"], "rules:" + str(tmp_path / "none.rule")],     # no valid line
           ["--stdout", paths["A"], "rule:no such rule"],
           ["--keyspace", paths["A"], "rules:" + str(tmp_path / "reject.rule")],   # hashcat's -r loader takes none of it
           ["--keyspace", paths["A"], "rule:c", paths["B"], paths["A"], paths["B"], paths["A"]]]  # five parts
    for argv in bad:
        rc, out, err = _cli(capfdbinary, *argv)
        assert (rc, out) == (255, b"") and b"dwpa_amd.chain" in err, argv
    # four parts with a modifier each are within the limit: the modifiers do not count
    four = [x for k in "ABAB" for x in (paths[k], "rule:c")]
    rc, out, err = _cli(capfdbinary, "--keyspace", *four)
    assert (rc, out.split()) == (0, [b"%d" % (len(P.LA) * len(P.LB)) ** 2])
    # the mask tool still refuses -j / -k
    from dwpa_amd import mask as MASK
    assert MASK.main(["--stdout", "-a", "1", "-j", "c", str(tmp_path / "a.txt"), str(tmp_path / "b.txt")]) == 255
    capfdbinary.readouterr()


def test_exported_and_declared():
    lib = L.load()
    header = open(L.HEADER).read()
    for name in ("dwpa_scan_set_chain_rules", "dwpa_crack_chain_rules"):
        assert hasattr(lib, name) and name in L.SIGNATURES and name in header
    assert lib.dwpa_abi_version() == 4
    assert "rules" in dwpa_amd.crack_chain.__doc__ and hasattr(dwpa_amd.Scan, "set_chain_rules")


_NODEV_CHILD = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
from dwpa_amd import _lib as L
from dwpa_amd import m22000 as M
lib = L.load()
k = ctypes.c_uint64(7)
print(lib.dwpa_scan_set_chain_rules(None, 0, b":", 1, ctypes.byref(k)), k.value)
hf, out, words, rules, missing, none = sys.argv[2:8]
LIST, MASK = L.DWPA_CHAIN_LIST, L.DWPA_CHAIN_MASK
for parts, rl in (([(LIST, words), (MASK, "?d?d")], [rules, None]),
                  ([(LIST, words), (MASK, "?d?d")], [missing, None]),
                  ([(LIST, words), (MASK, "?d?d")], [none, None]),
                  ([(LIST, words), (MASK, "?d?d")], [None, rules]),
                  ([(LIST, words), (MASK, "?d?d")], [None, None])):
    rc, st = M.crack_chain(hf, parts, (), 0, 0, 8, out, rules=rl)
    s = M.crack_stats()
    print(rc, s["rules"], s["rules_skipped"], s["rules_rejmem"])
"""


def test_without_a_device(tmp_path):
    """dwpa_scan_set_chain_rules without a device: DWPA_E_NODEV, *keyspace untouched.  dwpa_crack_chain_rules: the
    rules files are looked at before any device -- the counts are published whatever becomes of the call, and an
    unreadable file, a file with no valid rule and rules on a mask part are named on stderr."""
    hf, words = tmp_path / "h.22000", tmp_path / "w.txt"
    hf.write_bytes(b"\n".join(S.CHALLENGE_LINES) + b"\n")
    words.write_bytes(b"word1\nword2\n")
    (tmp_path / "r.rule").write_text(":\nc\n>6 $#\nM [ 4\nno such rule\n")
    (tmp_path / "none.rule").write_text("no such rule\n>9\n")
    env = {k: v for k, v in os.environ.items() if k not in ("DWPA_CPU_FALLBACK", "ROCR_VISIBLE_DEVICES",
                                                            "DWPA_RULE_MODE")}
    env["HIP_VISIBLE_DEVICES"] = NO_DEVICES
    r = subprocess.run([sys.executable, "-c", _NODEV_CHILD, ROOT, str(hf), str(tmp_path / "o.key"), str(words),
                        str(tmp_path / "r.rule"), str(tmp_path / "missing.rule"), str(tmp_path / "none.rule")],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    err = str(L.DWPA_RC_ERROR)
    assert [ln.split() for ln in r.stdout.splitlines()] == [
        [str(L.DWPA_E_NODEV), "7"],
        [err, "2", "3", "2"],   # hashcat's loader: ':' and 'c' load, two reject / memory lines and a bad one do not
        [err, "0", "0", "0"],   # unreadable
        [err, "0", "2", "1"],   # no valid rule
        [err, "0", "0", "0"],   # rules on a mask part
        [err, "0", "0", "0"]], r.stdout
    assert "missing.rule: cannot be opened" in r.stderr and "none.rule: no valid rules left" in r.stderr
    assert "rules go with a list part" in r.stderr
    assert not (tmp_path / "o.key").exists()
