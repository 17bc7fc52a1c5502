"""CPU: ``python -m dwpa_amd.assoc`` -- --keyspace, --stdout, -s / -l windows and the exit statuses that need no device
-- and the host-only wrappers' argument checks.  Cracking through the command line is tests/test_gpu_assoc.py."""
import os
import subprocess
import sys

import pytest

import dwpa_amd
from dwpa_amd import _lib as L
from tests import assoc_plan as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    d = tmp_path_factory.mktemp("assoc_cli")
    lines, assoc = A.cpu_fixture()
    (d / "h.hash").write_bytes(b"\n".join(lines) + b"\n")
    A.write_assoc(d / "a.txt", assoc)
    (d / "r.rule").write_text("".join(r + "\n" for r in A.FILE_RULES))
    return {"dir": d, "lines": lines, "assoc": assoc, "hash": str(d / "h.hash"), "afile": str(d / "a.txt"),
            "rules": str(d / "r.rule")}


def cli(*argv):
    return subprocess.run([sys.executable, "-m", "dwpa_amd.assoc", *argv], cwd=ROOT, capture_output=True, timeout=120)


def text(plan, first, count):
    """--stdout of a window: the candidates in index order, the indices without one left out."""
    cands = [plan.candidate(i) for i in range(first, first + count)]
    return b"".join(c + b"\n" for c in cands if c is not None)


@pytest.mark.parametrize("single,use_rules", [(False, False), (True, False), (True, True)])
def test_keyspace_and_stdout(fx, single, use_rules):
    plan = A.Plan(fx["lines"], fx["assoc"], single, A.FILE_RULES if use_rules else None)
    extra = (["--single"] if single else []) + (["-r", fx["rules"]] if use_rules else [])
    r = cli(fx["hash"], fx["afile"], *extra, "--keyspace")
    assert r.returncode == 0 and r.stdout == b"%d\n" % plan.k, r.stderr[-2000:]
    r = cli(fx["hash"], fx["afile"], *extra, "--stdout")
    assert r.returncode == 0 and r.stdout == text(plan, 0, plan.k), r.stderr[-2000:]
    assert r.stdout.count(b"\n") < plan.k or not use_rules  # rules: some indices give no candidate
    # windows: inside one net, across nets, to the end, one index
    for s, l in ((1, 2), (plan.start[1] - 1, plan.start[3] - plan.start[1] + 2), (plan.k - 5, 0), (plan.k - 1, 1)):
        r = cli(fx["hash"], fx["afile"], *extra, "--stdout", "-s", str(s), *(["-l", str(l)] if l else []))
        assert r.returncode == 0 and r.stdout == text(plan, s, l or plan.k - s), (s, l, r.stderr[-2000:])
    r = cli(fx["hash"], fx["afile"], *extra, "--stdout", "-s", "0", "-l", str(plan.k + 100))  # clipped at K
    assert r.returncode == 0 and r.stdout == text(plan, 0, plan.k)


def test_single_alone(fx):
    plan = A.Plan(fx["lines"], None, True, None)
    r = cli(fx["hash"], "--single", "--keyspace")
    assert r.returncode == 0 and r.stdout == b"%d\n" % plan.k, r.stderr[-2000:]
    r = cli(fx["hash"], "--single", "--stdout")
    assert r.returncode == 0 and r.stdout == text(plan, 0, plan.k)


def test_malformed_lines_are_named_on_stderr(fx):
    r = cli(fx["hash"], fx["afile"], "--keyspace")
    assert r.returncode == 0
    bad = [i + 1 for i, ln in enumerate(fx["assoc"]) if A.parse_assoc_line(ln) is None]
    assert len(bad) == 4 and r.stderr.count(b"is not MAC_AP:WORD") == 4
    for n in bad:
        assert b"line %d is not MAC_AP:WORD" % n in r.stderr


def test_exit_255(fx, tmp_path):
    plan = A.Plan(fx["lines"], fx["assoc"], False, None)
    (tmp_path / "bad.rule").write_text("not a rule at all\n")
    for argv in ([fx["hash"], "--keyspace"],                                   # no source
                 ["--single", "--keyspace"],                                   # no hash file
                 [fx["hash"], fx["afile"], "extra", "--keyspace"],
                 [str(tmp_path / "missing.hash"), "--single", "--keyspace"],
                 [fx["hash"], str(tmp_path / "missing.txt"), "--keyspace"],
                 [fx["hash"], "--single", "-r", str(tmp_path / "missing.rule"), "--keyspace"],
                 [fx["hash"], "--single", "-r", str(tmp_path / "bad.rule"), "--keyspace"],
                 [fx["hash"], fx["afile"], "--stdout", "-s", str(plan.k)],     # skip at K
                 [fx["hash"], fx["afile"], "--stdout", "-s", "-1"],
                 [fx["hash"], fx["afile"], "--no-such-option"]):
        r = cli(*argv)
        assert r.returncode == 255 and r.stdout == b"", (argv, r.stderr[-2000:])


def test_wrapper_argument_checks(fx):
    with pytest.raises(L.DwpaError):
        dwpa_amd.assoc_candidates(fx["hash"], [-1], fx["afile"])
    with pytest.raises(L.DwpaError):
        dwpa_amd.assoc_candidates(fx["hash"], [2**64], fx["afile"])
    with pytest.raises(L.DwpaError):
        dwpa_amd.assoc_single(fx["lines"][0], 2**32)
    assert dwpa_amd.assoc_candidates(fx["hash"], [], fx["afile"]) == []
    assert L.load().dwpa_abi_version() == 4
    php = open(os.path.join(ROOT, "php", "dwpa22000.php")).read()
    hdr = open(L.HEADER).read()
    for hook in ("dwpa_debug_assoc_work", "dwpa_debug_assoc_segcap"):  # test hooks stay outside the header
        assert hasattr(L.load(), hook) and hook not in hdr and hook not in php
    assert L.assoc_work() == {"slots_derived": 0, "segments": 0}
