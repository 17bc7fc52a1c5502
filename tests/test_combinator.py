"""CPU: the combinator attack's command line (python -m dwpa_amd.mask -a 1: --stdout and the refusals), the no-device
answers of dwpa_scan_load_combinator / dwpa_crack_combinator and the exported names.  The reference is
itertools.product over the two word lists: the streamed (base) list is the outer loop, the amplifier the inner one,
and the join is always left + right."""
import gzip
import itertools
import os
import subprocess
import sys

import pytest

import dwpa_amd
from dwpa_amd import _lib as L
from dwpa_amd import mask as CLI
from tests import synth as S
from tests.test_mask import NO_DEVICES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BINARY = bytes([0x00, 0x0a, 0xff, 0x41])  # travels as $HEX[]: it holds a line feed
LEFT = [b"alpha", b"", b"p@ss word", BINARY, b"L" * 300, b"\xfe\x01\x80", b"last-no-newline"]
RIGHT = [b"second", b"caf\xc3\xa9", b"", b"crlf", b"\x7f\xff"]


def _lists(tmp_path):
    """A plain left list (an empty line, a $HEX[] word, a 300-byte line, binary bytes, no newline after the last word)
    and a gzip right list with CRLF endings and an empty line."""
    left, right = tmp_path / "left.txt", tmp_path / "right.txt.gz"
    text = [b"$HEX[" + w.hex().encode() + b"]" if w == BINARY else w for w in LEFT]
    left.write_bytes(b"\n".join(text))
    with gzip.open(right, "wb") as f:
        f.write(b"".join(w + b"\r\n" for w in RIGHT))
    return str(left), str(right)


def _expected(left, right, amplifier):
    if amplifier == "right":  # left is the base: outer loop
        pairs = itertools.product(left, right)
    else:
        pairs = ((lw, rw) for rw, lw in itertools.product(right, left))
    return b"".join(lw + rw + b"\n" for lw, rw in pairs)


def _cli(capfdbinary, *argv):
    rc = CLI.main(list(argv))
    cap = capfdbinary.readouterr()
    return rc, cap.out, cap.err


@pytest.mark.parametrize("amplifier", ["right", "left"])
def test_stdout_is_left_times_right(capfdbinary, tmp_path, amplifier):
    left, right = _lists(tmp_path)
    rc, out, _ = _cli(capfdbinary, "-a", "1", "--stdout", "--amplifier", amplifier, left, right)
    assert (rc, out) == (0, _expected(LEFT, RIGHT, amplifier))
    assert out.count(b"\n") >= len(LEFT) * len(RIGHT)  # unfiltered: the 300-byte line and the empty words are there
    # the lists the other way round (gzip left, plain right)
    rc, out, _ = _cli(capfdbinary, "--stdout", "--amplifier", amplifier, "-a", "1", right, left)
    assert (rc, out) == (0, _expected(RIGHT, LEFT, amplifier))


def test_stdout_amplifier_defaults_to_right(capfdbinary, tmp_path):
    left, right = _lists(tmp_path)
    rc, out, _ = _cli(capfdbinary, "-a", "1", "--stdout", left, right)
    assert (rc, out) == (0, _expected(LEFT, RIGHT, "right"))


def _bad(tmp_path):
    left, right = _lists(tmp_path)
    missing = str(tmp_path / "missing.txt")
    return [["-a", "1", "h.hash", left],                                  # one list only
            ["-a", "1", "--stdout", left],
            ["-a", "1", "h.hash", left, right, left],                     # three lists
            ["-a", "1", "--stdout", left, right, left],
            ["-a", "1", "-s", "1", "h.hash", left, right],
            ["-a", "1", "--stdout", "-s", "1", left, right],
            ["-a", "1", "-l", "5", "h.hash", left, right],
            ["-a", "1", "-i", "h.hash", left, right],
            ["-a", "1", "--stdout", "-i", left, right],
            ["-a", "1", "--keyspace", left, right],
            ["-a", "1", "-1", "abc", "h.hash", left, right],
            ["-a", "1", "--stdout", "-1", "abc", left, right],
            ["-a", "1", "-j", "c", "h.hash", left, right],
            ["-a", "1", "--stdout", "-j", "c", left, right],
            ["-a", "1", "-k", "$1", "h.hash", left, right],
            ["-a", "1", "--stdout", "-k", "$1", left, right],
            ["-a", "1", "--amplifier", "middle", "h.hash", left, right],  # an unknown --amplifier
            ["-a", "1", "--stdout", "--amplifier", "both", left, right],
            ["-a", "1", "--stdout", missing, right],
            ["-a", "1", "h.hash", left, missing]]


@pytest.mark.parametrize("case", range(20))
def test_bad_invocations(capfdbinary, tmp_path, case):
    """Each exits 255 with nothing on stdout and a message on stderr (no device is needed to refuse any of them)."""
    cases = _bad(tmp_path)
    assert len(cases) == 20
    rc, out, err = _cli(capfdbinary, *cases[case])
    assert rc == 255 and out == b"" and err.strip()


def test_as_a_module(tmp_path):
    left, right = _lists(tmp_path)
    r = subprocess.run([sys.executable, "-m", "dwpa_amd.mask", "-a", "1", "--stdout", "--amplifier", "left", left,
                        right], cwd=ROOT, capture_output=True, timeout=60)
    assert (r.returncode, r.stdout) == (0, _expected(LEFT, RIGHT, "left"))
    r = subprocess.run([sys.executable, "-m", "dwpa_amd.mask", "-a", "1", "--keyspace", left, right], cwd=ROOT,
                       capture_output=True, timeout=60)
    assert r.returncode == 255 and r.stdout == b"" and b"dwpa_amd.mask" in r.stderr


def test_exported_names():
    assert (dwpa_amd.DWPA_COMBI_AMP_RIGHT, dwpa_amd.DWPA_COMBI_AMP_LEFT) == (0, 1)
    assert callable(dwpa_amd.crack_combinator) and callable(dwpa_amd.Scan.load_combinator)
    for name in ("crack_combinator", "DWPA_COMBI_AMP_RIGHT", "DWPA_COMBI_AMP_LEFT"):
        assert name in dwpa_amd.__all__
    lib = L.load()
    assert lib.dwpa_scan_load_combinator and lib.dwpa_crack_combinator and lib.dwpa_abi_version() == 4


# ---------------------------------------------------------------------------------------------------------------
# without a device
# ---------------------------------------------------------------------------------------------------------------
_NODEV_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import dwpa_amd
from dwpa_amd import _lib as L
from dwpa_amd import m22000 as M
lib = L.load()
hf, out, d, missing = sys.argv[2:6]
print(lib.dwpa_device_count(),
      lib.dwpa_scan_load_combinator(None, None, None, 0, 1, None, None, 1, 0, 1, L.DWPA_COMBI_AMP_RIGHT, 8, 63, None),
      lib.dwpa_scan_load_combinator(None, None, None, 0, 1, None, None, 1, 0, 1, L.DWPA_COMBI_AMP_LEFT, 8, 63, None))
for hash_file, left, right, side in ((hf, d, d, 0), (hf, d, d, 1), (hf, missing, d, 0), (hf, d, missing, 0),
                                     (hf, missing, d, 1), (hf, d, missing, 5), (hf, d, d, 2), (hf, d, d, -1),
                                     (missing, d, d, 0)):
    rc, st = dwpa_amd.crack_combinator(hash_file, left, right, side, out_file=out)
    print(rc, *st)
print(M.crack_stats()["candidates"], dwpa_amd.DWPA_COMBI_AMP_RIGHT, dwpa_amd.DWPA_COMBI_AMP_LEFT)
"""


def test_without_a_device(tmp_path):
    """A process that sees no device: dwpa_scan_load_combinator says DWPA_E_NODEV, dwpa_crack_combinator
    DWPA_RC_ERROR; an unreadable left or right list is marked DWPA_E_IO in its own dict_status entry (whatever else is
    wrong with the call) with the other DWPA_DICT_OK; an unknown amp_side and a missing hash file are DWPA_RC_ERROR;
    no outfile is created."""
    hf, d = tmp_path / "h.hash", tmp_path / "d.txt"
    hf.write_bytes(b"\n".join(S.CHALLENGE_LINES) + b"\n")
    d.write_bytes(b"word1\nword2\n")
    env = {k: v for k, v in os.environ.items() if k not in ("DWPA_CPU_FALLBACK", "ROCR_VISIBLE_DEVICES")}
    env["HIP_VISIBLE_DEVICES"] = NO_DEVICES
    r = subprocess.run([sys.executable, "-c", _NODEV_CHILD, ROOT, str(hf), str(tmp_path / "o.key"), str(d),
                        str(tmp_path / "missing.txt")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    nodev, err, ok, io = (str(v) for v in (L.DWPA_E_NODEV, L.DWPA_RC_ERROR, L.DWPA_DICT_OK, L.DWPA_E_IO))
    assert [ln.split() for ln in r.stdout.splitlines()] == [
        [nodev] * 3, [err, ok, ok], [err, ok, ok], [err, io, ok], [err, ok, io], [err, io, ok], [err, ok, io],
        [err, ok, ok], [err, ok, ok], [err, ok, ok], ["0", "0", "1"]], r.stdout
    assert not (tmp_path / "o.key").exists()  # refused before the outfile is opened
