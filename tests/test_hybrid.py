"""CPU: the hybrid attacks' command line (python -m dwpa_amd.mask -a 6 / -a 7: --stdout and the refusals) and the
no-device answers of dwpa_scan_load_hybrid / dwpa_crack_hybrid.  The reference is itertools.product over the word list
and the mask expander of tests/test_mask.py: word-major, mask index fastest."""
import gzip
import itertools
import os
import subprocess
import sys

import pytest

from dwpa_amd import _lib as L
from dwpa_amd import mask as CLI
from tests import synth as S
from tests.test_mask import NO_DEVICES, ref_candidate, ref_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BINARY = bytes([0x00, 0x0a, 0xff, 0x41])  # travels as $HEX[]: it holds a line feed
WORDS_1 = [b"alpha", b"", b"p@ss word", BINARY, b"x" * 70, b"last-no-newline"]
WORDS_2 = [b"second", b"caf\xc3\xa9", b"crlf"]
MASK, CUSTOM = b"?1x?2", (b"ab", b"cde")


def _dicts(tmp_path):
    """A plain dictionary (an empty line, a $HEX[] word, no newline after the last word) and a gzip one with CRLF."""
    d1, d2 = tmp_path / "one.txt", tmp_path / "two.txt.gz"
    text = [b"$HEX[" + w.hex().encode() + b"]" if w == BINARY else w for w in WORDS_1]
    d1.write_bytes(b"\n".join(text))
    with gzip.open(d2, "wb") as f:
        f.write(b"".join(w + b"\r\n" for w in WORDS_2))
    return str(d1), str(d2)


def _expected(words, mask, custom, mode):
    sets, k = ref_sets(mask, custom)
    cands = [ref_candidate(sets, i) for i in range(k)]
    pairs = itertools.product(words, cands)
    return b"".join((w + m if mode == 6 else m + w) + b"\n" for w, m in pairs)


def _cli(capfdbinary, *argv):
    rc = CLI.main(list(argv))
    return rc, capfdbinary.readouterr().out


@pytest.mark.parametrize("mode", [6, 7])
def test_stdout_is_words_times_mask(capfdbinary, tmp_path, mode):
    d1, d2 = _dicts(tmp_path)
    sets = ("-1", "ab", "-2", "cde")
    order = (lambda dicts, mask: [*dicts, mask]) if mode == 6 else (lambda dicts, mask: [mask, *dicts])
    # one plain dictionary: the empty line, the $HEX[] word and the unterminated last line are words
    assert _cli(capfdbinary, "-a", str(mode), "--stdout", *sets, *order([d1], MASK.decode())) == \
        (0, _expected(WORDS_1, MASK, CUSTOM, mode))
    # a gzip dictionary
    assert _cli(capfdbinary, "-a", str(mode), "--stdout", *sets, *order([d2], MASK.decode())) == \
        (0, _expected(WORDS_2, MASK, CUSTOM, mode))
    # two dictionaries, in the order given
    assert _cli(capfdbinary, "--stdout", *sets, "-a", str(mode), *order([d2, d1], MASK.decode())) == \
        (0, _expected(WORDS_2 + WORDS_1, MASK, CUSTOM, mode))
    # custom sets in hex, raw bytes among them; a built-in set and a literal
    assert _cli(capfdbinary, "-a", str(mode), "--stdout", "--hex-charset", "-1", "00ff0a", "-3", "3f64",
                *order([d1, d2], "?1?d-?3")) == \
        (0, _expected(WORDS_1 + WORDS_2, b"?1?d-?3", (bytes([0, 255, 10]), None, b"?d"), mode))


def test_attack_mode_3_is_still_the_default(capfdbinary):
    assert _cli(capfdbinary, "--stdout", "-1", "01", "?1?1") == (0, b"00\n01\n10\n11\n")
    assert _cli(capfdbinary, "-a", "3", "--keyspace", "?d?d") == (0, b"100\n")


def _bad(tmp_path):
    d1, d2 = _dicts(tmp_path)
    missing = str(tmp_path / "missing.txt")
    return [["-a", "5", "h.hash", d1, "?d"], ["-a", "5", "--stdout", d1, "?d"], ["-a", "6", "--stdout", d1],
            ["-a", "6", "h.hash"], ["-a", "6", "h.hash", d1], ["-a", "6", "-s", "1", "h.hash", d1, "?d?d?d"],
            ["-a", "6", "--stdout", "-s", "1", d1, "?d"], ["-a", "6", "-l", "5", "h.hash", d1, "?d?d?d"],
            ["-a", "7", "-i", "h.hash", "?d?d?d", d1], ["-a", "7", "--stdout", "-i", "?d?d?d", d1],
            ["-a", "7", "--increment-min", "2", "h.hash", "?d?d?d", d1], ["-a", "6", "--keyspace", d1, "?d"],
            ["-a", "7", "--keyspace", "?d", d1], ["-a", "6", "--stdout", d1, "?x"], ["-a", "6", "h.hash", d1, "?d?"],
            ["-a", "7", "--stdout", "?1", d1], ["-a", "7", "h.hash", "?5", d1], ["-a", "6", "--stdout", missing, "?d"],
            ["-a", "6", "h.hash", d1, missing, "?d"], ["-a", "7", "h.hash", "?d", missing],
            ["-a", "7", "--stdout", "?d", d2, missing], ["-a", "6", "--stdout", "--hex-charset", "-1", "0g", d1, "?1"]]


@pytest.mark.parametrize("case", range(22))
def test_bad_invocations(capfdbinary, tmp_path, case):
    """Each exits 255 with nothing on stdout (no device is needed to refuse any of them)."""
    cases = _bad(tmp_path)
    assert len(cases) == 22
    rc, out = _cli(capfdbinary, *cases[case])
    assert rc == 255 and out == b""


def test_as_a_module(tmp_path):
    d1, _ = _dicts(tmp_path)
    r = subprocess.run([sys.executable, "-m", "dwpa_amd.mask", "-a", "7", "--stdout", "-1", "ab", "-2", "cde",
                        MASK.decode(), d1], cwd=ROOT, capture_output=True, timeout=60)
    assert (r.returncode, r.stdout) == (0, _expected(WORDS_1, MASK, CUSTOM, 7))
    r = subprocess.run([sys.executable, "-m", "dwpa_amd.mask", "-a", "6", "--keyspace", d1, "?d"], cwd=ROOT,
                       capture_output=True, timeout=60)
    assert r.returncode == 255 and r.stdout == b"" and b"dwpa_amd.mask" in r.stderr


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
      lib.dwpa_scan_load_hybrid(None, None, None, 0, 1, 0, 1, L.DWPA_HYBRID_WORD_MASK, 8, 63, None),
      lib.dwpa_scan_load_hybrid(None, None, None, 0, 1, 0, 1, L.DWPA_HYBRID_MASK_WORD, 8, 63, None))
for mask, dicts, mode in (("?d?d?d", [d], 6), ("?d?d?d", [d], 7), ("?d?", [d], 6), ("?d?d?d", [d, missing], 7),
                          ("?x", [missing, d], 6), ("?d?d?d", [d], 5)):
    rc, st = dwpa_amd.crack_hybrid(hf, dicts, mask, mode=mode, out_file=out)
    print(rc, *st)
print(M.crack_stats()["candidates"], dwpa_amd.DWPA_HYBRID_WORD_MASK, dwpa_amd.DWPA_HYBRID_MASK_WORD)
"""


def test_without_a_device(tmp_path):
    """A process that sees no device: dwpa_scan_load_hybrid says DWPA_E_NODEV, dwpa_crack_hybrid DWPA_RC_ERROR; a bad
    mask, an unknown mode and an unreadable dictionary are DWPA_RC_ERROR too, the unreadable dictionary marked
    DWPA_E_IO in dict_status (whatever else is wrong with the call), the readable ones DWPA_DICT_OK."""
    hf, d = tmp_path / "h.hash", tmp_path / "d.txt"
    hf.write_bytes(b"\n".join(S.CHALLENGE_LINES) + b"\n")
    d.write_bytes(b"word1\nword2\n")
    env = {k: v for k, v in os.environ.items() if k not in ("DWPA_CPU_FALLBACK", "ROCR_VISIBLE_DEVICES")}
    env["HIP_VISIBLE_DEVICES"] = NO_DEVICES
    r = subprocess.run([sys.executable, "-c", _NODEV_CHILD, ROOT, str(hf), str(tmp_path / "o.key"), str(d),
                        str(tmp_path / "missing.txt")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    nodev, err, ok, io = L.DWPA_E_NODEV, L.DWPA_RC_ERROR, L.DWPA_DICT_OK, L.DWPA_E_IO
    assert [ln.split() for ln in r.stdout.splitlines()] == [
        [str(nodev)] * 3, [str(err), str(ok)], [str(err), str(ok)], [str(err), str(ok)], [str(err), str(ok), str(io)],
        [str(err), str(io), str(ok)], [str(err), str(ok)], ["0", "6", "7"]], r.stdout
    assert not (tmp_path / "o.key").exists()  # refused before the outfile is opened
