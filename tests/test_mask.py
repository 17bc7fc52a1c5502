"""CPU: the hashcat -a 3 mask language on the host (dwpa_mask_keyspace / dwpa_mask_candidate, dwpa_amd/csrc/mask.cpp),
the no-device answers of the three device entry points, the command line (python -m dwpa_amd.mask) and the fuzz
target.  The reference is the small expander below: the built-in table, itertools.product order."""
import ctypes
import itertools
import os
import random
import string
import subprocess
import sys

import pytest

import dwpa_amd
from dwpa_amd import _lib as L
from dwpa_amd import m22000 as M
from dwpa_amd import mask as CLI
from tests import synth as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------
_SPECIAL = bytes(list(range(0x20, 0x30)) + list(range(0x3a, 0x41)) + list(range(0x5b, 0x61)) + list(range(0x7b, 0x7f)))
BUILTIN = {"l": string.ascii_lowercase.encode(), "u": string.ascii_uppercase.encode(), "d": b"0123456789",
           "h": b"0123456789abcdef", "H": b"0123456789ABCDEF", "s": _SPECIAL, "b": bytes(range(256))}
BUILTIN["a"] = BUILTIN["l"] + BUILTIN["u"] + BUILTIN["d"] + BUILTIN["s"]
assert len(_SPECIAL) == 33 and len(BUILTIN["a"]) == 95 == len(set(BUILTIN["a"]))


def _tokens(text, customs, ncustom):
    """One byte string per token of mask / custom-set text; ValueError for what the language refuses."""
    out, i = [], 0
    while i < len(text):
        if text[i:i + 1] != b"?":
            out.append(text[i:i + 1])
            i += 1
            continue
        c = text[i + 1:i + 2].decode("latin-1")
        if c == "":
            raise ValueError("lone ?")
        if c == "?":
            out.append(b"?")
        elif c in "1234":
            if int(c) > ncustom or customs[int(c) - 1] is None:
                raise ValueError("custom set")
            out.append(customs[int(c) - 1])
        elif c in BUILTIN:
            out.append(BUILTIN[c])
        else:
            raise ValueError("letter")
        i += 2
    return out


def ref_sets(mask, custom=()):
    """The set of every position, in order, duplicates dropped (first occurrence kept)."""
    custom = list(custom) + [None] * (4 - len(custom))
    cs = [None] * 4
    for k, c in enumerate(custom):
        if c is not None:
            cs[k] = bytes(dict.fromkeys(b"".join(_tokens(c, cs, k))))
            if not cs[k]:
                raise ValueError("empty set")
    sets = [bytes(dict.fromkeys(t)) for t in _tokens(mask, cs, 4)]
    k = 1
    for s in sets:
        k *= len(s)
    if not 1 <= len(sets) <= 63 or k > 2**64 - 1:
        raise ValueError("positions / keyspace")
    return sets, k


def ref_candidate(sets, i):
    """Element i of itertools.product(*sets): the mixed-radix numeral of i, last position fastest."""
    out = bytearray(len(sets))
    for p in range(len(sets) - 1, -1, -1):
        i, d = divmod(i, len(sets[p]))
        out[p] = sets[p][d]
    assert i == 0
    return bytes(out)


RAW = bytes([0x00, 0x0a, 0x7f, 0x80, 0xff]) + b"a"
# (mask, custom sets)
MASKS = [(b"?" + c.encode(), ()) for c in "ludhHsab"] + [
    (b"?l?u?d?h?H?s?a", ()), (b"??", ()), (b"a", ()), (b"?d", ()), (b"literal", ()), (b"pre??x?1?2?l", (b"ab", b"?dXY")),
    (b"?1", (b"?l?d",)), (b"?1?2?3?4", (b"ab", b"?1c", b"?2?1d", b"?3?d")), (b"?2?1", (b"?h?H", b"?1?s??")),
    (b"?1?1", (b"aabcabcdd",)), (b"?1x?1", (b"?d?h?d",)), (b"?3", (None, None, b"xyz")), (b"?4?1", (b"?a?b", None, None, b"?b")),
    (b"passw?1?1?1", (RAW,)), (b"?1?b", (bytes([0, 0, 10, 255, 0]),)), (b"\x00\xff?b\n", ()), (b"?b?b", ()),
    (b"?d" * 8, ()), (b"?1" * 8, (b"?l?d",)), (b"?a" * 8, ()), (b"?a" * 9, ()), (b"?b?b?b?b?b?b?b?a", ()),
    (b"?b?b?b?b?b?b?b?d", ()), (b"?d" * 19, ()), (b"?h" * 15, ()), (b"?l" * 13, ()), (b"a" * 63, ()), (b"?" * 126, ()),
    (b"?h" + b"x" * 30 + b"?H?s" + b"y" * 27 + b"?u?d?l", ()), (b"x?1y?2z?3w?4", (bytes([1, 2]), bytes([3, 4, 5]), b"?d", b"?1?2?3")),
    (b"?d" * 19 + b"A" * 44, ()), (b"?l?l?l?l?d?d?d?d", ()), (b"?u?l?l?l?l?l?d?d?s", ()), (b"?1?1?1?1?1?1?1?1?1?1", (b"01",)),
    (b"?s?s?s?s?s?s?s?s?s?s?s?s", ()),
]
BAD = [(b"?x", ()), (b"?", ()), (b"abc?", ()), (b"?d?", ()), (b"?1", ()), (b"?2", (b"ab",)), (b"?1", (b"?1",)),
       (b"?1", (b"?2", b"ab")), (b"?d", (b"",)), (b"?2", (None, b"")), (b"?d", (b"?",)), (b"?d", (b"?x",)), (b"", ()),
       (b"?5", (b"a", b"b", b"c", b"d")), (b"?0", ()), (b"?L", ()), (b"?b" * 8, ()), (b"?a" * 10, ()), (b"a" * 64, ()),
       (b"?d" * 64, ()), (b"?d" * 20, ()), (b"?1?2", (b"a", None))]


def test_the_cases_cover_the_language():
    assert len(MASKS) >= 40
    ks = [ref_sets(m, c)[1] for m, c in MASKS]
    ns = [len(ref_sets(m, c)[0]) for m, c in MASKS]
    assert 1 in ns and 63 in ns and 95 * 2**56 in ks and max(ks) < 2**64 and sum(k > 2**32 for k in ks) >= 8
    for m, c in BAD:
        with pytest.raises(ValueError):
            ref_sets(m, c)
    # the reference's index arithmetic is itertools.product order
    for m, c in MASKS:
        sets, k = ref_sets(m, c)
        if k <= 5000:
            assert [bytes(t) for t in itertools.product(*sets)] == [ref_candidate(sets, i) for i in range(k)]


@pytest.mark.parametrize("case", range(len(MASKS)))
def test_keyspace_and_candidates_equal_the_reference(case):
    mask, custom = MASKS[case]
    sets, k = ref_sets(mask, custom)
    assert M.mask_keyspace(mask, custom) == k
    assert M.mask_positions(mask, custom) == len(sets)
    rng = random.Random(case)
    idx = [0, k - 1] + ([rng.randrange(k) for _ in range(200)] if k > 202 else list(range(k)))
    for i in idx:
        assert M.mask_candidate(mask, i, custom) == ref_candidate(sets, i), (mask, i)
    with pytest.raises(L.DwpaError) as e:
        M.mask_candidate(mask, k, custom)
    assert e.value.code == L.DWPA_E_ARG


@pytest.mark.parametrize("case", range(len(BAD)))
def test_errors_are_arg(case):
    mask, custom = BAD[case]
    for call in (lambda: M.mask_keyspace(mask, custom), lambda: M.mask_candidate(mask, 0, custom)):
        with pytest.raises(L.DwpaError) as e:
            call()
        assert e.value.code == L.DWPA_E_ARG


def test_null_arguments():
    lib = L.load()
    k, n = ctypes.c_uint64(7), ctypes.c_uint32(7)
    assert lib.dwpa_mask_keyspace(b"?d?l", 4, None, ctypes.byref(n), ctypes.byref(k)) == 0  # custom may be NULL
    assert (n.value, k.value) == (2, 260)
    assert lib.dwpa_mask_keyspace(b"?d?l", 4, None, None, None) == 0
    assert lib.dwpa_mask_keyspace(None, 0, None, None, None) == L.DWPA_E_ARG
    assert lib.dwpa_mask_keyspace(b"?1", 2, None, None, None) == L.DWPA_E_ARG
    assert lib.dwpa_mask_candidate(b"?d", 2, None, 0, None, ctypes.byref(n)) == L.DWPA_E_ARG
    out = ctypes.create_string_buffer(b"\xaa" * 64, 64)
    assert lib.dwpa_mask_candidate(b"?d?d", 4, None, 42, out, ctypes.byref(n)) == 0
    assert out.raw == b"42" + bytes(62) and n.value == 2
    assert lib.dwpa_mask_keyspace(b"?d?dXYZ", 4, None, None, ctypes.byref(k)) == 0 and k.value == 100  # mask_len rules


@pytest.mark.parametrize("n", range(1, 20))
def test_digits_equal_the_numeric_keyspace(n):
    """?d x N at index v is load_numeric's candidate v: the zero-padded decimal."""
    rng = random.Random(n)
    k = 10**n
    assert M.mask_keyspace(b"?d" * n) == k
    for v in [0, 1, 9, 10, k - 1, k // 2] + [rng.randrange(k) for _ in range(50)]:
        if v < k:
            assert M.mask_candidate(b"?d" * n, v) == b"%0*d" % (n, v)


# ---------------------------------------------------------------------------------------------------------------
# without a device
# ---------------------------------------------------------------------------------------------------------------
_NODEV_CHILD = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
import dwpa_amd
from dwpa_amd import _lib as L
from dwpa_amd import m22000 as M
lib = L.load()
k = ctypes.c_uint64(0)
print(lib.dwpa_device_count(),
      lib.dwpa_scan_set_mask(None, b"?d?d", 4, None, ctypes.byref(k)),
      lib.dwpa_scan_load_mask(None, 0, 1, None),
      M.crack_mask(sys.argv[2], "?d?d?d?d?d?d?d?d", out_file=sys.argv[3]),
      M.mask_keyspace("?d?d?d?d?d?d?d?d"), M.mask_candidate("?d?l", 259).decode())
"""


def test_without_a_device(tmp_path):
    """A process that sees no device: the scan functions say DWPA_E_NODEV, dwpa_crack_mask DWPA_RC_ERROR, and the two
    host functions still work."""
    hf = tmp_path / "h.hash"
    hf.write_bytes(b"\n".join(S.CHALLENGE_LINES) + b"\n")
    env = {k: v for k, v in os.environ.items() if k not in ("DWPA_CPU_FALLBACK", "ROCR_VISIBLE_DEVICES")}
    env["HIP_VISIBLE_DEVICES"] = NO_DEVICES
    r = subprocess.run([sys.executable, "-c", _NODEV_CHILD, ROOT, str(hf), str(tmp_path / "o.key")], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == [str(L.DWPA_E_NODEV)] * 3 + [str(L.DWPA_RC_ERROR), "100000000", "9z"], r.stdout


NO_DEVICES = ""  # HIP_VISIBLE_DEVICES of the child


# ---------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------
def _cli(capfdbinary, *argv):
    rc = CLI.main(list(argv))
    return rc, capfdbinary.readouterr().out


def test_cli_keyspace(capfdbinary):
    assert _cli(capfdbinary, "--keyspace", "?d?d?d?d?d?d?d?d") == (0, b"100000000\n")
    assert _cli(capfdbinary, "--keyspace", "-1", "?l?d", "?1?1?1?1?1?1?1?1") == (0, b"%d\n" % 36**8)
    assert _cli(capfdbinary, "--keyspace", "-1", "ab", "-2", "?dXY", "pre??x?1?2?l") == (0, b"624\n")
    assert _cli(capfdbinary, "--keyspace", "--hex-charset", "-1", "000aff", "x?1?1") == (0, b"9\n")
    assert _cli(capfdbinary, "--keyspace", "unused.hash", "?a?a") == (0, b"9025\n")  # a hash file is allowed, not read
    assert _cli(capfdbinary, "--keyspace", "-i", "--increment-min", "2", "--increment-max", "3", "?d?d?l?l") == \
        (0, b"%d\n" % (100 + 2600))
    assert _cli(capfdbinary, "--keyspace", "-i", "?d?d?l") == (0, b"%d\n" % (10 + 100 + 2600))


def test_cli_stdout(capfdbinary):
    custom = (b"ab", b"?dXY")
    sets, k = ref_sets(b"pre??x?1?2?l", custom)
    every = [ref_candidate(sets, i) for i in range(k)]
    args = ("--stdout", "-1", "ab", "-2", "?dXY", "pre??x?1?2?l")
    assert _cli(capfdbinary, *args) == (0, b"".join(c + b"\n" for c in every))
    assert _cli(capfdbinary, *args, "-s", "37", "-l", "130") == (0, b"".join(c + b"\n" for c in every[37:167]))
    assert _cli(capfdbinary, *args, "--skip", "600", "--limit", "100") == (0, b"".join(c + b"\n" for c in every[600:]))
    assert _cli(capfdbinary, *args, "-s", "623") == (0, every[623] + b"\n")
    rc, out = _cli(capfdbinary, "--stdout", "-i", "-1", "01", "?1?1?d")
    assert rc == 0 and out.split(b"\n")[:-1] == [b"0", b"1", b"00", b"01", b"10", b"11"] + \
        [b"%d%d%d" % (a, b, c) for a in (0, 1) for b in (0, 1) for c in range(10)]
    rc, out = _cli(capfdbinary, "--stdout", "--hex-charset", "-1", "00ff0a", "?1?1")
    assert rc == 0 and out == b"".join(bytes([a, b]) + b"\n" for a in (0, 255, 10) for b in (0, 255, 10))


@pytest.mark.parametrize("argv", [["--keyspace", "?x"], ["--keyspace", "?1"], ["--stdout", "?d", "-s", "10"],
                                  ["--keyspace"], ["?d?d?d?d?d?d?d?d"], ["--keyspace", "a", "b", "c"],
                                  ["--stdout", "-s", "-1", "?d"], ["--stdout", "-i", "-s", "1", "?d?d"],
                                  ["--keyspace", "--increment-min", "2", "?d?d"], ["--keyspace", "?b?b?b?b?b?b?b?b"],
                                  ["--keyspace", "-i", "--increment-min", "3", "--increment-max", "2", "?d?d?d"],
                                  ["--keyspace", "--hex-charset", "-1", "0g", "?1"], ["--nope", "--keyspace", "?d"]])
def test_cli_bad_arguments(capfdbinary, argv):
    rc, out = _cli(capfdbinary, *argv)
    assert rc == 255 and out == b""


def test_cli_as_a_module():
    """python -m dwpa_amd.mask: the exit status is the return code (255 = hashcat's -1)."""
    r = subprocess.run([sys.executable, "-m", "dwpa_amd.mask", "--keyspace", "-1", "?l?d", "?1?1?1?1?1?1?1?1"], cwd=ROOT,
                       capture_output=True, timeout=60)
    assert (r.returncode, r.stdout) == (0, b"%d\n" % 36**8)
    r = subprocess.run([sys.executable, "-m", "dwpa_amd.mask", "--keyspace", "?d?"], cwd=ROOT, capture_output=True,
                       timeout=60)
    assert r.returncode == 255 and r.stdout == b"" and b"dwpa_amd.mask" in r.stderr


# ---------------------------------------------------------------------------------------------------------------
# the fuzz target
# ---------------------------------------------------------------------------------------------------------------
def test_mask_language_under_asan():
    """tools/mask_fuzz.cpp: mask.cpp alone (host code, a stand-alone program) under AddressSanitizer + UBSan over
    50,000 random and mutated masks and custom sets; an out-of-bounds access or UB aborts the binary."""
    subprocess.run(["make", "-s", "-C", ROOT, "tools/bin/mask_fuzz_asan"], check=True)
    r = subprocess.run([os.path.join(ROOT, "tools", "bin", "mask_fuzz_asan"), "50000"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    import json
    st = json.loads(r.stdout)
    assert st["masks_parsed"] > 2000 and st["refused"] > 2000 and st["candidates"] == 5 * st["masks_parsed"], st
