"""CPU: the chain attack on the host -- the command line (python -m dwpa_amd.chain: --stdout, --keyspace and the
refusals), dwpa_chain_keyspace / dwpa_chain_split against Python integers, the no-device answers of the device entry
points and the exported names.  The reference is itertools.product over the parts, a mask part expanded by
tests/test_mask.py's reference expander."""
import ctypes
import gzip
import itertools
import os
import subprocess
import sys

import pytest

import dwpa_amd
from dwpa_amd import _lib as L
from dwpa_amd import chain as CLI
from dwpa_amd import m22000 as M
from tests import synth as S
from tests.test_mask import NO_DEVICES, ref_candidate, ref_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BINARY = bytes([0x00, 0x0a, 0xff, 0x41])  # travels as $HEX[]: it holds a line feed
A = [b"alpha", b"", b"p@ss word", BINARY, b"L" * 300, b"\xfe\x01\x80", b"last-no-newline"]  # plain, no last newline
B = [b"second", b"caf\xc3\xa9", b"", b"crlf", b"\x7f\xff"]                                   # gzip, CRLF
C = [b"-", b"", b"_x_"]
D = [b"only"]                                                                                # radix 1
M1 = (b"?d?1", (b"xy",))   # 20
M2 = (b"a?2", (None, b"\x00\xff!"))  # a literal and a custom set of binary bytes: 3
CUSTOM = (b"xy", b"\x00\xff!")


def _files(tmp_path):
    paths = {}
    text = [b"$HEX[" + w.hex().encode() + b"]" if w == BINARY else w for w in A]
    (tmp_path / "a.txt").write_bytes(b"\n".join(text))
    with gzip.open(tmp_path / "b.txt.gz", "wb") as f:
        f.write(b"".join(w + b"\r\n" for w in B))
    (tmp_path / "c.txt").write_bytes(b"".join(w + b"\n" for w in C))
    (tmp_path / "d.txt").write_bytes(b"only\n")
    for k, name in (("A", "a.txt"), ("B", "b.txt.gz"), ("C", "c.txt"), ("D", "d.txt")):
        paths[k] = "list:" + str(tmp_path / name)
    return paths


LISTS = {"A": A, "B": B, "C": C, "D": D}
MASKS = {"M1": b"?d?1", "M2": b"a?2"}


def _choices(name):
    """Every choice of a part, in order."""
    if name in LISTS:
        return LISTS[name]
    sets, k = ref_sets(MASKS[name], CUSTOM)
    return [ref_candidate(sets, i) for i in range(k)]


def _argv(paths, shape):
    return [paths[n] if n in LISTS else "mask:" + os.fsdecode(MASKS[n]) for n in shape]


def _expected(shape, skip=0, limit=0):
    every = [b"".join(t) for t in itertools.product(*[_choices(n) for n in shape])]
    return every[skip:skip + limit if limit else None]


def _cli(capfdbinary, *argv):
    rc = CLI.main(list(argv))
    cap = capfdbinary.readouterr()
    return rc, cap.out, cap.err


SHAPES = [("A",), ("M1",), ("A", "B", "M1"), ("M1", "A", "M2"), ("A", "M2", "B", "C"), ("A", "B", "C", "D"),
          ("D", "M1"), ("C", "C")]


@pytest.mark.parametrize("shape", SHAPES, ids="-".join)
def test_stdout_is_the_product(capfdbinary, tmp_path, shape):
    paths = _files(tmp_path)
    sets = ["--hex-charset", "-1", b"xy".hex(), "-2", "00ff21"]
    rc, out, _ = _cli(capfdbinary, "--stdout", *sets, *_argv(paths, shape))
    exp = _expected(shape)
    assert (rc, out) == (0, b"".join(c + b"\n" for c in exp))
    k = len(exp)
    rc, out, _ = _cli(capfdbinary, "--keyspace", *sets, *_argv(paths, shape))
    assert (rc, out.split()) == (0, [b"%d" % k])
    # unfiltered: the 300-byte line and the empty words are there
    if "A" in shape:
        assert any(len(c) >= 300 for c in exp)
    for skip, limit in ((0, 1), (k - 1, 0), (k - 1, 1), (k - 1, 5), (1, k - 2), (k // 3, k // 2), (0, k), (0, k + 7)):
        rc, out, _ = _cli(capfdbinary, "--stdout", "-s", str(skip), "-l", str(limit), *sets, *_argv(paths, shape))
        assert (rc, out) == (0, b"".join(c + b"\n" for c in _expected(shape, skip, limit))), (skip, limit)


def test_stdout_agrees_with_chain_candidate(tmp_path):
    parts = [A, ("mask", b"a?2"), B]
    exp = _expected(("A", "M2", "B"))
    assert [M.chain_candidate(parts, i, CUSTOM) for i in range(len(exp))] == exp
    with pytest.raises(L.DwpaError):
        M.chain_candidate(parts, len(exp), CUSTOM)


def test_as_a_module(tmp_path):
    paths = _files(tmp_path)
    r = subprocess.run([sys.executable, "-m", "dwpa_amd.chain", "--stdout", "-s", "3", "-l", "40", paths["C"],
                        "mask:?d", paths["B"]], cwd=ROOT, capture_output=True, timeout=60)
    every = [b"".join(t) for t in itertools.product(C, [b"%d" % v for v in range(10)], B)]
    assert (r.returncode, r.stdout) == (0, b"".join(c + b"\n" for c in every[3:43]))
    r = subprocess.run([sys.executable, "-m", "dwpa_amd.chain", "--keyspace", "nolist"], cwd=ROOT,
                       capture_output=True, timeout=60)
    assert r.returncode == 255 and r.stdout == b"" and b"dwpa_amd.chain" in r.stderr


# ---------------------------------------------------------------------------------------------------------------
# keyspace and split against Python integers
# ---------------------------------------------------------------------------------------------------------------
F64 = [3, 5, 17, 257, 641, 65537, 6700417]  # the prime factors of 2^64 - 1
RADICES = [
    [2**64 - 1], [2**32 - 1, 2**32 + 1], [3 * 5 * 17 * 257, 641, 65537, 6700417], [65537 * 6700417, 641 * 257, 255],
    [1], [1, 1, 1, 1], [1, 2**64 - 1, 1], [7, 1, 9], [10, 10, 10, 10], [3, 10**10], [2**32 - 1, 2**32 - 1],
    [2**16, 2**16, 2**16, 2**16 - 1], [68, 19, 100], [2, 3, 5, 7],
]
REFUSED = [[2**64], [2**32, 2**32], [2**16, 2**16, 2**16, 2**16], [2**63, 2], [2**64 - 1, 2], [3, 2**64 - 1, 1],
           [2**32 + 1, 2**32], [], [1, 1, 1, 1, 1], [2, 2, 2, 2, 2]]
ZERO = [[0], [0, 5], [5, 0, 7], [2**64 - 1, 2**64 - 1, 0], [0, 0, 0, 0]]


def _split(radices, i):
    digits = []
    for r in reversed(radices):
        i, d = divmod(i, r)
        digits.append(d)
    assert i == 0
    return digits[::-1]


def test_the_radix_cases():
    prod = 1
    for f in F64:
        prod *= f
    assert prod == 2**64 - 1
    ks = []
    for r in RADICES:
        k = 1
        for v in r:
            k *= v
        ks.append(k)
    assert ks.count(2**64 - 1) >= 4 and max(ks) == 2**64 - 1 and 1 in ks
    for r in REFUSED:
        k = 1
        for v in r:
            k *= v
        assert k >= 2**64 or not 1 <= len(r) <= 4
    assert 2**32 * 2**32 == 2**64 and [2**32, 2**32] in REFUSED  # exactly 2^64


@pytest.mark.parametrize("radices", RADICES, ids=lambda r: "x".join("%x" % v for v in r))
def test_keyspace_and_split(radices):
    k = 1
    for v in radices:
        k *= v
    assert M.chain_keyspace(radices) == k
    for i in sorted({0, 1 % k, k // 2, k // 3 + 1 if k > 3 else 0, k - 1, min(k - 1, 2**32), min(k - 1, 2**32 - 1)}):
        assert M.chain_split(radices, i) == _split(radices, i), i
        d = M.chain_split(radices, i)
        assert all(0 <= x < r for x, r in zip(d, radices))
    with pytest.raises(L.DwpaError) as e:
        M.chain_split(radices, k)  # index K
    assert e.value.code == L.DWPA_E_ARG
    if k < 2**64 - 1:
        with pytest.raises(L.DwpaError):
            M.chain_split(radices, 2**64 - 1)


@pytest.mark.parametrize("radices", REFUSED, ids=lambda r: "x".join("%x" % v for v in r) or "none")
def test_keyspace_refused(radices):
    for call in (lambda: M.chain_keyspace(radices), lambda: M.chain_split(radices, 0)):
        with pytest.raises(L.DwpaError) as e:
            call()
        assert e.value.code == L.DWPA_E_ARG


@pytest.mark.parametrize("radices", ZERO, ids=lambda r: "x".join("%x" % v for v in r))
def test_a_radix_of_zero_is_an_empty_keyspace(radices):
    assert M.chain_keyspace(radices) == 0
    with pytest.raises(L.DwpaError) as e:
        M.chain_split(radices, 0)  # every index is >= K
    assert e.value.code == L.DWPA_E_ARG


def test_null_pointers_are_refused():
    lib = L.load()
    r = (ctypes.c_uint64 * 2)(3, 4)
    k = ctypes.c_uint64(0)
    assert lib.dwpa_chain_keyspace(None, 2, ctypes.byref(k)) == L.DWPA_E_ARG
    assert lib.dwpa_chain_keyspace(r, 2, None) == 0  # only the check
    assert lib.dwpa_chain_split(r, 2, 0, None) == L.DWPA_E_ARG


# ---------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------
def _bad(tmp_path):
    p = _files(tmp_path)
    a, b = p["A"], p["B"]
    missing = "list:" + str(tmp_path / "missing.txt")
    return [["h.hash"],                                        # no part
            ["--stdout"],
            ["--keyspace"],
            [],
            ["h.hash", a, b, a, b, a],                         # five parts
            ["--stdout", a, b, a, b, a],
            ["--keyspace", "mask:?d", "mask:?d", "mask:?d", "mask:?d", "mask:?d"],
            ["h.hash", a[5:]],                                 # a part without a prefix
            ["--stdout", a, "?d?d"],
            ["--stdout", "dict:" + a[5:]],
            ["h.hash", a, missing],                            # a missing list
            ["--stdout", missing, a],
            ["--keyspace", a, missing],
            ["h.hash", a, "mask:?x"],                          # a bad mask
            ["--stdout", "mask:?1", a],                        # ?1 is not defined
            ["--stdout", "mask:", a],
            ["--keyspace", "mask:" + "?d" * 64],
            ["--stdout", "mask:?b?b?b?b", "mask:?b?b?b?b"],    # 2^64
            ["--keyspace", "mask:?b?b?b?b", "mask:?b?b?b?b"],
            ["h.hash", "mask:?b?b?b?b", "mask:?b?b?b?b"],
            ["--stdout", "-s", "35", a, b],                    # skip >= K
            ["--stdout", "-s", "36", "-l", "1", a, b],
            ["--stdout", "-s", "-1", a, b],
            ["--stdout", "-l", "-1", a, b],
            ["--stdout", "--hex-charset", "-1", "xyz", "mask:?1", a],
            ["--stdout", "-d", "0", "--bogus", a]]


@pytest.mark.parametrize("case", range(26))
def test_bad_invocations(capfdbinary, tmp_path, case):
    """Each exits 255 with nothing on stdout and a message on stderr (no device is needed to refuse any of them)."""
    cases = _bad(tmp_path)
    assert len(cases) == 26
    rc, out, err = _cli(capfdbinary, *cases[case])
    assert rc == 255 and out == b"" and err.strip()


def test_the_last_index_is_not_refused(capfdbinary, tmp_path):
    p = _files(tmp_path)
    rc, out, _ = _cli(capfdbinary, "--stdout", "-s", "34", p["A"], p["B"])
    assert (rc, out) == (0, A[-1] + B[-1] + b"\n")


def test_an_empty_list_is_an_empty_keyspace(capfdbinary, tmp_path):
    p = _files(tmp_path)
    (tmp_path / "empty.txt").write_bytes(b"")
    e = "list:" + str(tmp_path / "empty.txt")
    assert _cli(capfdbinary, "--keyspace", p["A"], e, "mask:?b?b?b?b?b?b?b?a")[:2] == (0, b"0\n")
    assert _cli(capfdbinary, "--stdout", p["A"], e)[:2] == (0, b"")


def test_exported_names():
    assert (dwpa_amd.DWPA_CHAIN_LIST, dwpa_amd.DWPA_CHAIN_MASK, dwpa_amd.DWPA_CHAIN_MAX_PARTS) == (0, 1, 4)
    assert callable(dwpa_amd.crack_chain) and callable(dwpa_amd.Scan.set_chain) and callable(dwpa_amd.Scan.load_chain)
    for name in ("crack_chain", "chain_keyspace", "chain_split", "chain_candidate", "DWPA_CHAIN_LIST",
                 "DWPA_CHAIN_MASK", "DWPA_CHAIN_MAX_PARTS"):
        assert name in dwpa_amd.__all__ and hasattr(dwpa_amd, name)
    lib = L.load()
    assert lib.dwpa_scan_set_chain and lib.dwpa_scan_load_chain and lib.dwpa_crack_chain
    assert lib.dwpa_chain_keyspace and lib.dwpa_chain_split and lib.dwpa_abi_version() == 4
    with open(L.HEADER) as f:
        header = f.read()
    for name in ("dwpa_scan_set_chain", "dwpa_scan_load_chain", "dwpa_crack_chain", "dwpa_chain_keyspace",
                 "dwpa_chain_split", "dwpa_chain_part", "dwpa_chain_spec", "DWPA_CHAIN_MAX_PARTS 4"):
        assert name in header, name


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
hf, out, d, missing = sys.argv[2:6]
part = (L.ChainPart * 1)()
part[0].kind, part[0].mask, part[0].mask_len = L.DWPA_CHAIN_MASK, b"?d", 2
k = ctypes.c_uint64(0)
print(lib.dwpa_device_count(), lib.dwpa_scan_set_chain(None, part, 1, None, ctypes.byref(k)),
      lib.dwpa_scan_load_chain(None, 0, 1, 8, 63, None), lib.dwpa_scan_load_chain(None, 0, 0, 8, 63, None))
LIST, MASK = L.DWPA_CHAIN_LIST, L.DWPA_CHAIN_MASK
for hash_file, parts in ((hf, [(LIST, d), (MASK, "?d?d?d")]), (hf, [(MASK, "?d?d?d?d?d?d?d?d")]),
                         (hf, [(LIST, missing), (LIST, d)]), (hf, [(LIST, d), (MASK, "?d"), (LIST, missing)]),
                         (hf, [(LIST, missing), (MASK, "?x"), (LIST, missing), (LIST, d)]),
                         (hf, [(LIST, d), (MASK, "?x")]), (hf, [(7, d)]), (hf, []), (hf, [(LIST, d)] * 5),
                         (hf, [(MASK, "?b?b?b?b"), (MASK, "?b?b?b?b")]), (missing, [(LIST, d), (MASK, "?d?d?d")])):
    rc, st = dwpa_amd.crack_chain(hash_file, parts, out_file=out)
    print(rc, *st)
rc, st = dwpa_amd.crack_chain(hf, [(LIST, d), (MASK, "?d?d?d")], skip=2000, out_file=out)
print(rc, *st)
print(M.crack_stats()["candidates"], dwpa_amd.chain_keyspace([2, 1000]), *dwpa_amd.chain_split([2, 1000], 1999))
"""


def test_without_a_device(tmp_path):
    """A process that sees no device: dwpa_scan_set_chain / dwpa_scan_load_chain say DWPA_E_NODEV, dwpa_crack_chain
    DWPA_RC_ERROR; every unreadable list is marked DWPA_E_IO in its own part_status entry (whatever else is wrong with
    the call) with the others DWPA_DICT_OK; the two host functions still work; no outfile is created."""
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
        [nodev] * 4, [err, ok, ok], [err, ok], [err, io, ok], [err, ok, ok, io], [err, io, ok, io, ok],
        [err, ok, ok], [err, ok], [err], [err] + [ok] * 5, [err, ok, ok], [err, ok, ok], [err, ok, ok],
        ["0", "2000", "1", "999"]], r.stdout
    assert not (tmp_path / "o.key").exists()  # refused before the outfile is opened
