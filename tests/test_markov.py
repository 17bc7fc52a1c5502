"""CPU: the Markov-ordered mask attack on the host (dwpa_amd/csrc/markov.cpp): the trainer, the model file and its
loader, the thresholded keyspace, candidate i, the command lines (python -m dwpa_amd.markov, python -m dwpa_amd.mask
--markov / -t), the no-device answers and the fuzz target.

The reference below is independent of the library: train -> counts -> ranking -> candidate, written from the rules in
include/dwpa22000.h ("mask attack in Markov order").  The mask language comes from tests/test_mask.py."""
import ctypes
import gzip
import os
import random
import subprocess
import sys

import pytest

import dwpa_amd
from dwpa_amd import _lib as L
from dwpa_amd import m22000 as M
from dwpa_amd import markov as MCLI
from dwpa_amd import mask as CLI
from tests import synth as S
from tests.test_mask import RAW, _tokens, ref_candidate, ref_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = b"DWPAMKV1" + (63).to_bytes(4, "little") + (0).to_bytes(4, "little")
IDENTITY = bytes(range(256))


# ---------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------
def ref_counts(words):
    """{(p, a): {b: n}} over the words' first 63 bytes; the predecessor of position 0 is byte 0."""
    n = {}
    for w in words:
        prev = 0
        for p, b in enumerate(w[:63]):
            row = n.setdefault((p, prev), {})
            row[b] = row.get(b, 0) + 1
            prev = b
    return n


def ref_order(n, p, a):
    """The 256 bytes by count descending, ties by value ascending."""
    row = n.get((p, a))
    return IDENTITY if not row else bytes(sorted(range(256), key=lambda b: (-row.get(b, 0), b)))


def ref_image(n):
    return HEADER + b"".join(ref_order(n, p, a) for p in range(63) for a in range(256))


def mk_sets(mask, custom=()):
    """ref_sets without its keyspace limit: a threshold may bring a larger mask under 2^64."""
    custom = list(custom) + [None] * (4 - len(custom))
    cs = [None] * 4
    for k, c in enumerate(custom):
        if c is not None:
            cs[k] = bytes(dict.fromkeys(b"".join(_tokens(c, cs, k))))
    return [bytes(dict.fromkeys(t)) for t in _tokens(mask, cs, 4)]


def ref_radices(sets, t):
    return [len(s) if t == 0 else min(len(s), t) for s in sets]


def ref_keyspace(sets, t):
    k = 1
    for r in ref_radices(sets, t):
        k *= r
    return k


def ref_markov(n, sets, t, i):
    """Candidate i: digits over the radices, last position fastest; each digit picks from the ranking after the byte
    before it, filtered to the position's set."""
    rad = ref_radices(sets, t)
    digits = [0] * len(sets)
    for p in range(len(sets) - 1, -1, -1):
        i, digits[p] = divmod(i, rad[p])
    assert i == 0
    out, prev = bytearray(), 0
    for p, s in enumerate(sets):
        row = [b for b in ref_order(n, p, prev) if b in s][:rad[p]]
        prev = row[digits[p]]
        out.append(prev)
    return bytes(out)


def plain(w):
    """A word as a dictionary line."""
    ok = all(0x20 <= c <= 0x7e for c in w) and not w.startswith(b"$HEX[")
    return w if ok else b"$HEX[" + w.hex().encode() + b"]"


# ---------------------------------------------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------------------------------------------
EXAMPLE_WORDS = [b"abba", b"abab", b"baba", b"bbbb", b"abbb", b"ba"]


def _train_words():
    """Letters, digits and the raw bytes 0x00 0x0a 0x7f 0x80 0xff, so that each of those is ranked high somewhere,
    both as the byte chosen and as the byte before; ties (many counts of 1) and rows never seen; one 100-byte word."""
    rng = random.Random(0x3a7)
    alpha = RAW[:5] * 6 + b"abcdeXY0123456789lmnopq" + b"prex?"
    words = [bytes(rng.choice(alpha) for _ in range(rng.randint(1, 14))) for _ in range(500)]
    words += [bytes(rng.choice(RAW[:5]) for _ in range(8)) for _ in range(60)]
    words += [b"pre?x" + bytes(rng.choice(b"abXY0123") for _ in range(3)) for _ in range(40)]
    words.append(bytes(rng.choice(b"hHlr5z~") for _ in range(100)))
    words += [bytes([0x80] * 12), bytes([0xff, 0x00] * 6)]
    return words


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    d = tmp_path_factory.mktemp("markov")
    words = _train_words()
    path = d / "words.txt"
    path.write_bytes(b"".join(plain(w) + b"\n" for w in words))
    out = d / "m.dwmk"
    assert M.markov_train([str(path)], str(out)) == len(words)
    n = ref_counts(words)
    img = M.markov_load(str(out))
    return {"n": n, "img": img, "path": str(out), "words": words, "list": str(path), "dir": d}


def test_the_trained_file_is_the_reference_image(model):
    img, n = model["img"], model["n"]
    assert len(img) == L.DWPA_MARKOV_BYTES == 16 + 63 * 256 * 256 == 4128784
    assert img == ref_image(n)
    for at in range(16, len(img), 256):
        assert sorted(img[at:at + 256]) == list(range(256))
    # the model has what the cases below need: rankings that differ between two predecessors at one position and
    # between two positions for one predecessor, ties broken by value, and unseen rows in byte order
    assert ref_order(n, 1, ord("a")) != ref_order(n, 1, ord("b")) != IDENTITY
    assert ref_order(n, 1, ord("a")) != ref_order(n, 2, ord("a"))
    assert ref_order(n, 1, 0x00) != ref_order(n, 0, 0x00), "byte 0 as a real predecessor has a row of its own"
    assert ref_order(n, 40, ord("a")) == IDENTITY and any(ref_order(n, 62, a) != IDENTITY for a in b"hHlr5z~")
    assert not any(p > 62 for p, a in n)
    row = n[(3, ord("a"))]
    tied = [b for b in row if list(row.values()).count(row[b]) > 1]
    assert tied, "no tie in the row"
    assert MCLI.row(img, 1, 0x80) == ref_order(n, 1, 0x80) != IDENTITY


# (mask, custom, thresholds)
LONG = b"?h?H" + b"l" * 29 + b"?s?u" + b"r" * 28 + b"?d?l"
WRAP = (b"?d?dA?dB?d?dC?dD?1?2?3?4", (b"ab", b"cde", b"fghij", b"klmnopq"))
CASES = [
    (b"pre??x?1?2?l", (b"ab", b"?dXY"), (0, 1, 2, 3, 11, 12, 13, 25, 26, 27, 256)),  # n_p = 2, 12, 26
    (WRAP[0], WRAP[1], (0, 1, 2, 4, 6, 7, 8, 9, 10, 11, 256)),  # literals at byte lanes 2, 1, 0, 3, and as predecessors
    (b"?1?1?1", (RAW,), (0, 1, 2, 5, 6, 7, 256)),               # the raw bytes chosen and as predecessors
    (b"?b?1?b", (RAW,), (0, 1, 2, 255, 256)),
    (b"?b?b?b", (), (0, 3, 255, 256)),
    (b"\x00\xff?b\n\x80?b\x7f?b", (), (0, 1, 7, 256)),           # literal 0x00 0xff 0x0a 0x80 0x7f before a set
    (b"?d" * 8, (), (0, 1, 9, 10, 11)),
    (LONG, (), (0, 1, 3, 16, 256)),                             # 63 positions
    (b"?a" * 12, (), (10, 1)),                                  # 95^12 is above 2^64, 10^12 is not
    (b"?b?b?b?b?b?b?b?a", (), (0, 255, 256, 94, 95, 96)),       # just under 2^64
    (b"x", (), (0, 1, 256)), (b"?l", (), (0, 1, 25, 26, 27)),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_keyspace_and_candidates_equal_the_reference(model, case):
    mask, custom, thresholds = CASES[case]
    sets, n, img = mk_sets(mask, custom), model["n"], model["img"]
    rng = random.Random(case)
    for t in thresholds:
        k = ref_keyspace(sets, t)
        assert k < 2**64
        if t:
            assert M.mask_keyspace(mask, custom, threshold=t) == k and M.mask_positions(mask, custom, t) == len(sets)
        idx = list(range(k)) if k <= 1000 else [0, k - 1] + [rng.randrange(k) for _ in range(998)]
        got = M.mask_candidates(mask, idx, custom, img, t)
        assert len(got) == len(idx)
        for i, g in zip(idx, got):
            assert g == ref_markov(n, sets, t, i), (mask, t, i)
        for i in idx[:3]:
            assert M.mask_candidate(mask, i, custom, markov=img, threshold=t) == ref_markov(n, sets, t, i)
        for bad in (k, 2**64 - 1) if k < 2**64 - 1 else (k,):
            with pytest.raises(L.DwpaError) as e:
                M.mask_candidate(mask, bad, custom, markov=img, threshold=t)
            assert e.value.code == L.DWPA_E_ARG


@pytest.mark.parametrize("case", [0, 2, 11])
def test_candidate_sets(model, case):
    """t = 0: the plain mask's candidates in another order.  t > 0: a subset, no candidate twice."""
    mask, custom, thresholds = CASES[case]
    sets, k = ref_sets(mask, custom)
    every = sorted(ref_candidate(sets, i) for i in range(k))
    assert sorted(M.mask_candidates(mask, range(k), custom, model["img"], 0)) == every
    assert M.mask_keyspace(mask, custom, threshold=0) == M.mask_keyspace(mask, custom) == k
    for t in thresholds:
        kt = ref_keyspace(sets, t)
        got = M.mask_candidates(mask, range(kt), custom, model["img"], t)
        assert len(set(got)) == kt and set(got) <= set(every)


def test_the_worked_example(tmp_path):
    """Words abba abab baba bbbb abbb ba, mask ?1?1?2 with -1 ab -2 abc."""
    (tmp_path / "w").write_bytes(b"\n".join(EXAMPLE_WORDS) + b"\n")
    assert M.markov_train([str(tmp_path / "w")], str(tmp_path / "m")) == 6
    img = M.markov_load(str(tmp_path / "m"))
    assert img == ref_image(ref_counts(EXAMPLE_WORDS))
    custom = (b"ab", b"abc")

    def every(t):
        k = M.mask_keyspace(b"?1?1?2", custom, threshold=t)
        return b" ".join(M.mask_candidates(b"?1?1?2", range(k), custom, img, t))

    assert every(0) == b"abb aba abc aab aaa aac bab baa bac bbb bba bbc"
    assert every(2) == b"abb aba aab aaa bab baa bbb bba"
    assert every(1) == b"abb"
    n = ref_counts(EXAMPLE_WORDS)
    sets = mk_sets(b"?1?1?2", custom)
    assert [ref_markov(n, sets, 2, i) for i in range(8)] == every(2).split()


def test_argument_errors(model):
    img = model["img"]
    for call in (lambda: M.mask_keyspace(b"?d", threshold=257), lambda: M.mask_candidate(b"?d", 0, markov=img, threshold=257),
                 lambda: M.mask_keyspace(b"?a" * 12, threshold=96), lambda: M.mask_keyspace(b"?b" * 9, threshold=256),
                 lambda: M.mask_candidate(b"?d", 0, threshold=2), lambda: M.mask_keyspace(b"?x", threshold=3),
                 lambda: M.mask_candidate(b"?d", 0, markov=img[:-1]), lambda: M.mask_candidate(b"?d", 0, markov=b"")):
        with pytest.raises(L.DwpaError) as e:
            call()
        assert e.value.code == L.DWPA_E_ARG
    lib = L.load()
    k, n = ctypes.c_uint64(7), ctypes.c_uint32(7)
    assert lib.dwpa_mask_keyspace_markov(b"?d?l", 4, None, 5, ctypes.byref(n), ctypes.byref(k)) == 0
    assert (n.value, k.value) == (2, 25)
    assert lib.dwpa_mask_keyspace_markov(b"?d?l", 4, None, 5, None, None) == 0
    assert lib.dwpa_mask_keyspace_markov(None, 0, None, 5, None, None) == L.DWPA_E_ARG
    out = ctypes.create_string_buffer(b"\xaa" * 64, 64)
    assert lib.dwpa_mask_candidate_markov(b"?d?d", 4, None, None, 0, 0, 0, out, ctypes.byref(n)) == L.DWPA_E_ARG
    assert lib.dwpa_mask_candidate_markov(b"?d?d", 4, None, img, len(img), 0, 0, None, ctypes.byref(n)) == L.DWPA_E_ARG
    assert lib.dwpa_mask_candidate_markov(b"?d?d", 4, None, img, len(img), 0, 42, out, ctypes.byref(n)) == 0
    assert n.value == 2 and out.raw[2:] == bytes(62) and out.raw[:2] == ref_markov(model["n"], mk_sets(b"?d?d"), 0, 42)


# ---------------------------------------------------------------------------------------------------------------
# the trainer and the loader
# ---------------------------------------------------------------------------------------------------------------
def test_trainer(model, tmp_path):
    words, base = model["words"], open(model["path"], "rb").read()
    text = b"".join(plain(w) + b"\n" for w in words)

    def train(*paths):
        out = tmp_path / "o.dwmk"
        n = M.markov_train([str(p) for p in paths], str(out))
        return n, out.read_bytes()

    (tmp_path / "w.gz").write_bytes(gzip.compress(text))
    assert train(tmp_path / "w.gz") == (len(words), base), "a gzip copy"
    assert train(model["list"]) == (len(words), base), "a second run"
    half = len(words) // 2
    (tmp_path / "a").write_bytes(b"".join(plain(w) + b"\n" for w in words[:half]))
    (tmp_path / "b.gz").write_bytes(gzip.compress(b"".join(plain(w) + b"\n" for w in words[half:])))
    assert train(tmp_path / "a", tmp_path / "b.gz") == (len(words), base), "two lists = their concatenation"
    # CRLF, empty lines, $HEX[] for every word, no newline at the end
    crlf = b"\r\n\r\n".join(b"$HEX[" + w.hex().encode() + b"]" for w in words)
    (tmp_path / "c").write_bytes(b"\n" + crlf)
    assert train(tmp_path / "c") == (len(words), base)
    # a 100-byte word counts as its first 63 bytes
    long = [w for w in words if len(w) == 100]
    assert long
    (tmp_path / "d").write_bytes(b"".join(plain(w[:63]) + b"\n" for w in words))
    assert train(tmp_path / "d") == (len(words), base)
    assert any(model["n"].get((62, a)) for a in range(256)) and base == ref_image(ref_counts(words))


def test_trainer_errors(model, tmp_path):
    out = tmp_path / "o.dwmk"
    with pytest.raises(L.DwpaError) as e:
        M.markov_train([str(tmp_path / "missing")], str(out))
    assert e.value.code == L.DWPA_E_IO and not out.exists()
    gz = gzip.compress(b"".join(plain(w) + b"\n" for w in model["words"]) * 20)
    (tmp_path / "cut.gz").write_bytes(gz[:len(gz) // 2])
    lib = L.load()
    arr = (ctypes.c_char_p * 1)(str(tmp_path / "cut.gz").encode())
    words = ctypes.c_uint64(0)
    assert lib.dwpa_markov_train(arr, 1, str(out).encode(), ctypes.byref(words)) == L.DWPA_E_IO
    assert words.value > 0 and not out.exists(), "counted up to the damage, no file written"
    with pytest.raises(L.DwpaError) as e:
        M.markov_train([model["list"]], str(tmp_path / "no" / "such" / "dir.dwmk"))
    assert e.value.code == L.DWPA_E_IO
    assert lib.dwpa_markov_train(None, 0, str(out).encode(), None) == L.DWPA_E_ARG


def test_loader_refuses(model, tmp_path):
    img = model["img"]
    twice = bytearray(img)
    at = 16 + (5 * 256 + 0x61) * 256
    twice[at + 7] = twice[at + 8]
    for name, data, code in (("short", img[:-1], L.DWPA_E_ARG), ("long", img + b"\0", L.DWPA_E_ARG),
                             ("header", b"DWPAMKV2" + img[8:], L.DWPA_E_ARG),
                             ("positions", img[:8] + (62).to_bytes(4, "little") + img[12:], L.DWPA_E_ARG),
                             ("twice", bytes(twice), L.DWPA_E_ARG), ("empty", b"", L.DWPA_E_ARG)):
        p = tmp_path / name
        p.write_bytes(data)
        with pytest.raises(L.DwpaError) as e:
            M.markov_load(str(p))
        assert e.value.code == code, name
        assert L.load().dwpa_markov_check(data, len(data)) == L.DWPA_E_ARG
    with pytest.raises(L.DwpaError) as e:
        M.markov_load(str(tmp_path / "missing"))
    assert e.value.code == L.DWPA_E_IO
    assert L.load().dwpa_markov_check(img, len(img)) == 0
    with pytest.raises(L.DwpaError) as e:
        M.mask_candidate(b"?d", 0, markov=bytes(twice))
    assert e.value.code == L.DWPA_E_ARG


# ---------------------------------------------------------------------------------------------------------------
# the command lines
# ---------------------------------------------------------------------------------------------------------------
def _cli(capfdbinary, *argv, main=CLI.main):
    rc = main(list(argv))
    return rc, capfdbinary.readouterr().out


def test_cli_keyspace(capfdbinary, model):
    assert _cli(capfdbinary, "--keyspace", "-t", "10", "?l?l?l?l?l?l?l?l") == (0, b"100000000\n")
    assert _cli(capfdbinary, "--keyspace", "--markov-threshold", "10", "?a" * 12) == (0, b"%d\n" % 10**12)
    assert _cli(capfdbinary, "--keyspace", "-t", "3", "-1", "ab", "-2", "?dXY", "pre??x?1?2?l") == (0, b"18\n")
    assert _cli(capfdbinary, "--keyspace", "--markov", model["path"], "?d?d") == (0, b"100\n")
    assert _cli(capfdbinary, "--keyspace", "-t", "256", "?d?d") == (0, b"100\n")
    assert _cli(capfdbinary, "--keyspace", "-t", "2", "-i", "--increment-min", "2", "?d?d?l?l") == (0, b"%d\n" % (4 + 8 + 16))


def test_cli_stdout(capfdbinary, model):
    custom = (b"ab", b"?dXY")
    sets, n = mk_sets(b"pre??x?1?2?l", custom), model["n"]
    args = ("--stdout", "--markov", model["path"], "-1", "ab", "-2", "?dXY", "pre??x?1?2?l")
    for t in (0, 1, 3, 12):
        every = [ref_markov(n, sets, t, i) for i in range(ref_keyspace(sets, t))]
        targ = ("-t", str(t)) if t else ()
        assert _cli(capfdbinary, *args, *targ) == (0, b"".join(c + b"\n" for c in every))
        if len(every) > 40:
            assert _cli(capfdbinary, *args, *targ, "-s", "7", "-l", "30") == (0, b"".join(c + b"\n" for c in every[7:37]))
    rc, out = _cli(capfdbinary, "--stdout", "--markov", model["path"], "-t", "2", "-i", "-1", "01", "?1?1?d")
    exp = []
    for m in (b"?1", b"?1?1", b"?1?1?d"):
        s = mk_sets(m, (b"01",))
        exp += [ref_markov(n, s, 2, i) for i in range(ref_keyspace(s, 2))]
    assert rc == 0 and out.split(b"\n")[:-1] == exp and len(exp) == 2 + 4 + 8


def test_cli_refusals(capfdbinary, model, tmp_path):
    (tmp_path / "bad.dwmk").write_bytes(model["img"][:100])
    (tmp_path / "w").write_bytes(b"password\n")
    m, w = model["path"], str(tmp_path / "w")
    for argv in (["--stdout", "-t", "2", "?d?d"],                           # candidates without a model
                 ["h.hash", "-t", "2", "?d?d?d?d?d?d?d?d"],
                 ["--keyspace", "-t", "0", "?d"], ["--keyspace", "-t", "257", "?d"], ["--keyspace", "-t", "-1", "?d"],
                 ["--stdout", "--markov", m, "-t", "257", "?d"],
                 ["-a", "6", "--stdout", "--markov", m, w, "?d"], ["-a", "7", "--stdout", "-t", "2", "?d", w],
                 ["-a", "1", "--stdout", "--markov", m, w, w], ["-a", "1", "--stdout", "-t", "2", w, w],
                 ["--stdout", "--markov", str(tmp_path / "bad.dwmk"), "?d"],
                 ["--stdout", "--markov", str(tmp_path / "missing"), "?d"],
                 ["--keyspace", "-t", "96", "?a" * 12], ["--stdout", "--markov", m, "-t", "2", "-s", "4", "?d?d"]):
        rc, out = _cli(capfdbinary, *argv)
        assert rc == 255 and out == b"", argv
    CLI.main(["--stdout", "-t", "2", "?d?d"])
    assert b"dwpa_amd.markov train" in capfdbinary.readouterr().err


def test_cli_markov_module(model, tmp_path):
    """python -m dwpa_amd.markov train / show, as a module: needs no device."""
    out = tmp_path / "m.dwmk"
    r = subprocess.run([sys.executable, "-m", "dwpa_amd.markov", "train", str(out), model["list"]], cwd=ROOT,
                       capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == b"" and out.read_bytes() == model["img"], r.stderr[-2000:]
    r = subprocess.run([sys.executable, "-m", "dwpa_amd.markov", "show", str(out), "-p", "1", "-a", "0x80"], cwd=ROOT,
                       capture_output=True, timeout=120)
    assert r.returncode == 0 and bytes.fromhex(r.stdout.decode()) == ref_order(model["n"], 1, 0x80), r.stderr[-2000:]
    assert MCLI.main(["show", str(out)]) == 0
    for argv in (["show", str(tmp_path / "missing")], ["show", str(out), "-p", "63"], ["show", str(out), "-a", "256"],
                 ["show", str(out), "-a", "x"], ["train", str(out)], ["train", str(out), str(tmp_path / "missing")], []):
        assert MCLI.main(argv) == 255, argv


_NODEV_CHILD = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
import dwpa_amd
from dwpa_amd import _lib as L
from dwpa_amd import m22000 as M
lib = L.load()
img = M.markov_load(sys.argv[4])
k = ctypes.c_uint64(0)
print(lib.dwpa_device_count(),
      lib.dwpa_scan_set_mask_markov(None, b"?d?d", 4, None, img, len(img), 2, ctypes.byref(k)),
      M.crack_mask(sys.argv[2], "?d?d?d?d?d?d?d?d", out_file=sys.argv[3], markov=sys.argv[4], threshold=2),
      M.mask_keyspace("?d?d?d?d?d?d?d?d", threshold=2), M.mask_candidate("?d?l", 3, markov=img, threshold=2).hex())
"""


def test_without_a_device(model, tmp_path):
    """A process that sees no device: the scan function says DWPA_E_NODEV, dwpa_crack_mask_markov DWPA_RC_ERROR, and
    the host functions still work."""
    hf = tmp_path / "h.hash"
    hf.write_bytes(b"\n".join(S.CHALLENGE_LINES) + b"\n")
    env = {k: v for k, v in os.environ.items() if k not in ("DWPA_CPU_FALLBACK", "ROCR_VISIBLE_DEVICES")}
    env["HIP_VISIBLE_DEVICES"] = ""
    r = subprocess.run([sys.executable, "-c", _NODEV_CHILD, ROOT, str(hf), str(tmp_path / "o.key"), model["path"]],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    exp = ref_markov(model["n"], mk_sets(b"?d?l"), 2, 3).hex()
    assert r.stdout.split() == [str(L.DWPA_E_NODEV)] * 2 + [str(L.DWPA_RC_ERROR), "256", exp], r.stdout


# ---------------------------------------------------------------------------------------------------------------
# the fuzz target
# ---------------------------------------------------------------------------------------------------------------
def test_markov_host_code_under_asan():
    """tools/markov_fuzz.cpp: markov.cpp and mask.cpp alone (host code, a stand-alone program) under AddressSanitizer
    + UBSan: random masks, thresholds, model images (valid and damaged) and indices against a second, naive
    implementation in the tool; a difference, an out-of-bounds access or UB fails the binary."""
    subprocess.run(["make", "-s", "-C", ROOT, "tools/bin/markov_fuzz_asan"], check=True)
    r = subprocess.run([os.path.join(ROOT, "tools", "bin", "markov_fuzz_asan"), "3000"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    import json
    st = json.loads(r.stdout)
    assert st["masks_parsed"] > 500 and st["refused"] > 100 and st["damaged_refused"] > 100, st
    assert st["candidates"] > 5 * st["masks_parsed"] and st["tables"] > 100, st
