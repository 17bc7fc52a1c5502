"""CPU: the table attack on the host (dwpa_amd/csrc/table.cpp): the table grammar, the keyspace and the candidates
against the independent reference of tests/table_plan.py, the built-in toggle table, the command line
(python -m dwpa_amd.table --keyspace / --stdout) and the fuzz target."""
import gzip
import itertools
import os
import random
import subprocess
import sys

import pytest

import dwpa_amd
from dwpa_amd import _lib as L
from dwpa_amd import table as CLI
from tests import table_plan as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------
# the grammar
# ---------------------------------------------------------------------------------------------------------------
ACCEPTED = [
    (b"a=b\n", {0x61: b"b"}),
    (b"a=a\na=@\n", {0x61: b"a@"}),                                     # file order
    (b"a=@\na=a", {0x61: b"@a"}),                                       # no newline at the end
    (b"\\x61=\\x40\n\\x00=\\xFF\n\\xfF=\\x00\n", {0x61: b"@", 0x00: b"\xff", 0xff: b"\x00"}),
    (b"===\n", {0x3d: b"="}),
    (b"#=#\n#=a\n", {0x23: b"#a"}),                                     # a mapping, not a comment
    (b"a=b\r\n\r\nc=d\r\n", {0x61: b"b", 0x63: b"d"}),                  # CRLF, and an empty CRLF line
    (b"a=\r\r\n", {0x61: b"\r"}),                                       # one CR is the line end, the other the value
    (b"a=b\na=b\na=c\n", {0x61: b"bc"}),                                # a repeated (K, V) line is ignored
    (b"\\=x\nx=\\\n", {0x5c: b"x", 0x78: b"\\"}),                       # a backslash that starts no \xHH is itself
    (b"\\=\\\n", {0x5c: b"\\"}),
    (b"".join(b"a=%c\n" % v for v in b"0123456789ABCDEF"), {0x61: b"0123456789ABCDEF"}),   # 16 alternatives
    (b"".join(b"a=%c\n" % v for v in b"0123456789ABCDEF") + b"a=3\n", {0x61: b"0123456789ABCDEF"}),  # the 17th repeats
]
REFUSED = [
    (b"", 1), (b"\n\r\n\n", 4),                                         # no mapping at all: the lines + 1
    (b"a=b\nab\n", 2), (b"a=b\n=\n", 2), (b"a\n", 1), (b"a=\n", 1), (b"a=bc\n", 1), (b"ab=c\n", 1),
    (b"a=b\n\na=b=c\n", 3), (b"a=b \n", 1), (b" a=b\n", 1), (b"a=b\n# comment\n", 2), (b"\n\n a= \n", 3),
    (b"\\x6=a\n", 1), (b"\\xg1=a\n", 1), (b"a=\\x4\n", 1), (b"a=\\x41\\x42\n", 1), (b"a=b\r\r\n", 1),
    (b"".join(b"a=%c\n" % v for v in b"0123456789ABCDEFG"), 17),        # a 17th alternative
]


@pytest.mark.parametrize("case", range(len(ACCEPTED)))
def test_grammar_accepted(case):
    text, want = ACCEPTED[case]
    got = dwpa_amd.table_parse(text)
    ref = T.ref_parse(text)
    for c in range(256):
        assert got[c] == ref[c] == want.get(c, bytes([c])), (text, c)  # an unnamed byte stays; a key loses its original


@pytest.mark.parametrize("case", range(len(REFUSED)))
def test_grammar_refused_with_line_number(case):
    text, line = REFUSED[case]
    with pytest.raises(L.DwpaError) as e:
        dwpa_amd.table_parse(text)
    assert e.value.code == L.DWPA_E_ARG and e.value.line == line, text
    with pytest.raises(ValueError) as r:
        T.ref_parse(text)
    assert r.value.args[0] == line, text
    with pytest.raises(L.DwpaError):
        dwpa_amd.table_keyspace(text, [b"password"])


def test_key_without_identity():
    t = b"a=@\na=4\n"
    assert dwpa_amd.table_keyspace(t, [b"banana12"])["keyspace"] == 8
    c = dwpa_amd.table_candidates(t, [b"banana12"], range(8))
    assert c == [b"b@n@n@12", b"b@n@n412", b"b@n4n@12", b"b@n4n412", b"b4n@n@12", b"b4n@n412", b"b4n4n@12", b"b4n4n412"]


def test_toggle():
    """--toggle on abcd1234: 16 candidates in itertools.product order, the word itself first."""
    t = dwpa_amd.table_builtin("toggle")
    alt = dwpa_amd.table_parse(t)
    for c in range(256):
        ch = bytes([c])
        assert alt[c] == (ch + ch.swapcase() if ch.isalpha() and c < 128 else ch)
    want = [bytes(x) for x in itertools.product(b"aA", b"bB", b"cC", b"dD", b"1", b"2", b"3", b"4")]
    assert dwpa_amd.table_candidates(t, [b"abcd1234"], range(16)) == want and want[0] == b"abcd1234"
    assert want[1] == b"abcD1234" and want[15] == b"ABCD1234"
    assert dwpa_amd.table_candidates(t, [b"ABcd1234"], [0, 1, 4]) == [b"ABcd1234", b"ABcD1234", b"Abcd1234"]
    with pytest.raises(L.DwpaError):
        dwpa_amd.table_builtin("leet")


# ---------------------------------------------------------------------------------------------------------------
# keyspace and candidates against the reference
# ---------------------------------------------------------------------------------------------------------------
def _random_case(rng):
    keys = rng.sample(range(256), rng.randint(1, 12))
    mapping = {k: bytes(rng.sample(range(256), rng.choice((1, 1, 2, 2, 3, 5, 16)))) for k in keys}
    text = T.table_text(mapping, hexed=True)
    pool = keys + rng.sample(range(256), 6)
    words = [bytes(rng.choice(pool) for _ in range(rng.choice((0, 3, 7, 8, 8, 9, 10, 12, 20, 63, 64, 70))))
             for _ in range(rng.randint(0, 25))]
    return text, words, rng.choice((0, 1, 2, 8, 63)), rng.choice((8, 12, 63, 64, 200)), rng.choice((0, 1, 6, 100, 5000))


@pytest.mark.parametrize("seed", range(40))
def test_keyspace_and_candidates_match_the_reference(seed):
    rng = random.Random(0x7ab1e + seed)
    text, words, minlen, maxlen, word_max = _random_case(rng)
    plan = T.Plan(text, words, minlen, maxlen, word_max)
    ks = dwpa_amd.table_keyspace(text, words, minlen, maxlen, word_max)
    assert ks == {"keyspace": plan.k, "kept": plan.kept(), "dropped_len": plan.why.count(T.DROP_LEN),
                  "dropped_max": plan.why.count(T.DROP_MAX)}
    if plan.k == 0:
        with pytest.raises(L.DwpaError):
            dwpa_amd.table_candidates(text, words, [0], minlen, maxlen, word_max)
        return
    ids = sorted({0, plan.k - 1, *plan.start[:-1], *[s - 1 for s in plan.start[1:]],
                  *[rng.randrange(plan.k) for _ in range(200)]})
    assert dwpa_amd.table_candidates(text, words, ids, minlen, maxlen, word_max) == [plan.candidate(i) for i in ids]
    with pytest.raises(L.DwpaError) as e:
        dwpa_amd.table_candidates(text, words, [plan.k], minlen, maxlen, word_max)
    assert e.value.code == L.DWPA_E_ARG


def test_keyspace_above_u64_is_refused():
    """Kept words of 2^31 candidates each: 2^33 of them are 2^64, which no index can name; 2^33 - 1 of them fit.  (The
    list is too long to build; three are enough to show the sum is a sum, and the refusal is test_table_plan's fuzz.)"""
    t = T.TABLE
    w = T.PLAN_BIG.words
    assert dwpa_amd.table_keyspace(t, w)["keyspace"] == 3 * 2**31
    assert dwpa_amd.table_keyspace(t, w * 5)["keyspace"] == 15 * 2**31


# ---------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------
def _cli(capfdbinary, *argv):
    rc = CLI.main(list(argv))
    return rc, capfdbinary.readouterr().out


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("table_cli")
    plan = T.PLAN_DROPS_WIDE
    small = T.Plan(T.TABLE, T.PLAN_DROPS.words)  # word_max 0: the drops' list with its 15- and 64-count words kept
    (d / "t.table").write_bytes(T.TABLE)
    (d / "bad.table").write_bytes(b"a=b\nnot a mapping\n")
    (d / "list").write_bytes(b"".join(b"$HEX[" + w.hex().encode() + b"]\n" for w in small.words))
    (d / "list.gz").write_bytes(gzip.compress(b"abcd1234\r\nshort\r\nzz99zz99\r\n"))
    return {"dir": d, "plan": plan, "small": small, "table": str(d / "t.table"), "list": str(d / "list"),
            "gz": str(d / "list.gz"), "bad": str(d / "bad.table")}


def test_cli_keyspace_and_stdout(capfdbinary, files):
    small = files["small"]
    assert small.k == 56 + 15 + 64
    assert _cli(capfdbinary, "--keyspace", "--table-file", files["table"], files["list"]) == (0, b"%d\n" % small.k)
    capped = T.Plan(T.TABLE, small.words, word_max=14)
    assert _cli(capfdbinary, "--keyspace", "--table-max", "14", "--table-file", files["table"], files["list"]) == \
        (0, b"%d\n" % capped.k)
    rc, out = _cli(capfdbinary, "--stdout", "--table-file", files["table"], files["list"])
    assert rc == 0 and out == b"".join(small.candidate(i) + b"\n" for i in range(small.k))
    for s, l in ((0, 1), (14, 3), (small.k - 5, 0), (small.k - 1, 100), (7, 60)):
        rc, out = _cli(capfdbinary, "--stdout", "-s", str(s), "-l", str(l), "--table-file", files["table"], files["list"])
        hi = small.k if not l else min(small.k, s + l)
        assert rc == 0 and out == b"".join(small.candidate(i) + b"\n" for i in range(s, hi)), (s, l)
    rc, out = _cli(capfdbinary, "--stdout", "--toggle", files["gz"])  # gzip, CRLF; "short" owns no index
    want = [bytes(x) for x in itertools.product(b"aA", b"bB", b"cC", b"dD", b"1", b"2", b"3", b"4")] + \
           [bytes(x) for x in itertools.product(b"zZ", b"zZ", b"9", b"9", b"zZ", b"zZ", b"9", b"9")]
    assert rc == 0 and out == b"".join(w + b"\n" for w in want)
    assert _cli(capfdbinary, "--keyspace", "--toggle", files["gz"]) == (0, b"32\n")


def test_cli_refusals(capfdbinary, files):
    """Exit 255 and nothing on stdout."""
    t, lst = files["table"], files["list"]
    for argv in (["--keyspace", lst],                                              # no table
                 ["--keyspace", "--toggle", "--table-file", t, lst],               # two tables
                 ["--keyspace", "--table-file", files["bad"], lst],                # a bad table
                 ["--keyspace", "--table-file", str(files["dir"] / "missing"), lst],
                 ["--keyspace", "--table-file", t, str(files["dir"] / "missing")],
                 ["--keyspace", "--table-file", t],                                # no list
                 ["--keyspace", "--table-file", t, lst, lst],                      # a hash file with --keyspace
                 ["--stdout", "-s", str(files["small"].k), "--table-file", t, lst],   # skip >= K
                 ["--stdout", "-s", "-1", "--table-file", t, lst],
                 ["--stdout", "--table-max", str(2**32), "--table-file", t, lst],
                 ["--table-file", t, lst],                                         # no hash file
                 ["--no-such-option", lst]):
        assert _cli(capfdbinary, *argv) == (255, b""), argv
    assert CLI.main(["--keyspace", "--table-file", files["bad"], lst]) == 255
    assert b"line 2" in capfdbinary.readouterr().err


def test_cli_module(files):
    """python -m dwpa_amd.table --stdout as a module: needs no device and no hash file."""
    r = subprocess.run([sys.executable, "-m", "dwpa_amd.table", "--stdout", "--toggle", "-s", "15", "-l", "2",
                        files["gz"]], cwd=ROOT, capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout == b"ABCD1234\nzz99zz99\n", r.stderr[-2000:]
    r = subprocess.run([sys.executable, "-m", "dwpa_amd.table", "--keyspace", "--table-file", files["bad"],
                        files["gz"]], cwd=ROOT, capture_output=True, timeout=120)
    assert r.returncode == 255 and r.stdout == b"" and b"line 2" in r.stderr


# ---------------------------------------------------------------------------------------------------------------
# the fuzz target
# ---------------------------------------------------------------------------------------------------------------
def test_table_host_code_under_asan():
    """tools/table_fuzz.cpp: table.cpp alone (host code, a stand-alone program) under AddressSanitizer + UBSan: the
    parser on random bytes, counts against a 128-bit product, every candidate against a naive odometer; a difference,
    an out-of-bounds access or UB fails the binary."""
    subprocess.run(["make", "-s", "-C", ROOT, "tools/bin/table_fuzz_asan"], check=True)
    r = subprocess.run([os.path.join(ROOT, "tools", "bin", "table_fuzz_asan"), "1500"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "1500 cases ok" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
