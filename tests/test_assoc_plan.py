"""CPU: the library's association plan (dwpa_assoc_plan / _candidates / _single: nets, the association file, the single
generator, entries, start[], candidate(id)) against the plain-Python reference of tests/assoc_plan.py, on every fixture
and for every index."""
import pytest

import dwpa_amd
from dwpa_amd import _lib as L
from tests import assoc_plan as A


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    d = tmp_path_factory.mktemp("assoc_plan")
    lines, assoc = A.cpu_fixture()
    (d / "h.hash").write_bytes(b"\n".join(lines) + b"\n")
    A.write_assoc(d / "a.txt", assoc)
    A.write_assoc(d / "a.gz", assoc, gz=True, crlf=True)
    (d / "r.rule").write_text("".join(r + "\n" for r in A.FILE_RULES))
    return {"dir": d, "lines": lines, "assoc": assoc, "hash": str(d / "h.hash"), "afile": str(d / "a.txt"),
            "agz": str(d / "a.gz"), "rules": str(d / "r.rule")}


CASES = [("file", True, False, False), ("file+single", True, True, False), ("single", False, True, False),
         ("single+rules", False, True, True), ("file+rules", True, False, True), ("all", True, True, True)]


def _same(fx, plan, afile, single, rules):
    assert dwpa_amd.assoc_plan(fx["hash"], afile, single, rules) == plan.info()
    got = dwpa_amd.assoc_candidates(fx["hash"], range(plan.k), afile, single, rules)
    exp = [(plan.candidate(i), plan.first_line(i)) for i in range(plan.k)]
    assert got == exp


@pytest.mark.parametrize("name,use_file,single,use_rules", CASES)
def test_plan_and_every_candidate(fx, name, use_file, single, use_rules):
    plan = A.Plan(fx["lines"], fx["assoc"] if use_file else None, single, A.FILE_RULES if use_rules else None)
    assert plan.k > 0 and len(plan.nets) == 7
    _same(fx, plan, fx["afile"] if use_file else None, single, fx["rules"] if use_rules else None)
    if use_rules:  # some index gives no candidate, some rule changes the length
        cands = [plan.candidate(i) for i in range(plan.k)]
        assert None in cands and len({len(c) for c in cands if c}) > 3


def test_gzip_and_crlf(fx):
    plan = A.Plan(fx["lines"], fx["assoc"], True, None)
    _same(fx, plan, fx["agz"], True, None)


def test_the_fixture_holds_what_the_issue_names(fx):
    plan = A.Plan(fx["lines"], fx["assoc"], True, None)
    assert plan.net_of_line[4] is None and plan.nets[3][2] == [3, 5]  # the unusable line shifts input lines, not nets
    assert plan.unmatched == 1 and plan.malformed == 4 and plan.file_lines == len(fx["assoc"])
    assert plan.dropped >= 3  # the duplicate, the empty word, the 257-byte word (and the generator's repeats)
    assert b"M" * 256 in plan.words[2] and b"L" * 257 not in plan.words[2]
    assert b"colon:\xff-000001" in plan.words[3] and b"$HEX[zz]" in plan.words[3]
    assert b"UPPER-MAC-000001" in plan.words[1] and b"with:colons:inside-1" in plan.words[6]
    assert plan.words[4][:3] == plan.words[5][:3] == A.counter_words(b"assoc4", 3)  # one MAC, two ESSIDs
    # the wrap: 000000000000 - 1 and ffffffffffff + 1
    assert b"ffffffffffff" in plan.words[0] and b"FFFFFFFF" in plan.words[0] and b"000000000001" in plan.words[0]
    assert b"000000000000" in plan.words[1] and b"fffffffffffe" in plan.words[1]
    # an all-digit BSSID: upper and lower case are one entry, 9 words instead of 18
    assert sum(1 for w in plan.words[2] if w.isdigit()) == 9
    # ESSIDs of 4 and 7 bytes: without rules only ESSID123 (7) / ESSID1, ESSID123, ESSID! (7 + 1..3) reach 8 bytes
    assert [w for w in plan.words[0] if w.lower().startswith(b"four")] == []
    assert {w for w in plan.words[1] if w.lower().startswith(b"seven77")} == {
        b"Seven771", b"SEVEN771", b"seven771", b"Seven77123", b"SEVEN77123", b"seven77123", b"Seven77!", b"SEVEN77!",
        b"seven77!"}
    ruled = A.Plan(fx["lines"], None, True, A.FILE_RULES)
    assert b"four" in ruled.words[0] and b"linksys" in ruled.words[6]  # minlen 1 with rules: linksys + $1 is reachable
    assert b"linksys1" in {ruled.candidate(i) for i in range(ruled.start[6], ruled.start[7])}
    assert len(plan.nets[3][0]) == 32 and plan.nets[3][0] + b"123" in plan.words[3]


def test_single_per_line(fx):
    for ln in fx["lines"]:
        key = A.line_net(ln)
        for minlen in (1, 8, 33):
            if key is None:
                with pytest.raises(L.DwpaError):
                    dwpa_amd.assoc_single(ln, minlen)
            else:
                assert dwpa_amd.assoc_single(ln, minlen) == A.single(key[1], key[0], minlen)
    assert len(dwpa_amd.assoc_single(fx["lines"][0], 1)) == 18 + 4 * 2  # "four" is its own lower case


def test_refusals(fx, tmp_path):
    def refused(code, *a):
        with pytest.raises(L.DwpaError) as e:
            dwpa_amd.assoc_plan(*a)
        assert e.value.code == code, a

    refused(L.DWPA_E_ARG, fx["hash"], None, False, None)  # no source
    refused(L.DWPA_E_IO, fx["hash"], str(tmp_path / "missing"), False, None)
    refused(L.DWPA_E_IO, str(tmp_path / "missing"), None, True, None)
    refused(L.DWPA_E_IO, fx["hash"], None, True, str(tmp_path / "missing"))
    (tmp_path / "bad.rule").write_text("not a rule at all\n")
    refused(L.DWPA_E_RULE, fx["hash"], None, True, str(tmp_path / "bad.rule"))
    plan = A.Plan(fx["lines"], None, True, None)
    with pytest.raises(L.DwpaError) as e:
        dwpa_amd.assoc_candidates(fx["hash"], [plan.k], None, True, None)
    assert e.value.code == L.DWPA_E_ARG


def test_two_to_the_32_choices_in_one_net_are_refused(fx, tmp_path):
    """65,536 words of one net under 65,536 rules are 2^32 choices: refused; under 65,535 rules they run."""
    m = A.line_net(fx["lines"][0])[1].hex().encode()
    A.write_assoc(tmp_path / "big.txt", [m + b":w%05d" % i for i in range(65536)])
    (tmp_path / "r65536.rule").write_text(":\n" * 65536)
    (tmp_path / "r65535.rule").write_text(":\n" * 65535)
    with pytest.raises(L.DwpaError) as e:
        dwpa_amd.assoc_plan(fx["hash"], str(tmp_path / "big.txt"), False, str(tmp_path / "r65536.rule"))
    assert e.value.code == L.DWPA_E_ARG
    info = dwpa_amd.assoc_plan(fx["hash"], str(tmp_path / "big.txt"), False, str(tmp_path / "r65535.rule"))
    assert info["keyspace"] == 65536 * 65535 and info["entries"] == 65536 and info["rules"] == 65535
    got = dwpa_amd.assoc_candidates(fx["hash"], [0, 65535, 65536, info["keyspace"] - 1], str(tmp_path / "big.txt"),
                                    False, str(tmp_path / "r65535.rule"))
    assert got == [(None, 0)] * 4  # six bytes each: below 8
