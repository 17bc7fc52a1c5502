"""GPU recall of the client hot loop: every candidate slot of a scan must be found.

The scan path (dictionary / rules / numeric prep -> PBKDF2 -> key-parallel verify -> hit buffer) fails silently in one
direction: a candidate that is dropped, derived wrongly or verified against the wrong PMK is simply not reported.  The
other scan tests plant a handful of keys among thousands, so every other lane of their launches could hold a wrong PMK.
Here EVERY loaded candidate is the PSK of one line per ESSID, and the hits of a scan must be exactly the set the CPU
oracle expects -- none missing, none extra, none twice, each with the oracle's PMK.

Which PBKDF2 kernel a launch gets depends only on its size relative to the device (pbkdf2_module.cpp), and for a scan
the size is the scan's `batch`, not the number of words loaded.  The batch sizes below are computed from the device's
CU count by the same rules, and every test asserts the exact set of PBKDF2 kernels that ran (the library's
dwpa_debug_pbkdf2_kernels hook), so a change of the selection rules fails these tests instead of quietly moving them
to another kernel.
"""
import ctypes
import gzip
import os
import pickle
import random
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

import dwpa_amd  # noqa: E402
from dwpa_amd import _lib as L  # noqa: E402
from dwpa_amd.device import Dictionary  # noqa: E402
from oracle import oracle as O  # noqa: E402
from oracle import rules as R  # noqa: E402
from tests import synth as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE_ENV = "DWPA_RECALL_FIXTURE"  # set for the forced-build children: the parent's pickled fixture
NC = 8
OFFSETS = (0, 1, -1, 2, -2, -3, 4, -4)  # planted nonce offsets, each in both endians
ESSIDS = (b"R", b"recall-mid-13", bytes(0x41 + i % 26 for i in range(52)))  # 52: the salt's 2nd SHA-1 block
JUNK_LENGTHS = (0, 7, 64, 65, 300)  # outside the 8..63 filter
MIN_KEPT = 321  # 5 waves + 1 lane
RULES = [":", "l", "u", "$1", "c $1 $2 $3", "^e ^h ^t", "d", "[ [ [", "!a $a", ">9 $1", "$1 $2 $3 $4 $5 $6 $7 $8"]
N_RULE_WORDS = 60


# ---------------------------------------------------------------------------------------------------------------
# kernel selection, restated from pbkdf2_module.cpp
# ---------------------------------------------------------------------------------------------------------------
def _env_flag(name):
    e = os.environ.get(name, "")
    return bool(e) and e[0] != "0"


def _cu_count():
    """hipDeviceAttributeMultiprocessorCount of device 0, from the HIP runtime the library has loaded."""
    L.load()
    with open("/proc/self/maps") as f:
        path = next((ln.split()[-1] for ln in f if "libamdhip64.so" in ln), None)
    assert path, "the library maps no libamdhip64"
    hip = ctypes.CDLL(path)
    v = ctypes.c_int(0)
    assert hip.hipDeviceGetAttribute(ctypes.byref(v), 63, 0) == 0  # 63: hipDeviceAttributeMultiprocessorCount
    assert 1 <= v.value <= 4096, v.value
    return v.value


@pytest.fixture(scope="module")
def sizes():
    """Smallest / largest batch (a multiple of 64) that selects each PBKDF2 variant on this device.  level_lanes =
    CUs x 4 SIMDs x 64; a launch of `pmks` slots runs the plain kernel while 2 * pmks <= level_lanes, the priority
    kernel while 2 * pmks <= 8 * level_lanes, the queue kernel above that.  One-ESSID launches: pmks = batch;
    multi-group launches of the three ESSIDs: pmks = 3 x batch."""
    assert dwpa_amd.device_count() >= 1
    ll = _cu_count() * 4 * 64
    def up(x):  # smallest multiple of 64 above x
        return (x // 64 + 1) * 64
    s = {"level_lanes": ll,
         "one": {"plain": ll // 2 // 64 * 64,       # the largest plain launch: 2 * batch <= level_lanes
                 "p": up(ll // 2),                  # the smallest priority launch
                 "q": up(4 * ll)},                  # the smallest queue launch: 2 * batch > 8 * level_lanes
         "mg": {"plain": ll // 6 // 64 * 64, "p": up(ll // 6), "q": up(8 * ll // 6)}}
    for kind, n in (("one", 1), ("mg", 3)):
        b = s[kind]
        assert 2 * n * b["plain"] <= ll < 2 * n * b["p"] and 2 * n * (b["p"] - 64) <= ll
        assert 2 * n * (b["q"] - 64) <= 8 * ll < 2 * n * b["q"]
        assert MIN_KEPT + 64 <= b["plain"] < b["p"] < b["q"]
    return s


def expected_kernel(kind, variant):
    """The one kernel a scan launch of this kind ('one' / 'mg') and size class must run, given the process's
    DWPA_PBKDF2_PLAIN / DWPA_PBKDF2_ISSUE switches."""
    if _env_flag("DWPA_PBKDF2_PLAIN"):
        return {"one": "k_pbkdf2", "mg": "k_pbkdf2_mg"}[kind]
    if variant == "plain" and _env_flag("DWPA_PBKDF2_ISSUE"):
        variant = "p"
    stem = {"one": "k_pbkdf2_gfx950", "mg": "k_pbkdf2_gfx950_mg"}[kind]
    return {"plain": {"one": "k_pbkdf2", "mg": "k_pbkdf2_mg"}[kind], "p": stem + "_p", "q": stem + "_q"}[variant]


# ---------------------------------------------------------------------------------------------------------------
# the all-plants fixture (CPU)
# ---------------------------------------------------------------------------------------------------------------
def _word(rng, n, binary, seen):
    while True:
        if binary:  # any byte but NUL (a trailing NUL is HMAC key padding), LF and CR (a dictionary file's line ends)
            w = bytes(rng.choice(_BIN) for _ in range(n))
        else:
            w = bytes(rng.randint(0x21, 0x7E) for _ in range(n))
        if w not in seen and not w.startswith(b"$HEX["):
            seen.add(w)
            return w


_BIN = [b for b in range(1, 256) if b not in (10, 13)]


def _build_words(rng):
    """The dictionary: every kept length 8..63 at every byte offset mod 4 of the packed bytes (load_key_block's
    aligned-dword path shifts by it), filtered-out words interleaved so that compaction moves slots, >= MIN_KEPT kept
    words, all distinct, the last word kept and ending at an unaligned byte."""
    need = {(n, r) for n in range(8, 64) for r in range(4)}
    words, seen = [], set()
    off = kept = 0
    while need or kept < MIN_KEPT or off % 4 == 0:
        r = off % 4
        want = sorted(n for n in range(8, 64) if (n, r) in need)
        if want:
            n = rng.choice(want)
        elif need:  # nothing left to cover at this offset: a 65-byte filtered word moves it on by one
            n = 65
        else:
            n = rng.choice([m for m in range(8, 64) if (off + m) % 4])
        if 8 <= n <= 63:
            need.discard((n, r))
            words.append(_word(rng, n, kept % 7 == 3, seen))
            kept += 1
            if kept % 4 == 0 and (need or kept < MIN_KEPT):
                m = JUNK_LENGTHS[kept // 4 % len(JUNK_LENGTHS)]
                words.append(_word(rng, m, False, seen) if m else b"")
                off += m
        else:
            words.append(_word(rng, n, False, seen))
        off += n
    return words


def _line(kind, nc, endian, psk, essid, pmk, rng):
    ap, sta = rng.randbytes(6), rng.randbytes(6)
    if kind == 0:
        return S.pmkid_line(psk, essid, ap, sta, the_pmk=pmk)
    return S.eapol_line(psk, essid, ap, sta, rng.randbytes(32), rng.randbytes(32), kind, nc, endian,
                        mp=(0x00, 0x80, 0x02)[nc % 3], the_pmk=pmk, rng=rng)


def _plant_lines(psks, essids, rng, stride=16):
    """One line per (essid, psk): kinds cycle through PMKID and keyver 1/2/3, EAPOL lines carry every OFFSETS x endian.
    Returns (lines, [(essid index, psk index)], [pmk], [(nc, endian) the oracle reports])."""
    lines, owner, pmks, found = [], [], [], []
    for e, essid in enumerate(essids):
        raw = O.c_pbkdf2_many(psks, essid, threads=8)
        for i, psk in enumerate(psks):
            k = len(lines)
            pmk = raw[32 * i:32 * i + 32]
            line = _line(k % 4, OFFSETS[k // 4 % 8], ("LE", "BE")[k // 32 % 2], psk, essid, pmk, rng)
            exp = O.c_check_key_m22000(line, [psk], pmk, NC)  # the PMK handed over: no second derive
            assert exp and exp[0] == psk and exp[3] == pmk, (k, exp)
            if k % stride == 0:  # and the whole check, derive included, for a fixed stride of the lines
                assert O.c_check_key_m22000(line, [psk], False, NC) == exp, k
            lines.append(line)
            owner.append((e, i))
            pmks.append(pmk)
            found.append((exp[1], exp[2]))
    assert len(set(lines)) == len(lines)
    return lines, owner, pmks, found


def _build_fixture():
    rng = random.Random(0x5ca9)
    words = _build_words(rng)
    kept = [i for i, w in enumerate(words) if 8 <= len(w) <= 63]
    # the conditions the tests rely on
    assert len(kept) >= MIN_KEPT and len({words[i] for i in kept}) == len(kept)  # no PSK twice within an ESSID
    offs = [0]
    for w in words:
        offs.append(offs[-1] + len(w))
    assert {(len(words[i]), offs[i] % 4) for i in kept} == {(n, r) for n in range(8, 64) for r in range(4)}
    assert {len(w) for w in words if not 8 <= len(w) <= 63} == set(JUNK_LENGTHS)
    assert kept[-1] == len(words) - 1 and offs[-1] % 4 != 0
    assert kept != list(range(len(kept)))  # compaction moves slots: ids[] must carry the original index
    psks = [words[i] for i in kept]
    lines, owner, pmks, found = _plant_lines(psks, ESSIDS, rng)
    for kv in (1, 2, 3):  # every keyver reports every planted offset in both endians
        seen = {found[k] for k in range(kv, len(lines), 4)}
        assert all((o, en) in seen for o in OFFSETS if o for en in ("LE", "BE")) and 0 in {nc for nc, _ in seen}, kv
    assert all(found[k] == (None, None) for k in range(0, len(lines), 4))  # PMKID lines
    plants = [(k, kept[i], nc, en, pmk) for k, ((e, i), (nc, en), pmk) in enumerate(zip(owner, found, pmks))]

    # rules: every surviving candidate (word x rule inside 8..63) is a plant
    base = []
    for j in range(N_RULE_WORDS):
        n = (5, 6, 7, 8, 9, 11, 14, 30, 33, 56, 60, 63)[j % 12]
        w = bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(n))
        if j % 3 == 0:
            w = w[:1].upper() + w[1:3] + w[3:5].upper() + w[5:]  # mixed case: ':' and 'l' differ
        base.append(w)
    assert len(set(base)) == len(base)
    ops = [R.parse(r) for r in RULES]
    assert all(o is not None for o in ops)
    by_psk = {}
    outcomes = set()
    for wi, w in enumerate(base):
        for ri, o in enumerate(ops):
            c = R.apply(o, w)
            outcomes.add("reject" if c is None else "short" if len(c) < 8 else "long" if len(c) > 63 else "kept")
            if c is not None and 8 <= len(c) <= 63:
                by_psk.setdefault(c, []).append(wi * len(RULES) + ri)
    assert outcomes == {"reject", "short", "long", "kept"}
    assert any(len(ids) > 1 for ids in by_psk.values())  # two rules, one candidate
    rpsks = sorted(by_psk)
    rlines, rowner, rpmks, rfound = _plant_lines(rpsks, ESSIDS, rng)
    rplants = [(k, cid, nc, en, pmk) for k, ((e, i), (nc, en), pmk) in enumerate(zip(rowner, rfound, rpmks))
               for cid in by_psk[rpsks[i]]]
    return {"words": words, "kept": kept, "lines": lines, "plants": plants,
            "rule_words": base, "rule_lines": rlines, "rule_plants": rplants,
            "rule_psk": [rpsks[i] for e, i in rowner], "psk": [psks[i] for e, i in owner]}


@pytest.fixture(scope="module")
def fx():
    path = os.environ.get(FIXTURE_ENV)
    if path:  # a forced-build child: the parent's fixture
        with open(path, "rb") as f:
            return pickle.load(f)
    return _build_fixture()


@pytest.fixture(scope="module")
def dev(fx):
    assert dwpa_amd.device_count() >= 1
    return {"dict": Dictionary.from_words(fx["words"]), "rule_dict": Dictionary.from_words(fx["rule_words"])}


def _hitset(hits):
    got = [(h["line"], h["cand"], h["nc"], h["endian"], h["pmk"]) for h in hits]
    assert len(set(got)) == len(got), "a hit was reported twice"
    return set(got)


def _expect(plants, lo, hi):
    return {p for p in plants if lo <= p[1] < hi}


def _assert_same(got, exp, what):
    missing, extra = exp - got, got - exp
    assert not missing and not extra, (what, "missing %d" % len(missing), sorted(missing)[:3],
                                       "extra %d" % len(extra), sorted(extra)[:3])


def _prefix_with_kept(kept, k):
    """The shortest dictionary prefix that holds k kept words."""
    return kept[k - 1] + 1


def _loads(fx):
    """(first, count, kept) of the dictionary loads, in an order in which no slot of a load was derived with the same
    word by an earlier load of the scan: a stale PMK can then never stand in for one the kernel skipped."""
    kept = fx["kept"]
    out = [(0, _prefix_with_kept(kept, k), k) for k in (1, 63, 64, 65, 256, 257, len(kept))]
    first = kept[37]  # a window that starts inside the dictionary, at a kept word: 130 kept words, two waves + 2 lanes
    out.append((first, kept[37 + 129] + 1 - first, 130))
    return out


def _scan_all(sc, mode):
    if mode == "run":
        sc.run()
    else:
        for g in range(sc.groups):
            sc.pbkdf2(g)
            sc.verify(g)


def _dict_recall(fx, dev, batch, mode, kernel):
    d = dev["dict"]
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(fx["lines"], nc=NC, batch=batch)
    try:
        assert sc.groups == len(ESSIDS)
        for first, count, nkept in _loads(fx):
            sc.load_dict(d.off.ptr, d.data.ptr, first, count)
            assert sc.loaded() == nkept
            _scan_all(sc, mode)
            _assert_same(_hitset(sc.hits(cap=4096)), _expect(fx["plants"], first, first + count),
                         (mode, batch, first, count))
    finally:
        sc.close()
    assert L.pbkdf2_kernels() == {kernel}


# ---------------------------------------------------------------------------------------------------------------
# a-d: the scan API
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "p", "q"])
def test_per_group_path_finds_every_slot(fx, dev, sizes, variant):
    """a. pbkdf2(g) / verify(g) per ESSID group at the batch sizes that select k_pbkdf2, k_pbkdf2_gfx950_p and
    k_pbkdf2_gfx950_q: dictionary prefixes with 1, 63, 64, 65, 256, 257 and all kept words, and one window with
    first > 0; the hits are exactly the planted (line, cand, nc, endian, pmk)."""
    _dict_recall(fx, dev, sizes["one"][variant], "per_group", expected_kernel("one", variant))


@pytest.mark.parametrize("variant", ["plain", "p", "q"])
def test_run_path_finds_every_slot(fx, dev, sizes, variant):
    """b. The same through run(): one multi-group launch of the three ESSIDs, at batch sizes that select k_pbkdf2_mg,
    k_pbkdf2_gfx950_mg_p and k_pbkdf2_gfx950_mg_q.  In the queue case most items lie past the loaded count, so each
    wave takes several and must skip the empty ones."""
    _dict_recall(fx, dev, sizes["mg"][variant], "run", expected_kernel("mg", variant))


@pytest.mark.parametrize("kind,variant,mode", [("one", "p", "per_group"), ("mg", "q", "run")])
def test_rules_path_finds_every_candidate(fx, dev, sizes, kind, variant, mode):
    """c. set_rules + load_rules: words x rules with rules that reject, shorten below 8 and lengthen past 63, and
    two rules that give one candidate.  A line expects every id word * nrules + rule whose oracle result is its
    PSK."""
    d = dev["rule_dict"]
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(fx["rule_lines"], nc=NC, batch=sizes[kind][variant])
    try:
        assert sc.set_rules("\n".join(RULES)) == len(RULES)
        nr, nw = len(RULES), len(fx["rule_words"])
        for first, count in ((0, nw), (7, 23)):
            sc.load_rules(d.off.ptr, d.data.ptr, first, count)
            exp = _expect(fx["rule_plants"], first * nr, (first + count) * nr)
            assert sc.loaded() == len({p[1] for p in exp})
            _scan_all(sc, mode)
            _assert_same(_hitset(sc.hits(cap=8192)), exp, (mode, first, count))
    finally:
        sc.close()
    assert L.pbkdf2_kernels() == {expected_kernel(kind, variant)}


NUMERIC = [(8, 99_999_900, 100),          # the top of the 8-digit keyspace
           (10, 2**32 - 50, 100),         # across 2^32
           (20, 2**64 - 100, 100),        # up to 2^64 - 1, all 20 digits
           (9, 100_000_037, 130)]         # first not a multiple of 64, two waves + 2 lanes


@pytest.mark.parametrize("digits,first,count", NUMERIC)
def test_numeric_keyspace_finds_every_value(sizes, digits, first, count):
    """d. load_numeric with every value of the range a plant (k_prep_numeric takes up to 20 digits and 64-bit
    values; the suite had it at 8 digits only)."""
    rng = random.Random(digits)
    essid = b"recall-numeric"
    psks = [b"%0*d" % (digits, v) for v in range(first, first + count)]
    assert all(len(p) == digits for p in psks)
    lines, owner, pmks, found = _plant_lines(psks, [essid], rng)
    exp = {(k, first + i, nc, en, pmk) for k, ((e, i), (nc, en), pmk) in enumerate(zip(owner, found, pmks))}
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(lines, nc=NC, batch=sizes["one"]["p"])
    try:
        sc.load_numeric(first, count, digits)
        assert sc.loaded() == count
        _scan_all(sc, "per_group")
        _assert_same(_hitset(sc.hits(cap=4096)), exp, (digits, first))
    finally:
        sc.close()
    assert L.pbkdf2_kernels() == {expected_kernel("one", "p")}


# ---------------------------------------------------------------------------------------------------------------
# e: the hit buffer's boundary
# ---------------------------------------------------------------------------------------------------------------
def _same_psk_lines(psk, essid, n, rng):
    pmk = O.c_pbkdf2(psk, essid)
    lines = [S.pmkid_line(psk, essid, rng.randbytes(6), rng.randbytes(6), the_pmk=pmk) for _ in range(n)]
    assert len(set(lines)) == n and O.c_check_key_m22000(lines[-1], [psk], False, NC) == [psk, None, None, pmk]
    return lines, pmk


def test_hit_buffer_filled_exactly():
    """e1. hitcap = max(batch, 65536): 256 PMKID lines that share one PSK x a dictionary of 256 copies of it give
    65536 hits, the last one in the buffer's last record.  Every (line, cand) pair comes back once."""
    rng = random.Random(0xe1)
    psk, essid = b"hit-buffer-psk", b"recall-hitbuf"
    lines, pmk = _same_psk_lines(psk, essid, 256, rng)
    d = Dictionary.from_words([psk] * 256)
    L.pbkdf2_kernels(reset=True)
    sc = dwpa_amd.Scan(lines, nc=NC, batch=256)
    try:
        sc.load_dict(d.off.ptr, d.data.ptr, 0, 256)
        _scan_all(sc, "per_group")
        hits = sc.hits(cap=1 << 16)
    finally:
        sc.close()
    assert len(hits) == 1 << 16
    assert {(h["line"], h["cand"]) for h in hits} == {(ln, c) for ln in range(256) for c in range(256)}
    assert all(h["pmk"] == pmk and h["nc"] is None for h in hits)
    assert L.pbkdf2_kernels() == {expected_kernel("one", "plain")}


def test_scan_usable_after_hit_overflow(fx, dev):
    """e2. 258 x 256 hits are more than hitcap: hits() raises DWPA_E_OVERFLOW (the records past hitcap were never
    written).  The same scan then scans the all-plants dictionary and returns exactly its hits: the overflow must
    not leave the hit counter above hitcap (it did: scan_hits_raw returned before it reset the counter, and every
    later hits() of the scan failed with the same code)."""
    rng = random.Random(0xe2)
    kept = fx["kept"]
    at = kept[200]
    psk, essid = fx["words"][at], b"recall-hitbuf"
    lines, pmk = _same_psk_lines(psk, essid, 258, rng)
    d = Dictionary.from_words([psk] * 256)
    L.pbkdf2_kernels(reset=True)
    assert len(fx["words"]) <= 1024
    sc = dwpa_amd.Scan(lines, nc=NC, batch=1024)
    try:
        sc.load_dict(d.off.ptr, d.data.ptr, 0, 256)
        _scan_all(sc, "per_group")
        with pytest.raises(L.DwpaError) as e:
            sc.hits(cap=1 << 17)
        assert e.value.code == L.DWPA_E_OVERFLOW
        ad = dev["dict"]
        sc.load_dict(ad.off.ptr, ad.data.ptr, 0, len(fx["words"]))
        assert sc.loaded() == len(kept)
        _scan_all(sc, "per_group")
        _assert_same(_hitset(sc.hits(cap=4096)), {(ln, at, None, None, pmk) for ln in range(258)}, "after overflow")
    finally:
        sc.close()
    assert L.pbkdf2_kernels() == {expected_kernel("one", "plain")}


# ---------------------------------------------------------------------------------------------------------------
# f: the product path
# ---------------------------------------------------------------------------------------------------------------
def _plain(b):
    return b if all(0x20 <= c <= 0x7E and c != 0x3A for c in b) and not b.startswith(b"$HEX[") \
        else b"$HEX[" + b.hex().encode() + b"]"


def _records(lines, psks):
    """The outfile record of each line: MIC or PMKID : AP : STA : ESSID : PSK (crack_common.cpp outfile_record)."""
    out = []
    for line, psk in zip(lines, psks):
        f = line.split(b"*")
        out.append(b":".join([f[2], f[3], f[4], _plain(bytes.fromhex(f[5].decode())), _plain(psk)]))
    return out


MG_KERNELS = {"k_pbkdf2_mg", "k_pbkdf2_gfx950_mg", "k_pbkdf2_gfx950_mg_p", "k_pbkdf2_gfx950_mg_q"}


def _crack(tmp_path, lines, psks, dict_path, rules_path, **kw):
    hf, out = tmp_path / "h.hash", tmp_path / "o.key"
    hf.write_bytes(b"\n".join(lines) + b"\n")
    L.pbkdf2_kernels(reset=True)
    rc = dwpa_amd.crack_files(str(hf), [str(dict_path)], rules_path and str(rules_path), NC, str(out), batch=512,
                              nc_mode=L.DWPA_NC_HASHCAT, **kw)
    ran = L.pbkdf2_kernels()
    assert rc == 0
    recs = out.read_bytes().split(b"\n")
    assert recs.pop() == b""
    assert sorted(recs) == sorted(_records(lines, psks))  # every line exactly once, with its PSK
    assert ran and ran <= MG_KERNELS, ran


def test_crack_files_cracks_every_line(fx, tmp_path):
    """f1. dwpa_crack_files (hashcat NC mode, batch 512) over the all-plants hash file and the dictionary as a .gz
    with CRLF endings in its first half and one $HEX[] entry: rc 0, and the outfile holds every line once."""
    words = list(fx["words"])
    hexed = fx["kept"][10]
    words[hexed] = b"$HEX[" + words[hexed].hex().encode() + b"]"
    half = len(words) // 2
    d = tmp_path / "d.txt.gz"
    with gzip.open(d, "wb") as f:
        f.write(b"".join(w + b"\r\n" for w in words[:half]) + b"".join(w + b"\n" for w in words[half:]))
    _crack(tmp_path, fx["lines"], fx["psk"], d, None)


def test_crack_files_rules_cracks_every_line(fx, tmp_path):
    """f2. The same for the rules fixture with a rule file (every rule line loaded: the reject rules run too)."""
    d, rf = tmp_path / "d.txt", tmp_path / "r.rule"
    d.write_bytes(b"".join(w + b"\n" for w in fx["rule_words"]))
    rf.write_text("\n".join(RULES) + "\n")
    _crack(tmp_path, fx["rule_lines"], fx["rule_psk"], d, rf, rule_mode=L.DWPA_RULES_FULL)


# ---------------------------------------------------------------------------------------------------------------
# g: the check path's non-priority kernel
# ---------------------------------------------------------------------------------------------------------------
def test_check_path_non_priority_kernel(sizes):
    """g. dwpa_pbkdf2_pmk over enough distinct keys that the head is 9 wave units (one unit = level_lanes / 2 PMKs):
    more than one priority round, so the head runs k_pbkdf2_gfx950_ms, which no other test compares PMKs of.  The
    oracle checks >= 512 positions (0, both sides of every wave-unit boundary, the last head PMK, the first tail PMK,
    the last key); every other PMK must equal a re-derivation in calls of <= 16384 keys, which run the plain-schedule
    kernel."""
    unit = sizes["level_lanes"] // 2
    head = 9 * unit
    assert 2 * head > 8 * sizes["level_lanes"] >= 2 * (head - unit)
    n = head + 37
    pad = bytes(0x21 + i % 94 for i in range(64))
    keys = [b"%08d" % i + pad[i % 7:i % 7 + i % 56] for i in range(n)]  # distinct, 8..63 bytes
    essid = b"recall-check-path"
    L.pbkdf2_kernels(reset=True)
    got = dwpa_amd.pbkdf2_pmk(keys, essid)
    ran = L.pbkdf2_kernels()
    big = "k_pbkdf2_ms" if _env_flag("DWPA_PBKDF2_PLAIN") else "k_pbkdf2_gfx950_ms"
    assert big in ran, ran
    assert ran <= {big, "k_pbkdf2_ms_tail"}, ran  # the 37-key tail: the host backend or the tail kernel
    pos = {0, head - 1, head, n - 1}
    for k in range(1, 10):
        pos |= {k * unit - 1, k * unit}
    rng = random.Random(9)
    while len(pos) < 512:
        pos.add(rng.randrange(n))
    pos = sorted(pos)
    ref = O.c_pbkdf2_many([keys[i] for i in pos], essid, threads=8)
    for j, i in enumerate(pos):
        assert got[i] == ref[32 * j:32 * j + 32], i
    L.pbkdf2_kernels(reset=True)
    step = 16384
    assert 2 * step <= sizes["level_lanes"]
    for b in range(0, n, step):
        assert dwpa_amd.pbkdf2_pmk(keys[b:b + step], essid) == got[b:b + step], b
    small = {"k_pbkdf2_ms"} if not _env_flag("DWPA_PBKDF2_ISSUE") or _env_flag("DWPA_PBKDF2_PLAIN") \
        else {"k_pbkdf2_gfx950_ms_p"}
    assert L.pbkdf2_kernels() == small


# ---------------------------------------------------------------------------------------------------------------
# h: a-d again with the kernel choice forced
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch", ["DWPA_PBKDF2_PLAIN", "DWPA_PBKDF2_ISSUE"])
def test_forced_builds(fx, tmp_path, switch):
    """h. Tests a-d in a fresh child process (the switches are read once per process) with the plain-schedule
    kernels forced, and with the issue-pass kernels forced; the masks they expect follow from the switch.  The
    child reads this process's fixture from a file."""
    fxp = tmp_path / "fixture.pkl"
    with open(fxp, "wb") as f:
        pickle.dump(fx, f)
    env = {k: v for k, v in os.environ.items() if k not in ("DWPA_PBKDF2_PLAIN", "DWPA_PBKDF2_ISSUE")}
    env.update({switch: "1", FIXTURE_ENV: str(fxp)})
    sel = "per_group_path or run_path or rules_path or numeric_keyspace"
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        os.path.abspath(__file__), "-k", sel], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "12 passed" in r.stdout, r.stdout[-500:]
