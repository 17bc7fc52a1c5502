"""CPU: the C-ABI library loads, exports every symbol include/dwpa22000.h declares, and its host-only helpers match
the oracle.  What compute calls do without a GPU (DWPA_E_NODEV, or the host backend when asked for) is
tests/test_host_backend.py::test_routing_without_a_device."""
import ctypes
import os
import re

import pytest

from dwpa_amd import _lib as L
from oracle import oracle as O
from tests import synth as S


def declared_symbols():
    txt = open(L.HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(dwpa_[a-z0-9_]+)\s*\(", txt)))


def test_header_declares_boundary():
    syms = declared_symbols()
    for s in ["dwpa_check_m22000", "dwpa_check_batch", "dwpa_pbkdf2_pmk", "dwpa_crack_files", "dwpa_scan_create",
              "dwpa_init", "dwpa_strerror", "dwpa_shutdown"]:
        assert s in syms


def test_library_exports_every_declared_symbol():
    lib = L.load()
    missing = [s for s in declared_symbols() if not hasattr(lib, s)]
    assert not missing, missing
    for s in L.SIGNATURES:
        assert hasattr(lib, s), s


def test_abi_version_and_strerror():
    lib = L.load()
    assert lib.dwpa_abi_version() == 4  # 4: host backend (allow_cpu_fallback, host_max_pmks, check_stats.backend)
    for code in [0, 1, -1, -2, -3, -4, -10, -12, -13, -14, -15, -16, -999]:
        assert lib.dwpa_strerror(code)


def test_debug_pbkdf2_kernels_hook():
    """dwpa_debug_pbkdf2_kernels (the test hook tests/test_gpu_recall.py reads which PBKDF2 kernel ran from): exported,
    outside the public header and the ABI version, and an empty mask in a process that has launched nothing."""
    import subprocess
    import sys
    assert hasattr(L.load(), "dwpa_debug_pbkdf2_kernels")
    assert "dwpa_debug_pbkdf2_kernels" not in declared_symbols()
    assert len(L.PBKDF2_KERNEL_NAMES) == len(set(L.PBKDF2_KERNEL_NAMES)) == 12
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    child = ("import sys; sys.path.insert(0, sys.argv[1]); from dwpa_amd import _lib as L; lib = L.load(); "
             "print(lib.dwpa_debug_pbkdf2_kernels(0), lib.dwpa_debug_pbkdf2_kernels(1), sorted(L.pbkdf2_kernels()))")
    r = subprocess.run([sys.executable, "-c", child, root], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip() == "0 0 []"


def test_debug_verify_kernels_hook():
    """dwpa_debug_verify_kernels and dwpa_debug_check_hit_records (the test hooks tests/test_gpu_check_recall.py reads
    from which verifier a check call ran and how many hit records it wrote): exported, outside the public header,
    the PHP cdef and the ABI version, and empty in a process that has launched nothing."""
    import subprocess
    import sys
    lib = L.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    php = open(os.path.join(root, "php", "dwpa22000.php")).read()
    for hook in ("dwpa_debug_verify_kernels", "dwpa_debug_check_hit_records"):
        assert hasattr(lib, hook)
        assert hook not in declared_symbols() and hook not in open(L.HEADER).read() and hook not in php
    assert lib.dwpa_abi_version() == 4
    names = L.VERIFY_KERNEL_NAMES
    assert len(names) == len(set(names)) == 12
    assert [n.split("<")[1] for n in names[:6]] == [n.split("<")[1] for n in names[6:]]  # the same classes twice
    assert all(n.startswith("k_verify<") for n in names[:6]) and all(n.startswith("k_verify_att<") for n in names[6:])
    child = ("import sys; sys.path.insert(0, sys.argv[1]); from dwpa_amd import _lib as L; lib = L.load(); "
             "print(lib.dwpa_debug_verify_kernels(0), lib.dwpa_debug_verify_kernels(1), sorted(L.verify_kernels()), "
             "L.check_hit_records(), L.check_hit_records(reset=True))")
    r = subprocess.run([sys.executable, "-c", child, root], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip() == "0 0 [] 0 0"


def test_debug_scan_work_hook():
    """dwpa_debug_scan_work (the test hook tests/test_gpu_retire_recall.py reads the scan path's derived groups, PBKDF2
    launches and verified line rows from): exported, outside the public header, the PHP cdef and the ABI version, zero
    in a process that has launched nothing, and `reset` returns the counters it clears."""
    import subprocess
    import sys
    lib = L.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    php = open(os.path.join(root, "php", "dwpa22000.php")).read()
    hook = "dwpa_debug_scan_work"
    assert hasattr(lib, hook)
    assert hook not in declared_symbols() and hook not in open(L.HEADER).read() and hook not in php
    assert lib.dwpa_abi_version() == 4
    assert L.SCAN_WORK_NAMES == ("groups_derived", "pbkdf2_launches", "line_rows")
    child = ("import sys; sys.path.insert(0, sys.argv[1]); from dwpa_amd import _lib as L; lib = L.load(); "
             "print(L.scan_work(), L.scan_work(reset=True), L.scan_work()); lib.dwpa_debug_scan_work(None, 1)")
    r = subprocess.run([sys.executable, "-c", child, root], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    zero = str(dict.fromkeys(L.SCAN_WORK_NAMES, 0))
    assert r.stdout.strip() == " ".join([zero] * 3)


def test_debug_crack_loads_hook():
    """dwpa_debug_crack_loads (the test hook tests/test_gpu_fill_recall.py reads the crack loop's loads issued,
    overflowed, empty and scanned from): exported, outside the public header, the PHP cdef and the ABI version, zero
    in a process that has launched nothing, and `reset` returns the counters it clears."""
    import subprocess
    import sys
    lib = L.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    php = open(os.path.join(root, "php", "dwpa22000.php")).read()
    hook = "dwpa_debug_crack_loads"
    assert hasattr(lib, hook)
    assert hook not in declared_symbols() and hook not in open(L.HEADER).read() and hook not in php
    assert lib.dwpa_abi_version() == 4
    assert L.CRACK_LOAD_NAMES == ("loads", "overflowed", "empty", "scanned")
    child = ("import sys; sys.path.insert(0, sys.argv[1]); from dwpa_amd import _lib as L; lib = L.load(); "
             "print(L.crack_loads(), L.crack_loads(reset=True), L.crack_loads()); lib.dwpa_debug_crack_loads(None, 1)")
    r = subprocess.run([sys.executable, "-c", child, root], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    zero = str(dict.fromkeys(L.CRACK_LOAD_NAMES, 0))
    assert r.stdout.strip() == " ".join([zero] * 3)


def test_debug_scan_pmks_hook():
    """dwpa_debug_scan_pmks (the test hook tests/test_gpu_pmk.py reads a scan's PMK buffers with): exported, outside the
    public header, the PHP cdef and the ABI version, and DWPA_E_ARG for a null scan, a null buffer or an unknown source
    before anything touches a device."""
    lib = L.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    php = open(os.path.join(root, "php", "dwpa22000.php")).read()
    hook = "dwpa_debug_scan_pmks"
    assert hasattr(lib, hook) and hook in L.SIGNATURES
    assert hook not in declared_symbols() and hook not in open(L.HEADER).read() and hook not in php
    assert lib.dwpa_abi_version() == 4
    out = (ctypes.c_uint32 * 32)(*([7] * 32))
    fake = ctypes.c_void_p(1)  # never dereferenced: the argument checks come first
    for scan, source, buf in ((None, 0, out), (None, 1, out), (fake, 0, None), (fake, 2, out), (fake, -1, out)):
        assert lib.dwpa_debug_scan_pmks(scan, source, 0, buf, 4, None) == L.DWPA_E_ARG
    assert list(out) == [7] * 32


def test_hc_unhex_matches_oracle():
    import dwpa_amd
    for k in [b"$HEX[414243]", b"$HEX[]", b"$HEX[41424]", b"$HEX[41zz]", b"$HEX[4142]x", b"plain", b"$HEX[00ff]",
              b"$HEX[AbCd]", b"$HEX[", b"1234567"]:
        assert dwpa_amd.hc_unhex(k) == O.hc_unhex(k), k


def test_hash_m22000_matches_oracle():
    import dwpa_amd
    for line in S.CHALLENGE_LINES + [b"WPA*01*a*b*c*d*e*f*g*h*i", b"WPA*01*x", b""]:
        assert dwpa_amd.hash_m22000(line) == O.c_hash_m22000(line)


def test_line_info_long_essid_prefix_and_length():
    """dwpa_line_info.essid holds the first 32 bytes of a longer ESSID and essid_len the full length (PHP accepts
    any even-length hex ESSID, common.php:28-36; the check itself salts with all of it)."""
    import dwpa_amd
    essid = bytes(range(65, 65 + 52))
    line = S.pmkid_line(b"password", essid, bytes(6), bytes([1] * 6))
    info = L.LineInfo()
    assert L.load().dwpa_parse_m22000(line, len(line), 128, L.DWPA_NC_PHP, ctypes.byref(info)) == 0
    assert info.essid_len == 52
    assert bytes(info.essid) == essid[:32]
    d = dwpa_amd.parse_m22000(line)
    assert (d["essid"], d["essid_len"]) == (essid[:32], 52)


def _structs(txt):
    """typedef struct { fields } name;  ->  {name: [normalised field declarations]}"""
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", txt, flags=re.S):
        out[name] = [" ".join(f.split()) for f in body.split(";") if f.strip()]
    return out


def test_php_ffi_cdef_matches_header():
    """php/dwpa22000.php declares the ABI again for FFI::cdef (the server binding, common.php:157-307); its structs
    and prototypes must stay identical to include/dwpa22000.h (PHP is not installed here, so this is the check)."""
    php = open(os.path.join(os.path.dirname(L.HEADER), "..", "php", "dwpa22000.php")).read()
    cdef = re.search(r"<<<'CDEF'(.*?)CDEF;", php, flags=re.S).group(1)
    hdr = open(L.HEADER).read()
    hs, ps = _structs(hdr), _structs(cdef)
    assert ps, "no structs in the PHP cdef"
    for name, fields in ps.items():
        assert hs.get(name) == fields, name
    def norm(s):
        s = " ".join(re.sub(r"/\*.*?\*/", "", s, flags=re.S).split())
        return re.sub(r"\s+([,);])", r"\1", s)
    for proto in re.findall(r"^\s*((?:int|const char \*)\s*dwpa_\w+\(.*?\);)", cdef, flags=re.M | re.S):
        assert norm(proto) in norm(hdr), proto


def test_nc_bound():
    """DWPA_NC_MAX: the header's bound, what it admits, and DWPA_E_ARG above it for EAPOL lines only (PHP ignores nc
    for PMKID lines); the PHP wrapper answers such a job with the original check_key_m22000 (codes <= -10)."""
    from dwpa_amd import m22000 as M
    hdr = open(L.HEADER).read()
    assert re.search(r"#define DWPA_NC_MAX (\d+)", hdr).group(1) == str(L.DWPA_NC_MAX)
    pmkid, eapol = S.CHALLENGE_LINES
    info = M.parse_m22000(eapol, L.DWPA_NC_MAX)
    assert info["attempts"] == 1 + 4 * ((L.DWPA_NC_MAX >> 1) + 1)
    assert M.parse_m22000(eapol, L.DWPA_NC_MAX, L.DWPA_NC_HASHCAT)["attempts"] == 1 + 4 * L.DWPA_NC_MAX
    assert M.parse_m22000(eapol, L.DWPA_NC_MAX + 1) == L.DWPA_E_ARG
    assert M.parse_m22000(eapol, 2**31 - 1, L.DWPA_NC_HASHCAT) == L.DWPA_E_ARG
    assert M.parse_m22000(eapol, -(2**31))["attempts"] == 1
    assert M.parse_m22000(pmkid, 2**31 - 1)["attempts"] == 1
    assert L.DWPA_E_ARG <= -10  # so php/dwpa22000.php falls back, never answers False


_NOMEM_CHILD = r"""
import ctypes, resource, sys
sys.path.insert(0, sys.argv[1])
from dwpa_amd import _lib as L
lib = L.load()
text = b":\n" * 20_000_000  # 40 MB of rules: the parsed set needs several times that
c = L.RulesCounts()
soft, hard = resource.getrlimit(resource.RLIMIT_AS)
vm = int([l for l in open("/proc/self/status") if l.startswith("VmSize")][0].split()[1]) * 1024
resource.setrlimit(resource.RLIMIT_AS, (vm + (64 << 20), hard))
rc = lib.dwpa_rules_count_ex(text, len(text), ctypes.byref(c))
print(rc)
"""


def test_no_exception_crosses_the_c_abi():
    """A host allocation that fails inside the library (std::bad_alloc) comes back as DWPA_E_NOMEM instead of
    aborting the caller's process (a PHP-FPM worker, help_crack): the child caps its address space, then asks the
    library to parse a rules text whose tables do not fit."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _NOMEM_CHILD, root], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip() == str(L.DWPA_E_NOMEM), (r.stdout, r.stderr[-2000:])


def test_python_nc_outside_int32_is_refused():
    """ctypes would wrap an nc outside int32 into a different window; the Python API refuses it before any call."""
    import dwpa_amd
    pmkid = S.CHALLENGE_LINES[0]
    for nc in (2**31, -2**31 - 1, 2**40 + 8):
        with pytest.raises(L.DwpaError) as e:
            dwpa_amd.check_key_m22000(pmkid, [b"aaaa1234"], False, nc)
        assert e.value.code == L.DWPA_E_ARG
        with pytest.raises(L.DwpaError):
            dwpa_amd.check_batch([(pmkid, [b"aaaa1234"], False, nc)])


def test_plain_c_client(tmp_path):
    """The header is plain C99 (what PHP FFI::cdef and any C caller consume): tools/abi_c_client.c compiles against it
    with -Wall -Wextra -Werror, links libdwpa22000.so and checks the reference's challenge (help_crack.py:692-699) with
    dwpa_check_m22000 and dwpa_check_batch, the host backend allowed (no GPU here: it answers)."""
    import subprocess
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "abi_c_client"
    lib = os.path.join(ROOT, "dwpa_amd", "lib")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "abi_c_client.c"), "-L", lib, "-ldwpa22000",
                    "-Wl,-rpath," + lib, "-o", str(exe)], check=True)
    env = dict(os.environ, DWPA_HOST_MAX_PMKS="1000000000")
    r = subprocess.run([str(exe)] + [l.decode() for l in S.CHALLENGE_LINES], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "line 1: rc 1 key_index 1 nc_valid 1 nc 4 endian 2" in r.stdout and "batch: both hit" in r.stdout
