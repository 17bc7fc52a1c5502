"""``python -m dwpa_amd.table HASHFILE DICT (--table-file FILE | --toggle)`` -- the table attack on libdwpa22000.so:
every combination of per-byte alternatives of every word, generated on the GPU (hashcat-legacy's ``-a 5 --table-file``;
``--toggle`` is its toggle-case attack ``-a 2``).

The table file holds one mapping per line, ``K=V``, with ``K`` and ``V`` each one literal byte or ``\\xHH``; a byte's
alternatives are its ``V`` s in file order (at most 16), a byte the file never names stays as it is, and a key keeps
its original only if the file says so (``a=a``).  ``===`` maps ``=`` to ``=`` and ``#=#`` is a mapping: there are no
comments.  Replacements are one byte each, so a candidate has its word's length.  ``--toggle`` is the built-in table
that maps every ASCII letter to itself and its other case.

DICT is a plain or gzip wordlist (``$HEX[]`` words decoded), held whole in device memory.  A word is kept when it has
8..63 bytes and at most ``--table-max`` combinations (default 2^32 - 1); the others own no indices.  Candidate ``i``:
the kept words in list order, within a word ``itertools.product`` over its bytes' alternative lists (the last position
runs fastest); ``-s`` / ``-l`` name a window of those indices.

The options are spelled as ``python -m dwpa_amd.chain`` spells them: ``-s/--skip``, ``-l/--limit``, ``-d`` (devices,
numbered from 1), ``-o``, ``--nonce-error-corrections``, ``--batch``.  The exit status is the call's return code (0
every hashline cracked, 1 exhausted, 255 error).  ``--keyspace`` and ``--stdout`` take no hash file and stay on the
host; ``--stdout`` prints exactly the window's candidates in id order.
"""
from __future__ import annotations

import argparse
import ctypes
import os
import sys
import tempfile

from . import _lib as L
from . import m22000 as M
from .mask import _devices, _words


def _parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m dwpa_amd.table", description=__doc__.split("\n\n")[0],
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("args", nargs="*", metavar="[HASHFILE] DICT",
                   help="an m22000 hash file and a wordlist; the wordlist alone with --keyspace / --stdout")
    p.add_argument("--table-file", default=None, metavar="FILE", help="the substitution table, K=V lines")
    p.add_argument("--toggle", action="store_true", help="the built-in table: every ASCII letter in both cases")
    p.add_argument("--table-max", type=int, default=0, metavar="N",
                   help="drop words with more than N combinations (0: 2^32 - 1)")
    p.add_argument("-s", "--skip", type=int, default=0, help="first index of the keyspace to run")
    p.add_argument("-l", "--limit", type=int, default=0, help="number of indices to run (0: to the end)")
    p.add_argument("-d", "--backend-devices", default="", metavar="LIST", help="devices to use, numbered from 1: 1,2")
    p.add_argument("-o", "--outfile", default="help_crack.key")
    p.add_argument("--nonce-error-corrections", type=int, default=8, metavar="N")
    p.add_argument("--batch", type=int, default=0, help="candidates per launch (0: the library's default)")
    p.add_argument("--keyspace", action="store_true", help="print the keyspace (the sum of the kept words' counts) and exit")
    p.add_argument("--stdout", action="store_true",
                   help="write the candidates of [skip, skip + limit) to standard output, one per line as raw bytes, "
                        "and exit")
    return p


def _fail(msg: str) -> int:
    print("dwpa_amd.table: " + msg, file=sys.stderr)
    return 255


_CHUNK = 1 << 14


def _host(a, table: bytes, path: str) -> int:
    """--keyspace / --stdout: nothing but the host."""
    words = list(_words(path))
    ks = M.table_keyspace(table, words, word_max=a.table_max)
    keyspace = ks["keyspace"]
    if a.keyspace:
        print(keyspace)
        return 0
    if keyspace and a.skip >= keyspace:
        return _fail("--skip is not below the keyspace")
    count = max(0, keyspace - a.skip)
    if a.limit:
        count = min(count, a.limit)
    lib = L.load()
    arr, n, keep = M._word_array(words)  # one array for every chunk of the window
    out = sys.stdout.buffer
    buf = ctypes.create_string_buffer(64 * _CHUNK)
    lens = (ctypes.c_uint32 * _CHUNK)()
    idx = (ctypes.c_uint64 * _CHUNK)()
    for first in range(a.skip, a.skip + count, _CHUNK):
        m = min(_CHUNK, a.skip + count - first)
        for k in range(m):
            idx[k] = first + k
        L.check(lib.dwpa_table_candidates(table, len(table), arr, n, 8, 63, a.table_max, idx, m, buf, lens),
                "table_candidates")
        raw = buf.raw
        out.write(b"".join(raw[64 * k:64 * k + lens[k]] + b"\n" for k in range(m)))
    out.flush()
    return 0


def main(argv=None) -> int:
    p = _parser()
    try:
        a = p.parse_args(argv)
    except SystemExit as e:  # argparse: 0 after --help, 2 for bad arguments
        return 0 if e.code in (0, None) else 255
    host_only = a.keyspace or a.stdout
    if len(a.args) != (1 if host_only else 2):
        return _fail("expected " + ("DICT" if host_only else "HASHFILE DICT"))
    if (a.table_file is None) == (not a.toggle):
        return _fail("expected one of --table-file FILE and --toggle")
    if a.skip < 0 or a.limit < 0 or not 0 <= a.table_max < 2**32:
        return _fail("-s and -l take non-negative numbers, --table-max 0..2^32 - 1")
    path = a.args[-1]
    if not os.path.isfile(path) or not os.access(path, os.R_OK):
        return _fail(f"list {path}: cannot be opened")
    try:
        if a.toggle:
            table = M.table_builtin("toggle")
        else:
            if not os.path.isfile(a.table_file) or not os.access(a.table_file, os.R_OK):
                return _fail(f"table {a.table_file}: cannot be opened")
            with open(a.table_file, "rb") as f:
                table = f.read()
        M.table_parse(table)  # refuses a bad table, naming its line, before the list is read
        if host_only:
            return _host(a, table, path)
        devices = _devices(a)
        if devices < 0:
            return 255
        with tempfile.TemporaryDirectory() as tmp:  # the built-in table goes to the library as a file
            tfile = a.table_file
            if a.toggle:
                tfile = os.path.join(tmp, "toggle.table")
                with open(tfile, "wb") as f:
                    f.write(table)
            rc = M.crack_table(a.args[0], path, tfile, a.table_max, a.skip, a.limit, a.nonce_error_corrections,
                               a.outfile, device_mask=devices, batch=a.batch)
    except (L.DwpaError, OSError) as e:
        return _fail(str(e))
    if rc in (0, 1):
        st = M.crack_stats()
        print("dwpa_amd.table: %s, %d/%d hashlines cracked, %d words, %d candidates in %.1f s" %
              ("cracked" if rc == 0 else "exhausted", st["cracked"], st["hashes"], st["words"], st["candidates"],
               st["seconds"]), file=sys.stderr)
        return rc
    return _fail("crack_table failed")


if __name__ == "__main__":
    sys.exit(main())
