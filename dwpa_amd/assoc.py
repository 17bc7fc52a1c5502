"""``python -m dwpa_amd.assoc HASHFILE [ASSOCFILE] [--single] [-r RULES]`` -- the association attack on
libdwpa22000.so: every net of the hash file against its own words, joined with the rules on the GPU (hashcat's ``-a 9``;
the per-net pass of ``web/rkg.php``).

A net is the pair (ESSID, MAC_AP) of a usable hashline; nets are numbered by first appearance.  ASSOCFILE (plain or
gzip) holds one ``MAC_AP:WORD`` per line -- 12 hex digits, a colon, the word, ``$HEX[]`` decoded for the word only --
for instance the output of a router keygen run per BSSID.  ``--single`` adds the built-in generator's words to every
net: the last 12, 10 and 8 hex digits of BSSID - 1, BSSID and BSSID + 1 in both cases, and the ESSID, ESSID1, ESSID123
and ESSID! as written, in upper and in lower case.  At least one of the two sources is required.  Within a net a word
that repeats an earlier one is dropped.

Net ``n`` with ``W`` words owns ``W x R`` consecutive indices under ``R`` rules (1 without ``-r``), rule-major with the
word fastest; ``-s`` / ``-l`` name a window of those indices.  A candidate is derived with its own net's ESSID and
verified against that net's lines only.

The options are spelled as ``python -m dwpa_amd.table`` spells them: ``-s/--skip``, ``-l/--limit``, ``-d`` (devices,
numbered from 1), ``-o``, ``--nonce-error-corrections``, ``--batch``.  The exit status is the call's return code (0
every hashline cracked, 1 exhausted, 255 error).  ``--keyspace`` and ``--stdout`` read the hash file -- the nets come
from it -- but crack nothing and need no device; ``--stdout`` prints the window's candidates in index order, one per
line as raw bytes, and omits the indices that give none (a rule that rejects, a result outside 8..63 bytes).
"""
from __future__ import annotations

import argparse
import os
import sys

from . import _lib as L
from . import m22000 as M
from .mask import _devices


def _parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m dwpa_amd.assoc", description=__doc__.split("\n\n")[0],
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("args", nargs="*", metavar="HASHFILE [ASSOCFILE]",
                   help="an m22000 hash file and, optionally, a file of MAC_AP:WORD lines")
    p.add_argument("--single", action="store_true", help="add the built-in generator's words (BSSID and ESSID derived)")
    p.add_argument("-r", "--rules-file", default=None, metavar="FILE", help="hashcat rules applied to every word")
    p.add_argument("-s", "--skip", type=int, default=0, help="first index of the keyspace to run")
    p.add_argument("-l", "--limit", type=int, default=0, help="number of indices to run (0: to the end)")
    p.add_argument("-d", "--backend-devices", default="", metavar="LIST", help="devices to use, numbered from 1: 1,2")
    p.add_argument("-o", "--outfile", default="help_crack.key")
    p.add_argument("--nonce-error-corrections", type=int, default=8, metavar="N")
    p.add_argument("--batch", type=int, default=0, help="candidates per launch (0: the library's default)")
    p.add_argument("--keyspace", action="store_true", help="print the keyspace (the sum of words x rules over the nets) "
                                                           "and exit")
    p.add_argument("--stdout", action="store_true",
                   help="write the candidates of [skip, skip + limit) to standard output, one per line as raw bytes, "
                        "and exit")
    return p


def _fail(msg: str) -> int:
    print("dwpa_amd.assoc: " + msg, file=sys.stderr)
    return 255


_CHUNK = 1 << 16


def _host(a, hash_file, assoc_file) -> int:
    """--keyspace / --stdout: nothing but the host."""
    keyspace = M.assoc_plan(hash_file, assoc_file, a.single, a.rules_file)["keyspace"]
    if a.keyspace:
        print(keyspace)
        return 0
    if keyspace and a.skip >= keyspace:
        return _fail("--skip is not below the keyspace")
    count = max(0, keyspace - a.skip)
    if a.limit:
        count = min(count, a.limit)
    out = sys.stdout.buffer
    for first in range(a.skip, a.skip + count, _CHUNK):
        m = min(_CHUNK, a.skip + count - first)
        cands = M.assoc_candidates(hash_file, range(first, first + m), assoc_file, a.single, a.rules_file)
        out.write(b"".join(c + b"\n" for c, _ in cands if c is not None))
    out.flush()
    return 0


def main(argv=None) -> int:
    p = _parser()
    try:
        a = p.parse_args(argv)
    except SystemExit as e:  # argparse: 0 after --help, 2 for bad arguments
        return 0 if e.code in (0, None) else 255
    if len(a.args) not in (1, 2):
        return _fail("expected HASHFILE [ASSOCFILE]")
    hash_file, assoc_file = a.args[0], a.args[1] if len(a.args) == 2 else None
    if assoc_file is None and not a.single:
        return _fail("expected at least one source: ASSOCFILE, --single, or both")
    if a.skip < 0 or a.limit < 0:
        return _fail("-s and -l take non-negative numbers")
    for what, path in (("hash file", hash_file), ("association file", assoc_file), ("rules", a.rules_file)):
        if path is not None and (not os.path.isfile(path) or not os.access(path, os.R_OK)):
            return _fail(f"{what} {path}: cannot be opened")
    try:
        if a.keyspace or a.stdout:
            return _host(a, hash_file, assoc_file)
        devices = _devices(a)
        if devices < 0:
            return 255
        rc = M.crack_assoc(hash_file, assoc_file, a.single, a.rules_file, a.skip, a.limit, a.nonce_error_corrections,
                           a.outfile, device_mask=devices, batch=a.batch)
    except (L.DwpaError, OSError) as e:
        return _fail(str(e))
    if rc in (0, 1):
        st = M.crack_stats()
        print("dwpa_amd.assoc: %s, %d/%d hashlines cracked, %d words, %d candidates in %.1f s" %
              ("cracked" if rc == 0 else "exhausted", st["cracked"], st["hashes"], st["words"], st["candidates"],
               st["seconds"]), file=sys.stderr)
        return rc
    return _fail("crack_assoc failed")


if __name__ == "__main__":
    sys.exit(main())
