"""``python -m dwpa_amd.chain HASHFILE PART [PART ...]`` -- the chain attack on libdwpa22000.so: up to four word lists
and masks joined left to right on the GPU.

Each PART is ``list:PATH`` (a plain or gzip wordlist, ``$HEX[]`` words decoded) or ``mask:MASK`` (hashcat's mask
language, ``?1``..``?4`` shared by all mask parts).  A candidate is one choice of every part, concatenated in the
order of the parts; candidate ``i`` is the ``i``-th element of ``itertools.product`` over the parts (the last part
runs fastest), and ``-s`` / ``-l`` name a window of those indices.  Candidates with a list word above 63 bytes or a
total length outside 8..63 are dropped on the GPU.

The options are spelled as ``python -m dwpa_amd.mask`` spells them: ``-1``..``-4``, ``--hex-charset``, ``-s/--skip``,
``-l/--limit``, ``-d`` (devices, numbered from 1), ``-o``, ``--nonce-error-corrections``, ``--batch``.  The exit status
is the call's return code (0 every hashline cracked, 1 exhausted, 255 error).  ``--keyspace`` and ``--stdout`` take no
hash file and stay on the host; ``--stdout`` prints every candidate of the window, unfiltered, in id order.

Every list is held whole in device memory; rules on parts and ``--increment`` are not available.
"""
from __future__ import annotations

import argparse
import os
import sys

from . import _lib as L
from . import m22000 as M
from .mask import _custom_sets, _devices, _words


def _parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m dwpa_amd.chain", description=__doc__.split("\n\n")[0],
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("args", nargs="*", metavar="[HASHFILE] PART",
                   help="an m22000 hash file and 1..4 parts, each list:PATH or mask:MASK; the parts alone with "
                        "--keyspace / --stdout")
    for k in "1234":
        p.add_argument("-" + k, "--custom-charset" + k, dest="c" + k, metavar="CS", help="custom set ?" + k)
    p.add_argument("--hex-charset", action="store_true", help="the custom sets are given in hex")
    p.add_argument("-s", "--skip", type=int, default=0, help="first index of the keyspace to run")
    p.add_argument("-l", "--limit", type=int, default=0, help="number of indices to run (0: to the end)")
    p.add_argument("-d", "--backend-devices", default="", metavar="LIST", help="devices to use, numbered from 1: 1,2")
    p.add_argument("-o", "--outfile", default="help_crack.key")
    p.add_argument("--nonce-error-corrections", type=int, default=8, metavar="N")
    p.add_argument("--batch", type=int, default=0, help="raw candidates per launch (0: the library's default)")
    p.add_argument("--keyspace", action="store_true",
                   help="print the chain's keyspace (the product of the lists' word counts and the masks' keyspaces) "
                        "and exit")
    p.add_argument("--stdout", action="store_true",
                   help="write the candidates of [skip, skip + limit) to standard output, one per line as raw "
                        "bytes, unfiltered, and exit")
    return p


def _fail(msg: str) -> int:
    print("dwpa_amd.chain: " + msg, file=sys.stderr)
    return 255


def _parts(ops):
    """[(kind, text)] of the PART operands, or the exit status after a message."""
    if not 1 <= len(ops) <= L.DWPA_CHAIN_MAX_PARTS:
        return _fail("expected 1..%d parts, each list:PATH or mask:MASK" % L.DWPA_CHAIN_MAX_PARTS)
    parts = []
    for op in ops:
        if op.startswith("list:"):
            path = op[5:]
            if not os.path.isfile(path) or not os.access(path, os.R_OK):
                return _fail(f"list {path}: cannot be opened")
            parts.append((L.DWPA_CHAIN_LIST, path))
        elif op.startswith("mask:"):
            parts.append((L.DWPA_CHAIN_MASK, os.fsencode(op[5:])))
        else:
            return _fail(f"part {op}: expected list:PATH or mask:MASK")
    return parts


def _candidates(choices, radices, first: int, count: int):
    """Candidates first .. first + count - 1: an odometer over the parts, started at chain_split's digits.
    choices[p](d) gives part p's bytes at digit d."""
    digits = M.chain_split(radices, first)
    cur = [c(d) for c, d in zip(choices, digits)]
    for n in range(count):
        yield b"".join(cur)
        p = len(digits) - 1
        while p >= 0 and n + 1 < count:
            digits[p] += 1
            if digits[p] < radices[p]:
                cur[p] = choices[p](digits[p])
                break
            digits[p] = 0
            cur[p] = choices[p](0)
            p -= 1


def main(argv=None) -> int:
    p = _parser()
    try:
        a = p.parse_args(argv)
    except SystemExit as e:  # argparse: 0 after --help, 2 for bad arguments
        return 0 if e.code in (0, None) else 255
    host_only = a.keyspace or a.stdout
    if not host_only and not a.args:
        return _fail("expected HASHFILE PART [PART ...]")
    parts = _parts(a.args if host_only else a.args[1:])
    if isinstance(parts, int):
        return parts
    custom = _custom_sets(a)
    if isinstance(custom, int):
        return custom
    if a.skip < 0 or a.limit < 0:
        return _fail("negative argument")
    try:
        for kind, text in parts:
            if kind == L.DWPA_CHAIN_MASK:
                M.mask_keyspace(text, custom)  # refuses a bad mask before any list is read
        if host_only:
            lists = [list(_words(text)) if kind == L.DWPA_CHAIN_LIST else None for kind, text in parts]
            radices = [M.mask_keyspace(text, custom) if ws is None else len(ws) for (kind, text), ws in zip(parts, lists)]
            keyspace = M.chain_keyspace(radices)
            if a.keyspace:
                print(keyspace)
                return 0
            if keyspace and a.skip >= keyspace:
                return _fail("--skip is not below the keyspace")
            count = max(0, keyspace - a.skip)
            if a.limit:
                count = min(count, a.limit)
            choices = [(lambda d, m=text: M.mask_candidate(m, d, custom)) if ws is None else ws.__getitem__
                       for (kind, text), ws in zip(parts, lists)]
            out = sys.stdout.buffer
            if count:
                for c in _candidates(choices, radices, a.skip, count):
                    out.write(c + b"\n")
            out.flush()
            return 0
        devices = _devices(a)
        if devices < 0:
            return 255
        rc, status = M.crack_chain(a.args[0], parts, custom, a.skip, a.limit, a.nonce_error_corrections, a.outfile,
                                   device_mask=devices, batch=a.batch)
    except (L.DwpaError, OSError) as e:
        return _fail(str(e))
    if rc in (0, 1):
        st = M.crack_stats()
        print("dwpa_amd.chain: %s, %d/%d hashlines cracked, %d words, %d candidates in %.1f s" %
              ("cracked" if rc == 0 else "exhausted", st["cracked"], st["hashes"], st["words"], st["candidates"],
               st["seconds"]), file=sys.stderr)
        return rc
    return _fail("crack_chain failed")


if __name__ == "__main__":
    sys.exit(main())
