"""``python -m dwpa_amd.mask HASHFILE MASK`` -- hashcat's ``-m 22000 -a 3`` mask attack on libdwpa22000.so, its
hybrid attacks ``-a 6 HASHFILE DICT [DICT...] MASK`` (word + mask) and ``-a 7 HASHFILE MASK DICT [DICT...]`` (mask +
word), and its combinator attack ``-a 1 HASHFILE LEFT RIGHT`` (word of one list + word of another).

It takes hashcat's spellings: ``-1``..``-4`` custom sets, ``-s/--skip``, ``-l/--limit``, ``-i --increment-min
--increment-max``, ``-d`` (devices, numbered from 1), ``-o``, ``--nonce-error-corrections``.  The exit status is the
call's return code (0 every hashline cracked, 1 exhausted, 255 error).  ``--keyspace`` and ``--stdout`` need no hash
file and stay on the host.

With ``-a 6`` / ``-a 7`` the dictionaries are plain or gzip wordlists (``$HEX[]`` words decoded); ``--stdout`` then
takes no hash file (``-a 6 --stdout DICT... MASK``) and prints every word x mask candidate, unfiltered, word-major
with the mask index fastest.  ``-s``, ``-l``, ``-i`` and ``--keyspace`` belong to ``-a 3`` only.

With ``-a 1`` every candidate is a word of LEFT followed by a word of RIGHT.  ``--amplifier right`` (the default)
holds RIGHT whole in device memory and streams LEFT; ``--amplifier left`` holds LEFT and streams RIGHT, for a RIGHT
too big to hold.  The candidates are the same, their order differs: the streamed list's words are the outer loop.
``-a 1 --stdout LEFT RIGHT`` takes no hash file and prints every pair, unfiltered, in that order.  ``-s``, ``-l``,
``-i``, ``--keyspace``, ``-1``..``-4`` and hashcat's single rules ``-j`` / ``-k`` are not available with ``-a 1``.

The candidates of a mask are hashcat's; their ORDER is the library's own (last position fastest, Python's
``itertools.product`` order), so ``-s`` / ``-l`` windows do not name the candidates hashcat's windows name.

``--markov FILE`` walks an ``-a 3`` mask in Markov order instead: every digit chooses from the model's ranking of the
bytes that follow the byte before it, most likely first, and ``-t / --markov-threshold N`` cuts every position down to
its N most likely bytes.  ``-i``, ``-s`` / ``-l`` (over the thresholded keyspace), ``--keyspace`` (with ``-t`` it needs
no model) and ``--stdout`` follow.  FILE comes from ``python -m dwpa_amd.markov train``: there are no built-in
statistics and hashcat's ``hashcat.hcstat2`` is not read, so this order is the library's own as well.
"""
from __future__ import annotations

import argparse
import gzip
import os
import sys

from . import _lib as L
from . import m22000 as M


def _parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m dwpa_amd.mask", description=__doc__.split("\n\n")[0],
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("args", nargs="+", metavar="[HASHFILE] MASK",
                   help="an m22000 hash file and a mask (?l ?u ?d ?h ?H ?s ?a ?b ?? ?1..?4, other bytes literal); "
                        "the mask alone with --keyspace / --stdout")
    p.add_argument("-a", "--attack-mode", type=int, default=3, metavar="N",
                   help="3 mask (default); 6 wordlist + mask: HASHFILE DICT [DICT...] MASK; 7 mask + wordlist: "
                        "HASHFILE MASK DICT [DICT...]; 1 combinator: HASHFILE LEFT RIGHT")
    p.add_argument("--amplifier", default="right", metavar="SIDE",
                   help="-a 1: the list held whole in device memory, right (default) or left; the other is streamed")
    p.add_argument("-j", "--rule-left", default=None, metavar="RULE", help="hashcat's -a 1 single rule: not supported here (python -m dwpa_amd.chain takes rule:TEXT "
                        "after a list: part)")
    p.add_argument("-k", "--rule-right", default=None, metavar="RULE", help="hashcat's -a 1 single rule: not supported")
    for k in "1234":
        p.add_argument("-" + k, "--custom-charset" + k, dest="c" + k, metavar="CS", help="custom set ?" + k)
    p.add_argument("--hex-charset", action="store_true", help="the custom sets are given in hex")
    p.add_argument("-s", "--skip", type=int, default=0, help="first index of the keyspace to run")
    p.add_argument("-l", "--limit", type=int, default=0, help="number of indices to run (0: to the end)")
    p.add_argument("-i", "--increment", action="store_true", help="run the mask's prefixes, shortest first")
    p.add_argument("--increment-min", type=int, default=0, metavar="N")
    p.add_argument("--increment-max", type=int, default=0, metavar="N")
    p.add_argument("-d", "--backend-devices", default="", metavar="LIST", help="devices to use, numbered from 1: 1,2")
    p.add_argument("-o", "--outfile", default="help_crack.key")
    p.add_argument("--nonce-error-corrections", type=int, default=8, metavar="N")
    p.add_argument("--batch", type=int, default=0, help="candidate slots per launch (0: the library's default)")
    p.add_argument("--markov", default=None, metavar="FILE",
                   help="-a 3: walk the mask in Markov order by this model (python -m dwpa_amd.markov train)")
    p.add_argument("-t", "--markov-threshold", type=int, default=None, metavar="N", dest="threshold",
                   help="-a 3: cut every position down to its N most likely bytes (1..256); needs --markov, except "
                        "with --keyspace")
    p.add_argument("--keyspace", action="store_true",
                   help="print the mask's whole keyspace (the number of candidates) and exit.  hashcat prints a "
                        "reduced figure for -a 3: the count its host loop steps through, without the part its "
                        "kernels amplify")
    p.add_argument("--stdout", action="store_true",
                   help="write the candidates of [skip, skip + limit) to standard output, one per line as raw "
                        "bytes, and exit")
    return p


def _fail(msg: str) -> int:
    print("dwpa_amd.mask: " + msg, file=sys.stderr)
    return 255


def main(argv=None) -> int:
    p = _parser()
    try:
        a = p.parse_args(argv)
    except SystemExit as e:  # argparse: 0 after --help, 2 for bad arguments
        return 0 if e.code in (0, None) else 255
    if a.rule_left is not None or a.rule_right is not None:
        return _fail("the single rules -j / -k are not supported: python -m dwpa_amd.chain takes rule:TEXT or rules:FILE "
                     "after a list: part")
    if a.attack_mode in (1, 6, 7) and (a.markov is not None or a.threshold is not None):
        return _fail(f"--markov / -t belong to -a 3: not available with -a {a.attack_mode}")
    if a.threshold is not None and not 1 <= a.threshold <= 256:
        return _fail("-t takes 1..256")
    if a.attack_mode == 1:
        return _combinator(a)
    if a.attack_mode in (6, 7):
        return _hybrid(a)
    if a.attack_mode != 3:
        return _fail("-a takes 1 (combinator), 3 (mask), 6 (wordlist + mask) or 7 (mask + wordlist)")
    host_only = a.keyspace or a.stdout
    if not (len(a.args) == 2 or (host_only and len(a.args) == 1)):
        return _fail("expected HASHFILE MASK" + (" or MASK" if host_only else ""))
    mask = os.fsencode(a.args[-1])
    custom = _custom_sets(a)
    if isinstance(custom, int):
        return custom
    increment = None
    if a.increment:
        increment = (a.increment_min or 1, a.increment_max)
    elif a.increment_min or a.increment_max:
        return _fail("--increment-min / --increment-max need -i")
    if a.skip < 0 or a.limit < 0 or a.increment_min < 0 or a.increment_max < 0:
        return _fail("negative argument")
    if increment and increment[1] and increment[0] > increment[1]:
        return _fail("--increment-min is above --increment-max")
    if increment and (a.skip or a.limit):
        return _fail("--increment cannot be combined with --skip / --limit")
    t = a.threshold or 0
    if t and a.markov is None and not a.keyspace:
        return _fail("-t needs --markov FILE: there are no built-in statistics; train a model with "
                     "python -m dwpa_amd.markov train OUT.dwmk DICT [DICT ...]")
    try:
        npos = M.mask_positions(mask, custom, t)
        keyspace = M.mask_keyspace(mask, custom, t)
        if host_only:
            if increment:
                lo, hi = increment[0], min(increment[1] or npos, npos)
                if lo > hi:
                    return _fail("--increment-min is above the mask's length")
                masks = [_prefix(mask, n) for n in range(lo, hi + 1)]
            else:
                masks = [mask]
            if a.keyspace:
                print(sum(M.mask_keyspace(m, custom, t) for m in masks))
                return 0
            model = None if a.markov is None else M.markov_load(a.markov)
            out = sys.stdout.buffer
            for m in masks:
                k = M.mask_keyspace(m, custom, t)
                if a.skip >= k:
                    return _fail("--skip is not below the keyspace")
                end = min(k, a.skip + a.limit) if a.limit else k
                if model is None:
                    for i in range(a.skip, end):
                        out.write(M.mask_candidate(m, i, custom) + b"\n")
                else:  # the Markov order, 4096 indices per call: the model is validated once per call
                    for i in range(a.skip, end, 4096):
                        out.write(b"".join(c + b"\n" for c in M.mask_candidates(m, range(i, min(end, i + 4096)), custom,
                                                                                model, t)))
            out.flush()
            return 0
        devices = _devices(a)
        if devices < 0:
            return 255
        if not increment and a.skip >= keyspace:
            return _fail("--skip is not below the keyspace")
        rc = M.crack_mask(a.args[0], mask, custom, a.skip, a.limit, increment, a.nonce_error_corrections, a.outfile,
                          device_mask=devices, batch=a.batch, markov=a.markov, threshold=t)
    except L.DwpaError as e:
        return _fail(str(e))
    if rc in (0, 1):
        st = M.crack_stats()
        print("dwpa_amd.mask: %s, %d/%d hashlines cracked, %d candidates in %.1f s" %
              ("cracked" if rc == 0 else "exhausted", st["cracked"], st["hashes"], st["candidates"], st["seconds"]),
              file=sys.stderr)
        return rc
    return _fail("crack_mask failed")


def _custom_sets(a):
    """The sets -1..-4 as bytes (None: not given), or the exit status after a message."""
    custom = []
    for k in "1234":
        c = getattr(a, "c" + k)
        if c is None:
            custom.append(None)
        elif a.hex_charset:
            try:
                custom.append(bytes.fromhex(c))
            except ValueError:
                return _fail(f"-{k}: not hex")
        else:
            custom.append(os.fsencode(c))
    return custom


def _devices(a) -> int:
    """-d as a device mask (0: every device), or -1 after a message."""
    devices = 0
    for d in a.backend_devices.split(","):
        if d.strip():
            if not d.strip().isdigit() or int(d) < 1 or int(d) > 32:
                _fail("-d takes device numbers from 1")
                return -1
            devices |= 1 << (int(d) - 1)
    return devices


def _words(path: str):
    """The words of a wordlist as the library's reader cuts them: plain or gzip, one per line, "\\n" or "\\r\\n", a
    last line without newline counted, empty lines kept, $HEX[] decoded."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:2] == b"\x1f\x8b":
        data = gzip.decompress(data)
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    for w in lines:
        if w.endswith(b"\r"):
            w = w[:-1]
        if len(w) > 5 and w.startswith(b"$HEX[") and w.endswith(b"]"):
            w = M.hc_unhex(w)
        yield w


def _hybrid(a) -> int:
    """-a 6 / -a 7: argument order as hashcat's, the mask last (6) or first (7) among the attack's operands."""
    mode = a.attack_mode
    if a.skip or a.limit or a.increment or a.increment_min or a.increment_max or a.keyspace:
        return _fail(f"-s, -l, -i and --keyspace are not available with -a {mode}")
    ops = a.args if a.stdout else a.args[1:]
    if len(ops) < 2 or (not a.stdout and len(a.args) < 3):
        return _fail(("expected " + ("" if a.stdout else "HASHFILE ")) +
                     ("DICT [DICT...] MASK" if mode == 6 else "MASK DICT [DICT...]"))
    mask = os.fsencode(ops[-1] if mode == 6 else ops[0])
    dicts = ops[:-1] if mode == 6 else ops[1:]
    custom = _custom_sets(a)
    if isinstance(custom, int):
        return custom
    try:
        keyspace = M.mask_keyspace(mask, custom)
        for d in dicts:
            if not os.path.isfile(d) or not os.access(d, os.R_OK):
                return _fail(f"dictionary {d}: cannot be opened")
        if a.stdout:
            out = sys.stdout.buffer
            for d in dicts:
                for w in _words(d):
                    for i in range(keyspace):
                        m = M.mask_candidate(mask, i, custom)
                        out.write((w + m if mode == 6 else m + w) + b"\n")
            out.flush()
            return 0
        devices = _devices(a)
        if devices < 0:
            return 255
        rc, status = M.crack_hybrid(a.args[0], dicts, mask, custom, mode, a.nonce_error_corrections, a.outfile,
                                    device_mask=devices, batch=a.batch)
    except (L.DwpaError, OSError) as e:
        return _fail(str(e))
    if rc in (0, 1):
        st = M.crack_stats()
        print("dwpa_amd.mask: %s, %d/%d hashlines cracked, %d words, %d candidates in %.1f s" %
              ("cracked" if rc == 0 else "exhausted", st["cracked"], st["hashes"], st["words"], st["candidates"],
               st["seconds"]), file=sys.stderr)
        return rc
    return _fail("crack_hybrid failed")


def _combinator(a) -> int:
    """-a 1: HASHFILE LEFT RIGHT as hashcat's; --stdout takes the two lists alone."""
    if a.skip or a.limit or a.increment or a.increment_min or a.increment_max or a.keyspace:
        return _fail("-s, -l, -i and --keyspace are not available with -a 1")
    if any(getattr(a, "c" + k) is not None for k in "1234") or a.hex_charset:
        return _fail("-1..-4 belong to a mask: not available with -a 1")
    if a.amplifier not in ("right", "left"):
        return _fail("--amplifier takes right or left")
    side = L.DWPA_COMBI_AMP_RIGHT if a.amplifier == "right" else L.DWPA_COMBI_AMP_LEFT
    ops = a.args if a.stdout else a.args[1:]
    if len(ops) != 2 or (not a.stdout and len(a.args) != 3):
        return _fail("expected " + ("" if a.stdout else "HASHFILE ") + "LEFT RIGHT")
    left, right = ops
    try:
        for d in ops:
            if not os.path.isfile(d) or not os.access(d, os.R_OK):
                return _fail(f"dictionary {d}: cannot be opened")
        if a.stdout:
            out = sys.stdout.buffer
            if side == L.DWPA_COMBI_AMP_RIGHT:
                amp = list(_words(right))
                for w in _words(left):
                    out.write(b"".join(w + r + b"\n" for r in amp))
            else:
                amp = list(_words(left))
                for w in _words(right):
                    out.write(b"".join(l + w + b"\n" for l in amp))
            out.flush()
            return 0
        devices = _devices(a)
        if devices < 0:
            return 255
        rc, status = M.crack_combinator(a.args[0], left, right, side, a.nonce_error_corrections, a.outfile,
                                        device_mask=devices, batch=a.batch)
    except (L.DwpaError, OSError) as e:
        return _fail(str(e))
    if rc in (0, 1):
        st = M.crack_stats()
        print("dwpa_amd.mask: %s, %d/%d hashlines cracked, %d words, %d candidates in %.1f s" %
              ("cracked" if rc == 0 else "exhausted", st["cracked"], st["hashes"], st["words"], st["candidates"],
               st["seconds"]), file=sys.stderr)
        return rc
    return _fail("crack_combinator failed")


def _prefix(mask: bytes, n: int) -> bytes:
    """The mask text of the first n positions."""
    i = 0
    for _ in range(n):
        i += 2 if mask[i:i + 1] == b"?" else 1
    return mask[:i]


if __name__ == "__main__":
    sys.exit(main())
