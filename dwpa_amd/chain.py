"""``python -m dwpa_amd.chain HASHFILE PART [PART ...]`` -- the chain attack on libdwpa22000.so: up to four word lists
and masks joined left to right on the GPU.

Each PART is ``list:PATH`` (a plain or gzip wordlist, ``$HEX[]`` words decoded) or ``mask:MASK`` (hashcat's mask
language, ``?1``..``?4`` shared by all mask parts).  A candidate is one choice of every part, concatenated in the
order of the parts; candidate ``i`` is the ``i``-th element of ``itertools.product`` over the parts (the last part
runs fastest), and ``-s`` / ``-l`` name a window of those indices.  Candidates with a list word above 63 bytes or a
total length outside 8..63 are dropped on the GPU.

A ``list:`` part may be followed by one modifier, which binds to that part and does not count towards the four:
``rules:FILE`` (a hashcat rules file) or ``rule:TEXT`` (one inline rule, the chain's counterpart of ``-j`` / ``-k``;
it loads as a rules file of one line).  The part's choices are then its (rule, word) pairs, rule-major with the word
fastest -- choice = rule * words + word -- and its piece is the rule applied to the word; a choice the rule engine
rejects (an empty word, one above 256 bytes, a reject function) gives no candidate, and the 63-byte limit applies to
the rule's result.  Rules load as ``-r`` files do everywhere in this package: hashcat's loader, which skips lines that
use reject or memory functions, unless ``DWPA_RULE_MODE=full``; lines that do not parse are skipped with a message, and
a modifier with no valid rule is an error.

The options are spelled as ``python -m dwpa_amd.mask`` spells them: ``-1``..``-4``, ``--hex-charset``, ``-s/--skip``,
``-l/--limit``, ``-d`` (devices, numbered from 1), ``-o``, ``--nonce-error-corrections``, ``--batch``.  The exit status
is the call's return code (0 every hashline cracked, 1 exhausted, 255 error).  ``--keyspace`` and ``--stdout`` take no
hash file and stay on the host; ``--stdout`` prints every candidate of the window, unfiltered, in id order, and omits
the choices a ruled part rejects, as ``hashcat --stdout -r`` does.

Every list is held whole in device memory; rules on mask parts and ``--increment`` are not available.
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile

from . import _lib as L
from . import m22000 as M
from .mask import _custom_sets, _devices, _words


def _parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="python -m dwpa_amd.chain", description=__doc__.split("\n\n")[0],
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("args", nargs="*", metavar="[HASHFILE] PART",
                   help="an m22000 hash file and 1..4 parts, each list:PATH or mask:MASK, a list optionally followed "
                        "by rules:FILE or rule:TEXT; the parts alone with --keyspace / --stdout")
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


def _rule_lines(text: bytes, source: str, quiet: bool):
    """The rules of a modifier as the crack call's loader keeps them (the process's rule mode), one line each.  quiet:
    no message per skipped line (the crack call prints its own)."""
    full = os.environ.get("DWPA_RULE_MODE") == "full"
    kept = []
    for n, line in enumerate(text.split(b"\n"), 1):
        line = line.rstrip(b"\r")
        c = M.rules_count_ex(line)
        if not c["present"]:
            continue
        if c["parsed"] and (full or c["loaded_hashcat"]):
            kept.append(line)
        elif not quiet:
            print("dwpa_amd.chain: skipping invalid or unsupported rule in %s on line %d: %s" %
                  (source, n, line.decode(errors="replace")), file=sys.stderr)
    return kept


def _parts(ops, quiet=False):
    """([(kind, text)] of the PART operands, [None or (source, rule lines) per part]), or the exit status after a
    message.  A rules:FILE / rule:TEXT operand binds to the list: part just before it."""
    parts, rules = [], []
    for op in ops:
        if op.startswith("rules:") or op.startswith("rule:"):
            if not parts:
                return _fail(f"{op}: a rules modifier follows the list: part it applies to")
            if parts[-1][0] != L.DWPA_CHAIN_LIST:
                return _fail(f"{op}: rules go with a list: part, not with a mask")
            if rules[-1] is not None:
                return _fail(f"{op}: the part has a rules modifier already")
            if op.startswith("rules:"):
                path = op[6:]
                if not os.path.isfile(path) or not os.access(path, os.R_OK):
                    return _fail(f"rules {path}: cannot be opened")
                with open(path, "rb") as f:
                    lines = _rule_lines(f.read(), path, quiet)
                rules[-1] = (path, lines)
            else:
                lines = _rule_lines(os.fsencode(op[5:]), op, quiet)
                rules[-1] = (None, lines)
            if not lines:
                return _fail(f"{op}: no valid rules left")
            continue
        rules.append(None)
        if op.startswith("list:"):
            path = op[5:]
            if not os.path.isfile(path) or not os.access(path, os.R_OK):
                return _fail(f"list {path}: cannot be opened")
            parts.append((L.DWPA_CHAIN_LIST, path))
        elif op.startswith("mask:"):
            parts.append((L.DWPA_CHAIN_MASK, os.fsencode(op[5:])))
        else:
            return _fail(f"part {op}: expected list:PATH or mask:MASK")
    if not 1 <= len(parts) <= L.DWPA_CHAIN_MAX_PARTS:
        return _fail("expected 1..%d parts, each list:PATH or mask:MASK" % L.DWPA_CHAIN_MAX_PARTS)
    return parts, rules


def _ruled(words, lines):
    """Choice d of a ruled list, rule-major: rule d // len(words) on word d % len(words); None when rejected."""
    text = b"\n".join(lines)
    return lambda d: M.rules_apply_host(text, d // len(words), words[d % len(words)])


def _candidates(choices, radices, first: int, count: int):
    """Candidates first .. first + count - 1: an odometer over the parts, started at chain_split's digits.
    choices[p](d) gives part p's bytes at digit d."""
    digits = M.chain_split(radices, first)
    cur = [c(d) for c, d in zip(choices, digits)]
    for n in range(count):
        if None not in cur:  # a ruled part rejected its choice: no candidate
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
    parts = _parts(a.args if host_only else a.args[1:], quiet=not host_only)
    if isinstance(parts, int):
        return parts
    parts, rules = parts
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
            radices = [M.mask_keyspace(text, custom) if ws is None else len(ws) * (len(r[1]) if r else 1)
                       for (kind, text), ws, r in zip(parts, lists, rules)]
            for ws, n, r in zip(lists, radices, rules):
                if r and n >= 2**32:
                    return _fail("%d words x %d rules is 2^32 choices or more" % (len(ws), len(r[1])))
            keyspace = M.chain_keyspace(radices)
            if a.keyspace:
                print(keyspace)
                return 0
            if keyspace and a.skip >= keyspace:
                return _fail("--skip is not below the keyspace")
            count = max(0, keyspace - a.skip)
            if a.limit:
                count = min(count, a.limit)
            choices = [(lambda d, m=text: M.mask_candidate(m, d, custom)) if ws is None else
                       _ruled(ws, r[1]) if r else ws.__getitem__ for (kind, text), ws, r in zip(parts, lists, rules)]
            out = sys.stdout.buffer
            if count:
                for c in _candidates(choices, radices, a.skip, count):
                    out.write(c + b"\n")
            out.flush()
            return 0
        devices = _devices(a)
        if devices < 0:
            return 255
        with tempfile.TemporaryDirectory() as tmp:  # an inline rule goes to the library as a one-line rules file
            files = None
            if any(rules):
                files = []
                for k, r in enumerate(rules):
                    if r and r[0] is None:
                        path = os.path.join(tmp, "rule%d.rule" % k)
                        with open(path, "wb") as f:
                            f.write(r[1][0] + b"\n")
                        files.append(path)
                    else:
                        files.append(r[0] if r else None)
            rc, status = M.crack_chain(a.args[0], parts, custom, a.skip, a.limit, a.nonce_error_corrections, a.outfile,
                                       device_mask=devices, batch=a.batch, rules=files)
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
