"""``python -m dwpa_amd.markov`` -- the Markov model of the mask attack (``python -m dwpa_amd.mask --markov FILE -t N``).

``train OUT.dwmk DICT [DICT ...]`` counts, per position 0..62 and per byte before it, the bytes of the words of the
lists (plain or gzip, read as every attack reads them; several lists count as their concatenation) and writes their
ranking to OUT.dwmk.  ``show FILE [-p POS] [-a BYTE]`` prints one row of a model: the 256 bytes that may follow BYTE
(decimal or 0x.., default 0: the start of a word) at position POS (default 0), most likely first.  Neither needs a
device.  The exit status is 0, or 255 after a message.
"""
from __future__ import annotations

import argparse
import sys

from . import _lib as L
from . import m22000 as M


def _fail(msg: str) -> int:
    print("dwpa_amd.markov: " + msg, file=sys.stderr)
    return 255


def row(model: bytes, pos: int, prev: int) -> bytes:
    """order[pos][prev] of a model image."""
    at = 16 + (pos * 256 + prev) * 256
    return model[at:at + 256]


def main(argv=None) -> int:
    p = argparse.ArgumentParser(prog="python -m dwpa_amd.markov", description=__doc__.split("\n\n")[0],
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = p.add_subparsers(dest="cmd")
    t = sub.add_parser("train", help="train a model from word lists")
    t.add_argument("out", metavar="OUT.dwmk")
    t.add_argument("dicts", nargs="+", metavar="DICT")
    s = sub.add_parser("show", help="print one row of a model")
    s.add_argument("file", metavar="FILE")
    s.add_argument("-p", "--position", type=int, default=0, metavar="POS")
    s.add_argument("-a", "--after", default="0", metavar="BYTE")
    try:
        a = p.parse_args(argv)
    except SystemExit as e:  # argparse: 0 after --help, 2 for bad arguments
        return 0 if e.code in (0, None) else 255
    try:
        if a.cmd == "train":
            words = M.markov_train(a.dicts, a.out)
            print("dwpa_amd.markov: %d words -> %s" % (words, a.out), file=sys.stderr)
            return 0
        if a.cmd == "show":
            try:
                prev = int(a.after, 0)
            except ValueError:
                return _fail("-a takes a byte value, decimal or 0x..")
            if not 0 <= a.position <= 62 or not 0 <= prev <= 255:
                return _fail("-p takes 0..62, -a takes 0..255")
            r = row(M.markov_load(a.file), a.position, prev)
            print(" ".join("%02x" % b for b in r))
            return 0
    except L.DwpaError as e:
        return _fail(str(e))
    return _fail("expected train or show")


if __name__ == "__main__":
    sys.exit(main())
