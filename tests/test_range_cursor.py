"""CPU: the shared cursor of the range attacks (dwpa_crack_mask, dwpa_crack_chain; dwpa_amd/csrc/crack_cursor.hpp)
through its stand-alone host check under ThreadSanitizer."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_range_cursor_under_tsan():
    """tools/range_cursor_check.cpp: with cap = 4, the segment lists {}, {[0,6) [7,7) [3,12)}, {[5,6)}, {[0,13)} and
    {[2^64-11, 2^64-1)} drained by 1 and by 8 threads.  The binary exits 1 unless the taken ranges tile the segments
    exactly, every count is 1..cap, no range crosses a segment, one thread sees them in order, and eight take() calls
    after the end all return false; a data race makes ThreadSanitizer fail it.  26 ranges: (0 + 5 + 1 + 4 + 3) x 2."""
    subprocess.run(["make", "-s", "-C", ROOT, "tools/bin/range_cursor_check"], check=True)
    r = subprocess.run([os.path.join(ROOT, "tools", "bin", "range_cursor_check")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert json.loads(r.stdout) == {"cases": 5, "ranges": 26}
