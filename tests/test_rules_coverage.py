"""CPU: every operation of the reference's rule file (help_crack/bestWPA.rule, what `hashcat --stdout -r
bestWPA.rule` expands at help_crack.py:508-509,575-576) is handled, checked from the repository alone.

The file itself stays in the reference and is not read here.  What the project records about it is the list of the
16 operations it uses (dwpa_amd/rulesets.py): `: r u l c T $ ^ ] [ s D ' d p f`.  Two facts are
pinned:

* every rule of `dwpa_amd.rulesets.wpa_rules()`, the rule set composed from those operations that the GPU rule tests
  (tests/test_gpu_parity.py, tests/test_gpu_baseline_sizes.py) run against the oracle, parses through the library's
  host rule parser (`dwpa_rules_expand` with out == NULL only parses, no device is touched) and through the rule
  oracle (oracle/rules.py), all together and each one on its own;
* the operations that rule set uses are exactly the 16 the file uses -- so the GPU rule engine is exercised on every
  operation bestWPA.rule can ask of it.
"""
import ctypes

from dwpa_amd import _lib as L
from dwpa_amd.rulesets import wpa_rules
from oracle import rules as R

BEST_WPA_OPS = ":rulcT$^][sD'dpf"


def _nrules_host(text: str) -> int:
    raw = text.encode("latin-1")
    n = ctypes.c_uint32(0)
    rc = L.load().dwpa_rules_expand(0, raw, len(raw), None, 0, None, None, ctypes.byref(n))
    assert rc == 0
    return n.value


def test_best_wpa_all_rules_parse_host_and_oracle():
    lines = wpa_rules()
    assert len(lines) == 148
    assert _nrules_host("\n".join(lines) + "\n") == len(lines)
    # rule by rule: each one parses on its own (none is silently merged or dropped)
    assert all(_nrules_host(l) == 1 for l in lines)
    assert all(R.parse(l) for l in lines)


def test_best_wpa_ops_covered_by_tested_rule_set():
    tested_ops = {op for l in wpa_rules() for op in R.parse(l)}
    # the op kinds the survey lists for the file, every one of them in the tested set
    assert len(BEST_WPA_OPS) == 16
    assert {op for op, *_ in tested_ops} == set(BEST_WPA_OPS)
