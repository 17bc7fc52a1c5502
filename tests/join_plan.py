"""The joins and length filters of the hybrid and combinator attacks, restated in Python (CPU, no library call).
tests/test_gpu_hybrid.py and tests/test_gpu_combinator.py plant with them, tests/prepared_plan.py models with them."""
COMBI_AMP_RIGHT, COMBI_AMP_LEFT = 0, 1  # include/dwpa22000.h DWPA_COMBI_AMP_*


def hybrid_join(word, m, mode):
    """Mode 6 (hashcat -a 6): word + mask candidate; mode 7: mask candidate + word."""
    return word + m if mode == 6 else m + word


def hybrid_keeps(word, npos, minlen=8, maxlen=63):
    """The hybrid filter: the word at most 63 bytes and the joined length inside minlen..maxlen."""
    return len(word) <= 63 and minlen <= len(word) + npos <= maxlen


def kept_words(words, npos, minlen=8, maxlen=63):
    return [i for i, w in enumerate(words) if hybrid_keeps(w, npos, minlen, maxlen)]


def combi_join(base, amp, side):
    return base + amp if side == COMBI_AMP_RIGHT else amp + base


def keeps(a, b, minlen=8, maxlen=63):
    """The combinator filter: both words at most 63 bytes and the joined length inside minlen..maxlen."""
    return len(a) <= 63 and len(b) <= 63 and minlen <= len(a) + len(b) <= maxlen
