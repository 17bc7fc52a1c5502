"""Python host side of libdwpa22000.so, mirroring dwpa's own interfaces for the m22000 path.

``check_key_m22000`` keeps the exact call signature and return shape of the PHP function it replaces
(web/common.php:157-307): ``False`` or ``[PSK, NC, endian, PMK]`` with ``NC``/``endian`` ``None`` for PMKID
lines, ``endian`` in ``{None, 'BE', 'LE'}``, ``PSK`` after ``$HEX[]`` decoding and ``PMK`` as 32 raw bytes.
The arithmetic runs in libdwpa22000.so: on the GPU, or on the library's host backend for small calls and (only when
asked for, ``init(allow_cpu_fallback=1)``) without a device; otherwise a call without a device raises ``DwpaError``.
"""
from __future__ import annotations

import ctypes
import os

from . import _lib as L

_ENDIAN = {0: None, 1: "BE", 2: "LE"}


def _b(x) -> bytes:
    if isinstance(x, str):
        return x.encode("utf-8", "surrogateescape")
    return bytes(x)


def device_count() -> int:
    return L.check(L.load().dwpa_device_count(), "device_count")


def init(device_mask: int = 0, batch: int = 0, rule_mode: int = L.DWPA_RULES_DEFAULT, allow_cpu_fallback: int = 0,
         host_max_pmks: int = 0) -> int:
    """dwpa_init: the process's device selection, check batch, rule-file mode and host backend switches
    (allow_cpu_fallback 1/-1/0 = on/off/DWPA_CPU_FALLBACK; host_max_pmks n/-1/0 = small-call threshold/never/
    DWPA_HOST_MAX_PMKS or the PMKs the host pool derives in 2 ms).  Returns 0 or raises (DWPA_E_NODEV without a device unless the
    fallback is on)."""
    cfg = L.Config(ctypes.sizeof(L.Config), int(device_mask), int(batch), 0, int(rule_mode), int(allow_cpu_fallback),
                   int(host_max_pmks))
    return L.check(L.load().dwpa_init(ctypes.byref(cfg)), "init")


def hc_unhex(key) -> bytes:
    """common.php:3-25 ($HEX[...] decoding), executed by the library's host code."""
    k = _b(key)
    out = ctypes.create_string_buffer(max(1, len(k)))
    n = ctypes.c_size_t(0)
    L.check(L.load().dwpa_hc_unhex(k, len(k), out, ctypes.byref(n)), "hc_unhex")
    return out.raw[:n.value]


def hash_m22000(hashline):
    """common.php:310-315: raw md5 over fields 1..7, or False."""
    h = _b(hashline)
    out = ctypes.create_string_buffer(16)
    if L.load().dwpa_hash_m22000(h, len(h), out) < 0:
        return False
    return out.raw


def parse_m22000(hashline, nc: int = 128, nc_mode: int = L.DWPA_NC_PHP):
    """Host-side parse (common.php:157-237 acceptance rules): dict of fields, or the negative parse code."""
    h = _b(hashline)
    info = L.LineInfo()
    rc = L.load().dwpa_parse_m22000(h, len(h), int(nc), int(nc_mode), ctypes.byref(info))
    if rc < 0:
        return rc
    return {"type": info.type, "keyver": info.keyver, "essid": bytes(info.essid[:min(32, info.essid_len)]),
            "essid_len": info.essid_len, "mac_ap": bytes(info.mac_ap[:min(16, info.mac_ap_len)]),
            "mac_sta": bytes(info.mac_sta[:min(16, info.mac_sta_len)]), "target_len": info.target_len,
            "attempts": info.attempts, "lists": info.lists, "never_matches": bool(info.never_matches),
            "hash_m22000": bytes(info.hash_m22000)}


def group_by_essid(hashlines):
    """Per-ESSID grouping of a work unit (get_work hands out one ESSID, web/content/get_work.php:96-109);
    duplicate lines (same hash_m22000 key, common.php:310-315) are dropped.  Returns {essid: [lines]}."""
    groups, seen = {}, set()
    for line in hashlines:
        p = parse_m22000(line)
        if isinstance(p, int) or p["hash_m22000"] in seen:
            continue
        seen.add(p["hash_m22000"])
        groups.setdefault(p["essid"] if p["essid_len"] <= 32 else _b(line).split(b"*")[5], []).append(_b(line))
    return groups


def _result(keys, r: L.Result):
    key = keys[r.key_index]
    key = _b(key)
    if key.startswith(b"$HEX["):
        key = hc_unhex(key)
    pmk = bytes(r.pmk)
    if not r.nc_valid:
        return [key, None, None, pmk]
    return [key, int(r.nc), _ENDIAN[int(r.endian)], pmk]


def _nc(nc) -> int:
    """The ABI's nc is an int32: a value outside it would be wrapped by ctypes into a different window."""
    v = int(nc)
    if not -2**31 <= v < 2**31:
        raise L.DwpaError(L.DWPA_E_ARG, f"nc {v} is outside int32")
    return v


def check_key_m22000(hashline, keys, pmk=False, nc: int = 128):
    """Drop-in for PHP check_key_m22000($hashline, $keys, $pmk=False, $nc=128)."""
    h = _b(hashline)
    keys = list(keys)
    arr, keep = L.bytes_array([None if k is None else _b(k) for k in keys])
    res = L.Result()
    pm = bytes(pmk) if pmk else None  # PHP: `if (!$pmk)` -- False/''/None all mean "derive"
    if pm is not None and len(pm) != 32:
        raise ValueError("pmk must be 32 bytes")
    rc = L.check(L.load().dwpa_check_m22000(h, len(h), arr, len(keys), pm, _nc(nc), ctypes.byref(res)),
                 "check_m22000")
    if rc != L.DWPA_HIT:
        return False
    return _result(keys, res)


class BatchJobs:
    """A dwpa_check_batch argument block built once (ctypes job/key arrays) and run any number of times."""

    def __init__(self, jobs):
        jobs = list(jobs)
        self.n = n = len(jobs)
        self.carr = (L.Job * max(1, n))()
        self._keep = []
        self.key_lists = []
        for i, (line, keys, pmk, nc) in enumerate(jobs):
            h = _b(line)
            keys = list(keys)
            arr, k = L.bytes_array([None if x is None else _b(x) for x in keys])
            pm = bytes(pmk) if pmk else None
            self._keep += [h, arr, k, pm]
            self.key_lists.append(keys)
            c = self.carr[i]
            c.line, c.line_len = h, len(h)
            c.keys, c.nkeys = ctypes.cast(arr, ctypes.POINTER(L.Bytes)), len(keys)
            c.pmk, c.nc = pm, _nc(nc)
        self.nkeys = sum(len(k) for k in self.key_lists)
        self.out = (L.Result * max(1, n))()
        self.rcs = (ctypes.c_int * max(1, n))()

    def run(self) -> None:
        L.check(L.load().dwpa_check_batch(self.carr, self.n, self.out, self.rcs), "check_batch")

    def results(self) -> list:
        res = []
        for i in range(self.n):
            if self.rcs[i] == L.DWPA_HIT:
                res.append(_result(self.key_lists[i], self.out[i]))
            else:
                L.check(self.rcs[i], "check_batch job")
                res.append(False)
        return res


def check_stats():
    """dwpa_check_last_stats: {jobs, slots, pmks, tail_pmks, tail_waves, tail_waves_raised, hits, backend, seconds}
    of this thread's last check call (backend: DWPA_BACKEND_DEVICE / _HOST_SMALL / _HOST_FALLBACK)."""
    st = L.CheckStats()
    L.check(L.load().dwpa_check_last_stats(ctypes.byref(st)), "check_last_stats")
    return {k: getattr(st, k) for k, _ in L.CheckStats._fields_ if k != "reserved"}


def resource_stats():
    """dwpa_resource_stats: {device_bytes, pinned_host_bytes, host_pool_threads, devices, call_contexts,
    call_contexts_used} this process's library holds now (host only)."""
    st = L.Resources()
    L.check(L.load().dwpa_resource_stats(ctypes.byref(st)), "resource_stats")
    return {k: getattr(st, k) for k, _ in L.Resources._fields_}


def check_batch(jobs):
    """jobs: iterable of (hashline, keys, pmk_or_False, nc).  Returns a list of check_key_m22000 results."""
    b = BatchJobs(jobs)
    b.run()
    return b.results()


def pbkdf2_pmk(keys, essid) -> list:
    """PMK = PBKDF2-HMAC-SHA1(key, essid, 4096, 32) for every key (raw bytes): on the GPU, or on the host backend for
    at most host_max_pmks keys."""
    keys = [_b(k) for k in keys]
    e = _b(essid)
    arr, keep = L.bytes_array(keys)
    out = ctypes.create_string_buffer(32 * max(1, len(keys)))
    L.check(L.load().dwpa_pbkdf2_pmk(arr, len(keys), e, len(e), out), "pbkdf2_pmk")
    raw = out.raw
    return [raw[32 * i:32 * i + 32] for i in range(len(keys))]


def rules_count(rules_text):
    """(rule lines present, rules that parse, 1-based line of the first that does not or 0) -- host only."""
    rt = _b(rules_text)
    present, parsed, first = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
    L.check(L.load().dwpa_rules_count(rt, len(rt), ctypes.byref(present), ctypes.byref(parsed), ctypes.byref(first)),
            "rules_count")
    return present.value, parsed.value, first.value


def rules_count_ex(rules_text) -> dict:
    """Both loaders' counts (host only): {present, parsed (DWPA_RULES_FULL loads these), loaded_hashcat (hashcat's
    -r loader keeps these), rejmem, invalid, first_invalid_line, first_rejmem_line}."""
    rt = _b(rules_text)
    c = L.RulesCounts()
    L.check(L.load().dwpa_rules_count_ex(rt, len(rt), ctypes.byref(c)), "rules_count_ex")
    return {k: getattr(c, k) for k, _ in L.RulesCounts._fields_ if k != "reserved"}


def rules_apply_host(rules_text, rule_index: int, word):
    """Rule `rule_index` of rules_text applied to `word` on the host by the GPU's interpreter: bytes or None."""
    rt, w = _b(rules_text), _b(word)
    out = ctypes.create_string_buffer(256)
    n = ctypes.c_uint32(0)
    L.check(L.load().dwpa_rules_apply_host(rt, len(rt), int(rule_index), w, len(w), out, ctypes.byref(n)),
            "rules_apply_host")
    return None if n.value == 0xFFFFFFFF else out.raw[:n.value]


def rules_expand_file(rules_file, sources, out_path, gzip_level: int = 0, device: int = 0):
    """`hashcat --stdout -r rules_file sources -o out_path` on the GPU: returns (words read, candidates written)."""
    src = [_b(x) for x in sources]
    arr = (ctypes.c_char_p * max(1, len(src)))(*src)
    w, c = ctypes.c_uint64(0), ctypes.c_uint64(0)
    L.check(L.load().dwpa_rules_expand_file(device, _b(rules_file), arr, len(src), _b(out_path), int(gzip_level),
                                            ctypes.byref(w), ctypes.byref(c)), "rules_expand_file")
    return w.value, c.value


def rules_expand(rules_text, words, device: int = 0):
    """GPU rule application (hashcat --stdout -r): returns [[candidate or None (rejected)] per rule] per word."""
    rt = _b(rules_text)
    words = [_b(w) for w in words]
    nr = ctypes.c_uint32(0)
    lib = L.load()
    L.check(lib.dwpa_rules_expand(device, rt, len(rt), None, 0, None, None, ctypes.byref(nr)), "rules_expand")
    nrules = nr.value
    if not words or not nrules:
        return [[] for _ in words]
    arr, keep = L.bytes_array(words)
    out = ctypes.create_string_buffer(len(words) * nrules * 256)
    lens = (ctypes.c_uint32 * (len(words) * nrules))()
    L.check(lib.dwpa_rules_expand(device, rt, len(rt), arr, len(words), out, lens, ctypes.byref(nr)), "rules_expand")
    raw = out.raw
    res = []
    for i in range(len(words)):
        row = []
        for r in range(nrules):
            c = i * nrules + r
            n = lens[c]
            row.append(None if n == 0xFFFFFFFF else raw[c * 256:c * 256 + n])
        res.append(row)
    return res


def crack_files(hash_file, dicts, rules_file=None, nonce_error_corrections: int = 8, out_file="help_crack.key",
                device_mask: int = 0, batch: int = 0, nc_mode: int = L.DWPA_NC_HASHCAT,
                rule_mode: int = L.DWPA_RULES_DEFAULT) -> int:
    """In-process hashcat -m22000 replacement; returns a hashcat exit code (0 cracked, 1 exhausted, -1 error).
    rule_mode: DWPA_RULES_DEFAULT (the process's: hashcat's -r loader unless DWPA_RULE_MODE=full), _HASHCAT or _FULL
    (reject / memory lines run too)."""
    return crack_files_ex(hash_file, dicts, rules_file, nonce_error_corrections, out_file, device_mask, batch,
                          nc_mode, rule_mode)[0]


def crack_files_ex(hash_file, dicts, rules_file=None, nonce_error_corrections: int = 8, out_file="help_crack.key",
                   device_mask: int = 0, batch: int = 0, nc_mode: int = L.DWPA_NC_HASHCAT,
                   rule_mode: int = L.DWPA_RULES_DEFAULT):
    """crack_files plus one status per dictionary: (rc, [DWPA_DICT_OK | DWPA_DICT_DAMAGED | DWPA_E_IO])."""
    cfg = L.Config(ctypes.sizeof(L.Config), device_mask, batch, nc_mode, rule_mode)
    dl = [_b(d) for d in dicts]
    darr = (ctypes.c_char_p * max(1, len(dl)))(*dl)
    st = (ctypes.c_int32 * max(1, len(dl)))()
    rc = L.load().dwpa_crack_files_ex(_b(hash_file), darr, len(dl), _b(rules_file) if rules_file else None,
                                      _nc(nonce_error_corrections), _b(out_file), ctypes.byref(cfg), st)
    return rc, [int(st[i]) for i in range(len(dl))]


def _custom(custom):
    """custom sets ?1..?4 (bytes/str, None = undefined) -> (ctypes array of 4 Bytes, keep-alive)."""
    custom = list(custom)
    if len(custom) > 4:
        raise L.DwpaError(L.DWPA_E_ARG, "at most four custom sets (?1..?4)")
    return L.bytes_array([None if c is None else _b(c) for c in custom] + [None] * (4 - len(custom)))


def _u64(v, what) -> int:
    v = int(v)
    if not 0 <= v < 2**64:
        raise L.DwpaError(L.DWPA_E_ARG, f"{what} {v} is outside uint64")
    return v


def markov_train(dicts, out_file) -> int:
    """Train a Markov model (include/dwpa22000.h "mask attack in Markov order") from word lists, plain or gzip, read
    as every attack reads them, and write it to out_file; returns the number of words that contributed.  Raises
    DwpaError(DWPA_E_IO) for an unreadable list or a damaged gzip stream (no file is written then)."""
    paths = [_b(d) for d in ([dicts] if isinstance(dicts, (str, bytes, os.PathLike)) else dicts)]
    arr = (ctypes.c_char_p * max(1, len(paths)))(*paths)
    words = ctypes.c_uint64(0)
    L.check(L.load().dwpa_markov_train(arr, len(paths), _b(out_file), ctypes.byref(words)), "markov_train")
    return words.value


def markov_load(path) -> bytes:
    """The Markov model file at `path` as a validated image (DWPA_MARKOV_BYTES bytes).  Raises DwpaError: DWPA_E_IO
    unreadable, DWPA_E_ARG another size, another header or a row that is no permutation of 0..255."""
    out = ctypes.create_string_buffer(L.DWPA_MARKOV_BYTES)
    L.check(L.load().dwpa_markov_load(_b(path), out, L.DWPA_MARKOV_BYTES), "markov_load")
    return out.raw


def _threshold(threshold) -> int:
    t = int(threshold)
    if not 0 <= t <= 256:
        raise L.DwpaError(L.DWPA_E_ARG, f"threshold {t}: 0 (none) or 1..256")
    return t


def _model(markov, threshold) -> bytes:
    if markov is None:
        raise L.DwpaError(L.DWPA_E_ARG, f"threshold {threshold} needs a Markov model (markov_train / markov_load): "
                                        "there are no built-in statistics")
    return bytes(markov)


def mask_keyspace(mask, custom=(), threshold: int = 0) -> int:
    """Keyspace of a hashcat -a 3 mask (host only): the product of its positions' set sizes.  custom: the sets
    ?1..?4 as raw bytes in the mask language.  threshold (hashcat -t, 1..256; 0 = none): every position cut down to
    that many bytes at most; needs no model.  Raises DwpaError(DWPA_E_ARG) for an invalid mask or K > 2**64 - 1."""
    m = _b(mask)
    arr, keep = _custom(custom)
    k = ctypes.c_uint64(0)
    if threshold:
        L.check(L.load().dwpa_mask_keyspace_markov(m, len(m), arr, _threshold(threshold), None, ctypes.byref(k)),
                "mask_keyspace_markov")
        return k.value
    L.check(L.load().dwpa_mask_keyspace(m, len(m), arr, None, ctypes.byref(k)), "mask_keyspace")
    return k.value


def mask_positions(mask, custom=(), threshold: int = 0) -> int:
    """Positions (candidate length) of a mask (host only); threshold as for mask_keyspace (a mask whose keyspace
    only fits under the threshold is valid only with it)."""
    m = _b(mask)
    arr, keep = _custom(custom)
    n = ctypes.c_uint32(0)
    if threshold:
        L.check(L.load().dwpa_mask_keyspace_markov(m, len(m), arr, _threshold(threshold), ctypes.byref(n), None),
                "mask_keyspace_markov")
        return n.value
    L.check(L.load().dwpa_mask_keyspace(m, len(m), arr, ctypes.byref(n), None), "mask_keyspace")
    return n.value


def mask_candidate(mask, index: int, custom=(), markov=None, threshold: int = 0) -> bytes:
    """Candidate `index` of a mask (host only), in the library's order: the mixed-radix numeral of the index with the
    last position fastest (itertools.product order; hashcat's own order differs, the candidate set does not).
    markov (a model image, markov_load) / threshold: the candidate of the Markov order instead, each digit choosing
    from the model's ranking after the byte before it; the image is validated on every call (mask_candidates takes
    many indices at once)."""
    if markov is not None or threshold:
        return mask_candidates(mask, [index], custom, markov, threshold)[0]
    m = _b(mask)
    arr, keep = _custom(custom)
    out = ctypes.create_string_buffer(64)
    n = ctypes.c_uint32(0)
    L.check(L.load().dwpa_mask_candidate(m, len(m), arr, _u64(index, "index"), out, ctypes.byref(n)), "mask_candidate")
    return out.raw[:n.value]


def mask_candidates(mask, indices, custom=(), markov=None, threshold: int = 0) -> list:
    """The Markov-order candidates (host only) of `indices` under a model image and a threshold, in one call."""
    m = _b(mask)
    arr, keep = _custom(custom)
    model = _model(markov, threshold)
    idx = [_u64(i, "index") for i in indices]
    ia = (ctypes.c_uint64 * max(1, len(idx)))(*idx)
    out = ctypes.create_string_buffer(64 * max(1, len(idx)))
    n = ctypes.c_uint32(0)
    L.check(L.load().dwpa_mask_candidates_markov(m, len(m), arr, model, len(model), _threshold(threshold), ia, len(idx),
                                                 out, ctypes.byref(n)), "mask_candidates_markov")
    return [out.raw[64 * k:64 * k + n.value] for k in range(len(idx))]


def crack_mask(hash_file, mask, custom=(), skip: int = 0, limit: int = 0, increment=None,
               nonce_error_corrections: int = 8, out_file="help_crack.key", device_mask: int = 0, batch: int = 0,
               nc_mode: int = L.DWPA_NC_HASHCAT, markov=None, threshold: int = 0) -> int:
    """In-process `hashcat -m22000 -a 3 hash_file mask`; returns a hashcat exit code (0 cracked, 1 exhausted,
    -1 error).  skip / limit: indices [skip, skip + limit) of the keyspace in the library's order (limit 0 = to the
    end).  increment: None = off, else (min, max) = the mask's prefixes of min..max positions, shortest first (not
    with skip / limit).  Runs on every selected device.  markov (the PATH of a model file, markov_train) / threshold
    (hashcat -t): the Markov order under that threshold instead; skip / limit then index the thresholded keyspace."""
    m = _b(mask)
    if b"\0" in m:
        raise L.DwpaError(L.DWPA_E_ARG, "crack_mask takes a NUL-terminated mask: put a NUL byte into a custom set")
    arr, keep = _custom(custom)
    imin, imax = (0, 0) if increment is None else (int(increment[0]), int(increment[1]))
    if increment is not None and not (imin or imax):
        imin = 1  # (0, 0) would mean "off" in the C call
    cfg = L.Config(ctypes.sizeof(L.Config), device_mask, batch, nc_mode)
    if markov is not None or threshold:
        if markov is None:
            _model(markov, threshold)
        return L.load().dwpa_crack_mask_markov(_b(hash_file), m, arr, _b(markov), _threshold(threshold),
                                               _u64(skip, "skip"), _u64(limit, "limit"), imin, imax,
                                               _nc(nonce_error_corrections), _b(out_file), ctypes.byref(cfg))
    return L.load().dwpa_crack_mask(_b(hash_file), m, arr, _u64(skip, "skip"), _u64(limit, "limit"), imin, imax,
                                    _nc(nonce_error_corrections), _b(out_file), ctypes.byref(cfg))


def crack_hybrid(hash_file, dicts, mask, custom=(), mode: int = L.DWPA_HYBRID_WORD_MASK,
                 nonce_error_corrections: int = 8, out_file="help_crack.key", device_mask: int = 0, batch: int = 0,
                 nc_mode: int = L.DWPA_NC_HASHCAT):
    """In-process `hashcat -m22000 -a 6 hash_file dicts... mask` (mode 6: word + mask candidate) or `-a 7 hash_file
    mask dicts...` (mode 7: mask candidate + word) over plain or gzip dictionaries, on every selected device.
    Returns (rc, dict_status): a hashcat exit code (0 cracked, 1 exhausted, -1 error) and one status per dictionary
    (DWPA_DICT_OK | DWPA_DICT_DAMAGED | DWPA_E_IO)."""
    m = _b(mask)
    if b"\0" in m:
        raise L.DwpaError(L.DWPA_E_ARG, "crack_hybrid takes a NUL-terminated mask: put a NUL byte into a custom set")
    arr, keep = _custom(custom)
    cfg = L.Config(ctypes.sizeof(L.Config), device_mask, batch, nc_mode)
    dl = [_b(d) for d in dicts]
    darr = (ctypes.c_char_p * max(1, len(dl)))(*dl)
    st = (ctypes.c_int32 * max(1, len(dl)))()
    rc = L.load().dwpa_crack_hybrid(_b(hash_file), darr, len(dl), m, arr, int(mode), _nc(nonce_error_corrections),
                                    _b(out_file), ctypes.byref(cfg), st)
    return rc, [int(st[i]) for i in range(len(dl))]


def crack_combinator(hash_file, left, right, amp_side: int = L.DWPA_COMBI_AMP_RIGHT,
                     nonce_error_corrections: int = 8, out_file="help_crack.key", device_mask: int = 0, batch: int = 0,
                     nc_mode: int = L.DWPA_NC_HASHCAT):
    """In-process `hashcat -m22000 -a 1 hash_file left right`: every word of `left` followed by every word of `right`
    (plain or gzip lists), on every selected device.  amp_side names the list held whole in device memory
    (DWPA_COMBI_AMP_RIGHT, the default, or DWPA_COMBI_AMP_LEFT); the other list is streamed.  Returns (rc,
    [left_status, right_status]): a hashcat exit code (0 cracked, 1 exhausted, -1 error) and one status per list
    (DWPA_DICT_OK | DWPA_DICT_DAMAGED | DWPA_E_IO)."""
    cfg = L.Config(ctypes.sizeof(L.Config), device_mask, batch, nc_mode)
    st = (ctypes.c_int32 * 2)()
    rc = L.load().dwpa_crack_combinator(_b(hash_file), _b(left), _b(right), int(amp_side),
                                        _nc(nonce_error_corrections), _b(out_file), ctypes.byref(cfg), st)
    return rc, [int(st[0]), int(st[1])]


def _radices(radices):
    r = [_u64(v, "radix") for v in radices]
    return (ctypes.c_uint64 * max(1, len(r)))(*r), len(r)


def chain_keyspace(radices) -> int:
    """Keyspace of a chain (host only): the product of its parts' radices -- a list's word count, a mask's keyspace.
    Raises DwpaError(DWPA_E_ARG) for no part, more than four, or a product above 2**64 - 1."""
    arr, n = _radices(radices)
    k = ctypes.c_uint64(0)
    L.check(L.load().dwpa_chain_keyspace(arr, n, ctypes.byref(k)), "chain_keyspace")
    return k.value


def chain_split(radices, index: int) -> list:
    """The digits of candidate `index` of a chain (host only), one per part, last part fastest: a list's word index,
    a mask part's own index.  Raises DwpaError(DWPA_E_ARG) as chain_keyspace does, and for index >= keyspace."""
    arr, n = _radices(radices)
    d = (ctypes.c_uint64 * max(1, n))()
    L.check(L.load().dwpa_chain_split(arr, n, _u64(index, "index"), d), "chain_split")
    return [int(d[i]) for i in range(n)]


def chain_candidate(parts, index: int, custom=(), rules=None):
    """Candidate `index` of a chain (host only).  parts: one entry per part, a sequence of words (bytes) for a list
    or ("mask", MASK) for a mask; the parts' choices at chain_split's digits, joined left to right.  Unfiltered.
    rules: one entry per part, None or the rule text of a list part (the whole language; lines that do not parse are
    skipped): that part's choices are then its (rule, word) pairs, rule-major -- digit = rule * len(words) + word --
    and its piece is the rule applied by the GPU's interpreter on the host (dwpa_rules_apply_host).  Returns None when
    a ruled part rejects its choice: an input word of 0 bytes or above 256, or a reject function."""
    parts = list(parts)
    rules = [None] * len(parts) if rules is None else list(rules)
    if len(rules) != len(parts):
        raise L.DwpaError(L.DWPA_E_ARG, "chain_candidate takes one rules entry per part")
    masks = [isinstance(p, tuple) and len(p) == 2 and p[0] == "mask" for p in parts]
    nrules = [None if r is None else rules_count(r)[1] for r in rules]
    for m, n in zip(masks, nrules):
        if n is not None and (m or n == 0):
            raise L.DwpaError(L.DWPA_E_ARG if m else L.DWPA_E_RULE, "rules go with a list part and need a valid rule")
    radices = [mask_keyspace(p[1], custom) if m else len(p) * (n or 1) for p, m, n in zip(parts, masks, nrules)]
    digits = chain_split(radices, index)
    out = []
    for p, m, d, r in zip(parts, masks, digits, rules):
        if m:
            piece = mask_candidate(p[1], d, custom)
        elif r is None:
            piece = _b(p[d])
        else:
            piece = rules_apply_host(r, d // len(p), p[d % len(p)])
            if piece is None:
                return None
        out.append(piece)
    return b"".join(out)


def crack_chain(hash_file, parts, custom=(), skip: int = 0, limit: int = 0, nonce_error_corrections: int = 8,
                out_file="help_crack.key", device_mask: int = 0, batch: int = 0, nc_mode: int = L.DWPA_NC_HASHCAT,
                rules=None, rule_mode: int = L.DWPA_RULES_DEFAULT):
    """The chain attack over hash_file, on every selected device.  parts: 1..4 entries (DWPA_CHAIN_LIST, path of a
    plain or gzip word list) or (DWPA_CHAIN_MASK, mask); a candidate is one choice of every part joined left to right,
    candidate id = its index in itertools.product order.  skip / limit: raw indices [skip, skip + limit) (limit 0 = to
    the end).  rules: None, or one entry per part, each None or the path of a rules file for that list part
    (dwpa_crack_chain_rules: the part's choices become its (rule, word) pairs, rule-major; the file loads under
    rule_mode as crack_files' does).  Returns (rc, part_status): a hashcat exit code (0 cracked, 1 exhausted, -1
    error) and one status per part (DWPA_DICT_OK | DWPA_DICT_DAMAGED | DWPA_E_IO)."""
    specs = [(int(k), _b(t)) for k, t in parts]
    for k, t in specs:
        if b"\0" in t:
            raise L.DwpaError(L.DWPA_E_ARG, "crack_chain takes NUL-terminated texts: put a NUL byte into a custom set")
    arr = (L.ChainSpec * max(1, len(specs)))(*[L.ChainSpec(k, t) for k, t in specs])
    carr, keep = _custom(custom)
    cfg = L.Config(ctypes.sizeof(L.Config), device_mask, batch, nc_mode, rule_mode)
    st = (ctypes.c_int32 * max(1, len(specs)))()
    if rules is None:
        rc = L.load().dwpa_crack_chain(_b(hash_file), arr, len(specs), carr, _u64(skip, "skip"), _u64(limit, "limit"),
                                       _nc(nonce_error_corrections), _b(out_file), ctypes.byref(cfg), st)
    else:
        rl = [None if r is None else _b(r) for r in rules]
        if len(rl) != len(specs):
            raise L.DwpaError(L.DWPA_E_ARG, "crack_chain takes one rules entry per part")
        rarr = (ctypes.c_char_p * max(1, len(rl)))(*rl)
        rc = L.load().dwpa_crack_chain_rules(_b(hash_file), arr, len(specs), rarr, carr, _u64(skip, "skip"),
                                             _u64(limit, "limit"), _nc(nonce_error_corrections), _b(out_file),
                                             ctypes.byref(cfg), st)
    return rc, [int(st[i]) for i in range(len(specs))]


def _word_array(words):
    """A sequence of words -> (ctypes array of Bytes, keep-alive): one buffer for all of them."""
    ws = [_b(w) for w in words]
    buf = ctypes.create_string_buffer(b"".join(ws), sum(len(w) for w in ws) + 1)
    base = ctypes.addressof(buf)
    arr = (L.Bytes * max(1, len(ws)))()
    pos = 0
    for i, w in enumerate(ws):
        arr[i].ptr, arr[i].len = base + pos, len(w)
        pos += len(w)
    return arr, len(ws), buf


def _u32(v, what) -> int:
    v = int(v)
    if not 0 <= v < 2**32:
        raise L.DwpaError(L.DWPA_E_ARG, f"{what} {v} is outside uint32")
    return v


def table_builtin(name="toggle") -> bytes:
    """The text of a built-in substitution table: "toggle" maps every ASCII letter to [itself, the other case]."""
    n = ctypes.c_size_t(0)
    L.check(L.load().dwpa_table_builtin(_b(name), None, 0, ctypes.byref(n)), "table_builtin")
    out = ctypes.create_string_buffer(n.value + 1)
    L.check(L.load().dwpa_table_builtin(_b(name), out, n.value, ctypes.byref(n)), "table_builtin")
    return out.raw[:n.value]


def table_parse(table) -> dict:
    """A table text (include/dwpa22000.h "table attack": K=V lines, each side one byte or \\xHH) as {byte: bytes of
    its alternatives in file order} for all 256 byte values (host only).  Raises DwpaError(DWPA_E_ARG) naming the
    line at fault (.line) for a line that is not K=V, a 17th alternative for one key, or a text with no mapping."""
    t = _b(table)
    img = ctypes.create_string_buffer(L.DWPA_TABLE_IMAGE_BYTES)
    bad = ctypes.c_uint32(0)
    rc = L.load().dwpa_table_parse(t, len(t), img, ctypes.byref(bad))
    if rc < 0:
        e = L.DwpaError(rc, f"table: line {bad.value} is not K=V, is a 17th alternative for its key, or the text holds "
                            "no mapping")
        e.line = bad.value
        raise e
    raw = img.raw
    return {c: raw[256 + 16 * c:256 + 16 * c + raw[c]] for c in range(256)}


def table_keyspace(table, words, minlen: int = 8, maxlen: int = 63, word_max: int = 0) -> dict:
    """The table attack's keyspace over a word list (host only): {keyspace, kept, dropped_len, dropped_max}.  A word is
    kept iff its length is in minlen..min(maxlen, 63) and the product of its bytes' alternative counts is at most
    word_max (0: 2**32 - 1).  Raises DwpaError(DWPA_E_ARG) for an invalid table or a keyspace above 2**64 - 1."""
    t = _b(table)
    arr, n, keep = _word_array(words)
    v = [ctypes.c_uint64(0) for _ in range(4)]
    L.check(L.load().dwpa_table_keyspace(t, len(t), arr, n, _u32(minlen, "minlen"), _u32(maxlen, "maxlen"),
                                         _u32(word_max, "word_max"), *[ctypes.byref(x) for x in v]), "table_keyspace")
    return dict(zip(("keyspace", "kept", "dropped_len", "dropped_max"), (x.value for x in v)))


def table_candidates(table, words, indices, minlen: int = 8, maxlen: int = 63, word_max: int = 0) -> list:
    """Candidates `indices` of the table attack over a word list (host only), in the library's order: kept words in
    list order, within a word itertools.product over its bytes' alternative lists (the last position fastest)."""
    t = _b(table)
    arr, n, keep = _word_array(words)
    idx = [_u64(i, "index") for i in indices]
    ia = (ctypes.c_uint64 * max(1, len(idx)))(*idx)
    out = ctypes.create_string_buffer(64 * max(1, len(idx)))
    ol = (ctypes.c_uint32 * max(1, len(idx)))()
    L.check(L.load().dwpa_table_candidates(t, len(t), arr, n, _u32(minlen, "minlen"), _u32(maxlen, "maxlen"),
                                           _u32(word_max, "word_max"), ia, len(idx), out, ol), "table_candidates")
    raw = out.raw
    return [raw[64 * k:64 * k + ol[k]] for k in range(len(idx))]


def crack_table(hash_file, dict_file, table_file, word_max: int = 0, skip: int = 0, limit: int = 0,
                nonce_error_corrections: int = 8, out_file="help_crack.key", device_mask: int = 0, batch: int = 0,
                nc_mode: int = L.DWPA_NC_HASHCAT) -> int:
    """The table attack over hash_file, on every selected device: every combination of the per-byte alternatives of
    table_file (K=V lines) for every word of dict_file (plain or gzip) of 8..63 bytes with at most word_max
    combinations (0: 2**32 - 1).  skip / limit: indices [skip, skip + limit) of the keyspace (limit 0 = to the end).
    Returns a hashcat exit code (0 cracked, 1 exhausted, -1 error)."""
    cfg = L.Config(ctypes.sizeof(L.Config), device_mask, batch, nc_mode)
    return L.load().dwpa_crack_table(_b(hash_file), _b(dict_file), _b(table_file), _u32(word_max, "word_max"),
                                     _u64(skip, "skip"), _u64(limit, "limit"), _nc(nonce_error_corrections),
                                     _b(out_file), ctypes.byref(cfg))


def _opt(path):
    return None if path is None else _b(path)


def _assoc_flags(single) -> int:
    return L.DWPA_ASSOC_SINGLE if single else 0


def assoc_single(hashline, minlen: int = 8) -> list:
    """The single generator's words for one hashline (host only), in order, duplicates included: from the BSSID b as a
    48-bit integer the last 12, 10 and 8 hex digits of b - 1, b, b + 1 (mod 2**48) in lower then upper case; from the
    ESSID e the words e, e1, e123, e! each followed by its ASCII upper and lower case where they differ, those shorter
    than minlen left out."""
    ln = _b(hashline)
    lib = L.load()
    nw, nb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = lib.dwpa_assoc_single(ln, len(ln), _u32(minlen, "minlen"), None, 0, None, 0, ctypes.byref(nw), ctypes.byref(nb))
    if rc != L.DWPA_E_OVERFLOW:
        L.check(rc, "assoc_single")
        if rc < 0:
            raise L.DwpaError(rc, "assoc_single: the hashline does not parse")
        return []
    out = ctypes.create_string_buffer(nb.value + 1)
    lens = (ctypes.c_uint32 * max(1, nw.value))()
    L.check(lib.dwpa_assoc_single(ln, len(ln), int(minlen), out, nb.value, lens, nw.value, ctypes.byref(nw),
                                  ctypes.byref(nb)), "assoc_single")
    raw, words, at = out.raw, [], 0
    for k in range(nw.value):
        words.append(raw[at:at + lens[k]])
        at += lens[k]
    return words


def assoc_plan(hash_file, assoc_file=None, single: bool = False, rules_file=None) -> dict:
    """The association attack's plan over a hash file (host only; the nets come from the hash file): {keyspace, nets,
    entries, file_lines, unmatched, malformed, dropped, rules}.  Raises DwpaError for no source, an unreadable file, a
    rules file that loads no rule, a keyspace above 2**64 - 1 or a net with 2**32 or more word x rule choices."""
    info = L.AssocInfo()
    L.check(L.load().dwpa_assoc_plan(_b(hash_file), _opt(assoc_file), _assoc_flags(single), _opt(rules_file),
                                     ctypes.byref(info)), "assoc_plan")
    return {n: int(getattr(info, n)) for n, _ in L.AssocInfo._fields_ if n != "reserved"}


def assoc_candidates(hash_file, indices, assoc_file=None, single: bool = False, rules_file=None) -> list:
    """Candidates `indices` of that plan (host only): [(candidate bytes, or None where the index gives none -- the rule
    rejects, or the result is outside 8..63 bytes --, the first input line of the index's net)]."""
    idx = [_u64(i, "index") for i in indices]
    ia = (ctypes.c_uint64 * max(1, len(idx)))(*idx)
    out = ctypes.create_string_buffer(64 * max(1, len(idx)))
    ol = (ctypes.c_uint32 * max(1, len(idx)))()
    fl = (ctypes.c_uint32 * max(1, len(idx)))()
    L.check(L.load().dwpa_assoc_candidates(_b(hash_file), _opt(assoc_file), _assoc_flags(single), _opt(rules_file), ia,
                                           len(idx), out, ol, fl), "assoc_candidates")
    raw = out.raw
    return [(None if ol[k] == 0xffffffff else raw[64 * k:64 * k + ol[k]], int(fl[k])) for k in range(len(idx))]


def crack_assoc(hash_file, assoc_file=None, single: bool = False, rules_file=None, skip: int = 0, limit: int = 0,
                nonce_error_corrections: int = 8, out_file="help_crack.key", device_mask: int = 0, batch: int = 0,
                nc_mode: int = L.DWPA_NC_HASHCAT) -> int:
    """The association attack over hash_file, on every selected device: every net (ESSID, MAC_AP) against its own words
    -- the MAC_AP:WORD lines of assoc_file, the single generator's with single=True, each under every rule of
    rules_file -- derived with that net's ESSID and verified against that net's lines only.  skip / limit: indices
    [skip, skip + limit) of the keyspace (limit 0 = to the end).  Returns a hashcat exit code (0 cracked, 1 exhausted,
    -1 error)."""
    cfg = L.Config(ctypes.sizeof(L.Config), device_mask, batch, nc_mode)
    return L.load().dwpa_crack_assoc(_b(hash_file), _opt(assoc_file), _assoc_flags(single), _opt(rules_file),
                                     _u64(skip, "skip"), _u64(limit, "limit"), _nc(nonce_error_corrections),
                                     _b(out_file), ctypes.byref(cfg))


def crack_stats():
    """dwpa_crack_last_stats: {words, candidates, hashes, cracked, seconds, rules, rules_skipped, rules_rejmem} of
    this thread's last crack call."""
    st = L.CrackStats()
    L.check(L.load().dwpa_crack_last_stats(ctypes.byref(st)), "crack_last_stats")
    return {"words": st.words, "candidates": st.candidates, "hashes": st.hashes, "cracked": st.cracked,
            "seconds": st.seconds, "rules": st.rules, "rules_skipped": st.rules_skipped,
            "rules_rejmem": st.rules_rejmem}


def crack_worker_stats():
    """dwpa_crack_worker_stats: per shard worker of this thread's last crack call, [{device, items, words,
    candidates, wait_s, scan_s}] (wait_s: time its scanner waited for the shared dictionary feed)."""
    lib = L.load()
    n = ctypes.c_size_t(0)
    L.check(lib.dwpa_crack_worker_stats(None, 0, ctypes.byref(n)), "crack_worker_stats")
    arr = (L.CrackWorker * max(1, n.value))()
    L.check(lib.dwpa_crack_worker_stats(arr, n.value, ctypes.byref(n)), "crack_worker_stats")
    return [{k: getattr(arr[i], k) for k, _ in L.CrackWorker._fields_} for i in range(n.value)]


class Scan:
    """Device-resident scan of one work unit (hashlines grouped by ESSID) -- the client hot loop.

    Pointers are raw device addresses (e.g. ``tensor.data_ptr()``), streams raw ``hipStream_t`` handles
    (e.g. ``torch.cuda.Stream.cuda_stream``); 0 = the null stream.
    """

    def __init__(self, lines, device: int = 0, nc: int = 8, nc_mode: int = L.DWPA_NC_PHP, batch: int = 1 << 22):
        self.lines = [_b(x) for x in lines]
        self._lib = L.load()
        n = len(self.lines)
        lp = (ctypes.c_char_p * max(1, n))(*self.lines)
        ll = (ctypes.c_size_t * max(1, n))(*[len(x) for x in self.lines])
        h = ctypes.c_void_p()
        L.check(self._lib.dwpa_scan_create(device, lp, ll, n, _nc(nc), int(nc_mode), int(batch), ctypes.byref(h)),
                "scan_create")
        self._h = h
        self.batch = (int(batch) + 63) & ~63
        self.groups = self._lib.dwpa_scan_num_groups(h)

    def line_status(self, i: int) -> int:
        return self._lib.dwpa_scan_line_status(self._h, i)

    def load_dict(self, d_offsets: int, d_bytes: int, first: int, count: int, minlen=8, maxlen=63, stream: int = 0):
        L.check(self._lib.dwpa_scan_load_dict(self._h, d_offsets, d_bytes, first, count, minlen, maxlen, stream),
                "scan_load_dict")

    def set_rules(self, rules_text) -> int:
        t = _b(rules_text)
        self.nrules = L.check(self._lib.dwpa_scan_set_rules(self._h, t, len(t)), "scan_set_rules")
        return self.nrules

    def load_rules(self, d_offsets: int, d_bytes: int, first_word: int, nwords: int, stream: int = 0):
        L.check(self._lib.dwpa_scan_load_rules(self._h, d_offsets, d_bytes, first_word, nwords, stream),
                "scan_load_rules")

    def load_numeric(self, first: int, count: int, digits: int = 8, stream: int = 0):
        L.check(self._lib.dwpa_scan_load_numeric(self._h, first, count, digits, stream), "scan_load_numeric")

    def set_mask(self, mask, custom=(), markov=None, threshold: int = 0) -> int:
        """Set the scan's hashcat -a 3 mask (custom: the sets ?1..?4 as raw bytes); returns its keyspace.  markov (a
        model image, markov_load) / threshold: the mask in Markov order under that threshold; load_mask then
        generates that order's candidates, and the keyspace returned is the thresholded one."""
        m = _b(mask)
        arr, keep = _custom(custom)
        k = ctypes.c_uint64(0)
        if markov is not None or threshold:
            model = _model(markov, threshold)
            L.check(self._lib.dwpa_scan_set_mask_markov(self._h, m, len(m), arr, model, len(model),
                                                        _threshold(threshold), ctypes.byref(k)), "scan_set_mask_markov")
            self.keyspace = k.value
            return k.value
        L.check(self._lib.dwpa_scan_set_mask(self._h, m, len(m), arr, ctypes.byref(k)), "scan_set_mask")
        self.keyspace = k.value
        return k.value

    def load_mask(self, first: int, count: int, stream: int = 0):
        """Mask candidates [first, first + count) into slots 0..count-1, generated on the GPU; candidate id = index."""
        if not 0 <= int(count) < 2**32:
            raise L.DwpaError(L.DWPA_E_ARG, f"count {count} is outside uint32")
        L.check(self._lib.dwpa_scan_load_mask(self._h, _u64(first, "first"), int(count), stream), "scan_load_mask")

    def load_hybrid(self, d_offsets: int, d_bytes: int, first_word: int, nwords: int, mask_first: int, mask_count: int,
                    mode: int = L.DWPA_HYBRID_WORD_MASK, minlen=8, maxlen=63, stream: int = 0):
        """Words [first_word, first_word + nwords) x indices [mask_first, mask_first + mask_count) of the mask set by
        set_mask, joined as word + mask candidate (mode 6) or mask candidate + word (mode 7) on the GPU.  Words whose
        joined length is outside minlen..maxlen leave no slots; candidate id = word index * keyspace + mask index."""
        for v, what in ((nwords, "nwords"), (mask_count, "mask_count"), (minlen, "minlen"), (maxlen, "maxlen")):
            if not 0 <= int(v) < 2**32:
                raise L.DwpaError(L.DWPA_E_ARG, f"{what} {v} is outside uint32")
        L.check(self._lib.dwpa_scan_load_hybrid(self._h, d_offsets, d_bytes, _u64(first_word, "first_word"),
                                                int(nwords), _u64(mask_first, "mask_first"), int(mask_count),
                                                int(mode), int(minlen), int(maxlen), stream), "scan_load_hybrid")

    def load_combinator(self, base_off: int, base_bytes: int, first_base: int, nbase: int, amp_off: int,
                        amp_bytes: int, amp_words: int, amp_first: int, amp_count: int,
                        amp_side: int = L.DWPA_COMBI_AMP_RIGHT, minlen=8, maxlen=63, stream: int = 0):
        """Base words [first_base, first_base + nbase) of one HBM-resident list x words [amp_first, amp_first +
        amp_count) of another (the amplifier, amp_words words in all), joined on the GPU as base + amplifier word
        (DWPA_COMBI_AMP_RIGHT) or amplifier word + base (DWPA_COMBI_AMP_LEFT).  A pair is kept iff both words are at most
        63 bytes and the joined length is in minlen..maxlen; candidate id = base index * amp_words + amplifier index."""
        for v, what in ((nbase, "nbase"), (amp_count, "amp_count"), (minlen, "minlen"), (maxlen, "maxlen")):
            if not 0 <= int(v) < 2**32:
                raise L.DwpaError(L.DWPA_E_ARG, f"{what} {v} is outside uint32")
        L.check(self._lib.dwpa_scan_load_combinator(self._h, base_off, base_bytes, _u64(first_base, "first_base"),
                                                    int(nbase), amp_off, amp_bytes, _u64(amp_words, "amp_words"),
                                                    _u64(amp_first, "amp_first"), int(amp_count), int(amp_side),
                                                    int(minlen), int(maxlen), stream), "scan_load_combinator")

    def set_chain(self, parts, custom=()) -> int:
        """Set the scan's chain: 1..4 parts, each (DWPA_CHAIN_LIST, d_offsets, d_bytes, nwords) -- an HBM-resident
        list, which the caller keeps alive -- or (DWPA_CHAIN_MASK, mask).  custom: the sets ?1..?4 shared by the mask
        parts.  Returns the chain's keyspace."""
        parts = list(parts)
        arr = (L.ChainPart * max(1, len(parts)))()
        keep = []
        for i, p in enumerate(parts):
            arr[i].kind = int(p[0])
            if arr[i].kind == L.DWPA_CHAIN_MASK:
                m = _b(p[1])
                keep.append(m)
                arr[i].mask, arr[i].mask_len = m, len(m)
            else:
                arr[i].d_offsets, arr[i].d_bytes, arr[i].nwords = p[1], p[2], _u64(p[3], "nwords")
        carr, ckeep = _custom(custom)
        k = ctypes.c_uint64(0)
        L.check(self._lib.dwpa_scan_set_chain(self._h, arr, len(parts), carr, ctypes.byref(k)), "scan_set_chain")
        self.chain_keyspace = k.value
        return k.value

    def set_chain_rules(self, part: int, rules_text) -> int:
        """Rules on list part `part` of the chain set by set_chain (rules_text: the whole rule language; empty takes
        them off).  The part's choices become its (rule, word) pairs, rule-major: digit = rule * nwords + word, the
        piece is rule(word), and the 63-byte limit applies to that result.  Returns the chain's new keyspace;
        self.chain_nrules holds the number of rules parsed."""
        t = _b(rules_text)
        if not 0 <= int(part) < 2**32:
            raise L.DwpaError(L.DWPA_E_ARG, f"part {part} is outside uint32")
        k = ctypes.c_uint64(0)
        self.chain_nrules = L.check(self._lib.dwpa_scan_set_chain_rules(self._h, int(part), t, len(t), ctypes.byref(k)),
                                    "scan_set_chain_rules")
        self.chain_keyspace = k.value
        return k.value

    def load_chain(self, first: int, count: int, minlen=8, maxlen=63, stream: int = 0):
        """Raw chain candidates [first, first + count), generated and joined on the GPU.  A candidate is kept iff
        every list word in it (for a ruled part: the rule's result) is at most 63 bytes, no ruled part rejects its
        choice and the total length is in minlen..maxlen; kept ones take compacted slots in index order; candidate id
        = its raw index."""
        for v, what in ((count, "count"), (minlen, "minlen"), (maxlen, "maxlen")):
            if not 0 <= int(v) < 2**32:
                raise L.DwpaError(L.DWPA_E_ARG, f"{what} {v} is outside uint32")
        L.check(self._lib.dwpa_scan_load_chain(self._h, _u64(first, "first"), int(count), int(minlen), int(maxlen),
                                               stream), "scan_load_chain")

    def set_table(self, d_offsets: int, d_bytes: int, nwords: int, table, minlen: int = 8, maxlen: int = 63,
                  word_max: int = 0):
        """Set the scan's table attack: an HBM-resident list (nwords + 1 byte offsets and the bytes, which the caller
        keeps alive) under a table text.  The words are counted on the GPU and the kept-word index is built and kept
        by the scan.  Returns (keyspace, kept).  The scan's mask and chain stay as they are."""
        t = _b(table)
        k, kept = ctypes.c_uint64(0), ctypes.c_uint64(0)
        L.check(self._lib.dwpa_scan_set_table(self._h, d_offsets, d_bytes, _u64(nwords, "nwords"), t, len(t),
                                              _u32(minlen, "minlen"), _u32(maxlen, "maxlen"),
                                              _u32(word_max, "word_max"), ctypes.byref(k), ctypes.byref(kept)),
                "scan_set_table")
        self.table_keyspace = k.value
        return k.value, kept.value

    def load_table(self, first: int, count: int, stream: int = 0):
        """Table candidates [first, first + count) into slots 0..count-1, generated on the GPU; candidate id = index."""
        L.check(self._lib.dwpa_scan_load_table(self._h, _u64(first, "first"), _u32(count, "count"), stream),
                "scan_load_table")

    @property
    def nets(self) -> int:
        """The scan's nets: the (ESSID, MAC_AP) pairs of its usable lines, numbered by first appearance."""
        return L.check(self._lib.dwpa_scan_num_nets(self._h), "scan_num_nets")

    def net_of_line(self, i: int) -> int:
        """The net of input line i (raises DwpaError for a line that is not usable)."""
        return L.check(self._lib.dwpa_scan_net_of_line(self._h, i), "scan_net_of_line")

    def set_assoc(self, words, net_of_word, rules_text=b"", minlen: int = 8, maxlen: int = 63) -> int:
        """Set the scan's association: words[i] (1..256 bytes) belongs to net net_of_word[i], net-major (the net
        numbers never decrease), duplicates already dropped.  rules_text: the whole rule language, empty for none.  Net
        n then owns W_n x R indices, rule-major with the word fastest.  Returns the keyspace."""
        ws = list(words)
        nets = [_u32(n, "net") for n in net_of_word]
        if len(nets) != len(ws):
            raise L.DwpaError(L.DWPA_E_ARG, "one net number per word")
        arr, n, keep = _word_array(ws)
        na = (ctypes.c_uint32 * max(1, n))(*nets)
        t = _b(rules_text)
        k = ctypes.c_uint64(0)
        L.check(self._lib.dwpa_scan_set_assoc(self._h, arr, na, n, t, len(t), _u32(minlen, "minlen"),
                                              _u32(maxlen, "maxlen"), ctypes.byref(k)), "scan_set_assoc")
        self.assoc_keyspace = k.value
        return k.value

    def load_assoc(self, first: int, count: int, stream: int = 0):
        """Association indices [first, first + count), generated on the GPU: the kept candidates of nets that still
        have an uncracked line take compacted slots in index order; candidate id = its index.  run() then derives each
        slot with its own net's ESSID and verifies it against that net's uncracked lines only."""
        L.check(self._lib.dwpa_scan_load_assoc(self._h, _u64(first, "first"), _u32(count, "count"), stream),
                "scan_load_assoc")

    def pbkdf2(self, group: int = 0, stream: int = 0):
        L.check(self._lib.dwpa_scan_pbkdf2(self._h, group, stream), "scan_pbkdf2")

    def verify(self, group: int = 0, stream: int = 0):
        L.check(self._lib.dwpa_scan_verify(self._h, group, stream), "scan_verify")

    def run(self, stream: int = 0):
        """PBKDF2 + verify of the loaded batch for every ESSID group with an uncracked line, many groups per
        launch (dwpa_scan_run)."""
        L.check(self._lib.dwpa_scan_run(self._h, stream), "scan_run")

    def loaded(self, stream: int = 0) -> int:
        c = ctypes.c_uint32(0)
        L.check(self._lib.dwpa_scan_loaded(self._h, ctypes.byref(c), stream), "scan_loaded")
        return c.value

    def hits(self, stream: int = 0, cap: int = 1 << 16):
        buf = (L.Hit * cap)()
        n = ctypes.c_size_t(0)
        L.check(self._lib.dwpa_scan_hits(self._h, buf, cap, ctypes.byref(n), stream), "scan_hits")
        out = []
        for i in range(min(n.value, cap)):
            h = buf[i]
            out.append({"cand": int(h.cand), "line": int(h.line),
                        "nc": int(h.nc) if h.nc_valid else None,
                        "endian": _ENDIAN[int(h.endian)] if h.nc_valid else None,
                        "pmk": bytes(h.pmk)})
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._lib.dwpa_scan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
