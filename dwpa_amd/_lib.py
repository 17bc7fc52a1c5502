"""ctypes binding of libdwpa22000.so (include/dwpa22000.h).

Importing works anywhere.  The check path and PBKDF2 run on the gfx950 device, or on the library's own host backend
for small calls and -- only when asked for (dwpa_config.allow_cpu_fallback, DWPA_CPU_FALLBACK=1) -- without a device;
otherwise a call without a device returns DWPA_E_NODEV and the wrappers raise ``DwpaError``, loudly.  The client
path (crack_files, scans, rule expansion) is device-only.
"""
from __future__ import annotations

import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DWPA_LIB", os.path.join(HERE, "lib", "libdwpa22000.so"))
HEADER = os.path.join(os.path.dirname(HERE), "include", "dwpa22000.h")

DWPA_MISS, DWPA_HIT = 0, 1
DWPA_E_FORMAT, DWPA_E_HEX, DWPA_E_TYPE, DWPA_E_KEYVER = -1, -2, -3, -4
DWPA_E_NODEV, DWPA_E_HIP, DWPA_E_ARG, DWPA_E_NOMEM, DWPA_E_IO, DWPA_E_OVERFLOW, DWPA_E_RULE = -10, -11, -12, -13, -14, -15, -16
DWPA_RC_CRACKED, DWPA_RC_EXHAUSTED, DWPA_RC_ERROR = 0, 1, -1
DWPA_NC_PHP, DWPA_NC_HASHCAT = 0, 1
DWPA_NC_MAX = 65664  # the largest nc / nonce_error_corrections taken (include/dwpa22000.h)
DWPA_HYBRID_WORD_MASK, DWPA_HYBRID_MASK_WORD = 6, 7  # hashcat -a 6 (word || mask) / -a 7 (mask || word)
DWPA_COMBI_AMP_RIGHT, DWPA_COMBI_AMP_LEFT = 0, 1  # hashcat -a 1: the list held whole in device memory
DWPA_CHAIN_LIST, DWPA_CHAIN_MASK, DWPA_CHAIN_MAX_PARTS = 0, 1, 4  # chain attack: the kind of a part, the most parts
DWPA_MARKOV_BYTES = 4128784  # a Markov model file / image: 16-byte header + 63 x 256 rows of 256 bytes
DWPA_TABLE_MAX_ALT, DWPA_TABLE_IMAGE_BYTES = 16, 4352  # table attack: alternatives per byte, the parsed table image
DWPA_ASSOC_SINGLE = 1  # association attack flags: add the single generator's words to every net
DWPA_DICT_OK, DWPA_DICT_DAMAGED = 0, 1  # dwpa_crack_files_ex per-dictionary status (or DWPA_E_IO)
DWPA_RULES_DEFAULT, DWPA_RULES_HASHCAT, DWPA_RULES_FULL = 0, 1, 2  # dwpa_config.rule_mode
DWPA_BACKEND_DEVICE, DWPA_BACKEND_HOST_SMALL, DWPA_BACKEND_HOST_FALLBACK = 0, 1, 2  # dwpa_check_stats.backend


class DwpaError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"dwpa error {code}: {msg}")
        self.code = code


class Bytes(ctypes.Structure):
    _fields_ = [("ptr", ctypes.c_void_p), ("len", ctypes.c_size_t)]


class Result(ctypes.Structure):
    _fields_ = [("key_index", ctypes.c_int32), ("nc", ctypes.c_int32), ("endian", ctypes.c_int8),
                ("nc_valid", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 2), ("pmk", ctypes.c_uint8 * 32)]


class Job(ctypes.Structure):
    _fields_ = [("line", ctypes.c_char_p), ("line_len", ctypes.c_size_t), ("keys", ctypes.POINTER(Bytes)),
                ("nkeys", ctypes.c_size_t), ("pmk", ctypes.c_char_p), ("nc", ctypes.c_int32)]


class Config(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("device_mask", ctypes.c_uint32), ("batch", ctypes.c_uint32),
                ("nc_mode", ctypes.c_int32), ("rule_mode", ctypes.c_int32), ("allow_cpu_fallback", ctypes.c_int32),
                ("host_max_pmks", ctypes.c_int32), ("reserved", ctypes.c_int32 * 1)]


class CrackStats(ctypes.Structure):
    _fields_ = [("words", ctypes.c_uint64), ("candidates", ctypes.c_uint64), ("hashes", ctypes.c_uint32),
                ("cracked", ctypes.c_uint32), ("seconds", ctypes.c_double), ("rules", ctypes.c_uint32),
                ("rules_skipped", ctypes.c_uint32), ("rules_rejmem", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class CrackWorker(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("items", ctypes.c_uint32), ("words", ctypes.c_uint64),
                ("candidates", ctypes.c_uint64), ("wait_s", ctypes.c_double), ("scan_s", ctypes.c_double)]


class CheckStats(ctypes.Structure):
    _fields_ = [("jobs", ctypes.c_uint32), ("slots", ctypes.c_uint32), ("pmks", ctypes.c_uint32),
                ("tail_pmks", ctypes.c_uint32), ("tail_waves", ctypes.c_uint32), ("tail_waves_raised", ctypes.c_uint32),
                ("hits", ctypes.c_uint32), ("backend", ctypes.c_uint32), ("seconds", ctypes.c_double)]


class Resources(ctypes.Structure):
    _fields_ = [("device_bytes", ctypes.c_uint64), ("pinned_host_bytes", ctypes.c_uint64),
                ("host_pool_threads", ctypes.c_uint32), ("devices", ctypes.c_uint32), ("call_contexts", ctypes.c_uint32),
                ("call_contexts_used", ctypes.c_uint32)]


class RulesCounts(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("present", "parsed", "loaded_hashcat", "rejmem", "invalid",
                                               "first_invalid_line", "first_rejmem_line", "reserved")]


class LineInfo(ctypes.Structure):
    _fields_ = [("type", ctypes.c_int32), ("keyver", ctypes.c_int32), ("essid_len", ctypes.c_uint32),
                ("mac_ap_len", ctypes.c_uint32), ("mac_sta_len", ctypes.c_uint32), ("target_len", ctypes.c_uint32),
                ("attempts", ctypes.c_uint32), ("lists", ctypes.c_uint32), ("never_matches", ctypes.c_uint32),
                ("essid", ctypes.c_uint8 * 32), ("mac_ap", ctypes.c_uint8 * 16), ("mac_sta", ctypes.c_uint8 * 16),
                ("hash_m22000", ctypes.c_uint8 * 16)]


class Hit(ctypes.Structure):
    _fields_ = [("cand", ctypes.c_uint64), ("line", ctypes.c_uint32), ("nc", ctypes.c_int32), ("endian", ctypes.c_int8),
                ("nc_valid", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 2), ("pmk", ctypes.c_uint8 * 32)]


class ChainPart(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("d_offsets", ctypes.c_void_p), ("d_bytes", ctypes.c_void_p),
                ("nwords", ctypes.c_uint64), ("mask", ctypes.c_char_p), ("mask_len", ctypes.c_size_t)]


class AssocInfo(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("keyspace", "nets", "entries", "file_lines", "unmatched", "malformed",
                                               "dropped")] + [("rules", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class ChainSpec(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("text", ctypes.c_char_p)]


_P = ctypes.c_void_p
SIGNATURES = {
    "dwpa_abi_version": ([], ctypes.c_int),
    "dwpa_init": ([ctypes.POINTER(Config)], ctypes.c_int),
    "dwpa_device_count": ([], ctypes.c_int),
    "dwpa_strerror": ([ctypes.c_int], ctypes.c_char_p),
    "dwpa_shutdown": ([], None),
    "dwpa_check_m22000": ([ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(Bytes), ctypes.c_size_t, ctypes.c_char_p,
                           ctypes.c_int, ctypes.POINTER(Result)], ctypes.c_int),
    "dwpa_check_batch": ([ctypes.POINTER(Job), ctypes.c_size_t, ctypes.POINTER(Result), ctypes.POINTER(ctypes.c_int)],
                         ctypes.c_int),
    "dwpa_check_last_stats": ([ctypes.POINTER(CheckStats)], ctypes.c_int),
    "dwpa_resource_stats": ([ctypes.POINTER(Resources)], ctypes.c_int),
    "dwpa_pbkdf2_pmk": ([ctypes.POINTER(Bytes), ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, _P], ctypes.c_int),
    "dwpa_hc_unhex": ([ctypes.c_char_p, ctypes.c_size_t, _P, ctypes.POINTER(ctypes.c_size_t)], ctypes.c_int),
    "dwpa_hash_m22000": ([ctypes.c_char_p, ctypes.c_size_t, _P], ctypes.c_int),
    "dwpa_parse_m22000": ([ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_void_p], ctypes.c_int),
    "dwpa_crack_files": ([ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_size_t, ctypes.c_char_p, ctypes.c_int,
                          ctypes.c_char_p, ctypes.POINTER(Config)], ctypes.c_int),
    "dwpa_crack_last_stats": ([ctypes.POINTER(CrackStats)], ctypes.c_int),
    "dwpa_crack_worker_stats": ([ctypes.POINTER(CrackWorker), ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)],
                                ctypes.c_int),
    "dwpa_crack_files_ex": ([ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_size_t, ctypes.c_char_p,
                             ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(Config), ctypes.POINTER(ctypes.c_int32)],
                            ctypes.c_int),
    "dwpa_rules_expand": ([ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(Bytes), ctypes.c_size_t, _P, _P,
                           ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
    "dwpa_rules_expand_file": ([ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_size_t,
                                ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64),
                                ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int),
    "dwpa_rules_count": ([ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32),
                          ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
    "dwpa_rules_count_ex": ([ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(RulesCounts)], ctypes.c_int),
    "dwpa_rules_apply_host": ([ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_size_t, _P,
                               ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
    "dwpa_scan_create": ([ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_size_t), ctypes.c_size_t,
                          ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.POINTER(_P)], ctypes.c_int),
    "dwpa_scan_num_groups": ([_P], ctypes.c_int),
    "dwpa_scan_line_status": ([_P, ctypes.c_size_t], ctypes.c_int),
    "dwpa_scan_load_dict": ([_P, _P, _P, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _P],
                            ctypes.c_int),
    "dwpa_scan_set_rules": ([_P, ctypes.c_char_p, ctypes.c_size_t], ctypes.c_int),
    "dwpa_scan_load_rules": ([_P, _P, _P, ctypes.c_uint64, ctypes.c_uint32, _P], ctypes.c_int),
    "dwpa_scan_load_numeric": ([_P, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _P], ctypes.c_int),
    "dwpa_mask_keyspace": ([ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(Bytes), ctypes.POINTER(ctypes.c_uint32),
                            ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int),
    "dwpa_mask_candidate": ([ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(Bytes), ctypes.c_uint64, _P,
                             ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
    "dwpa_scan_set_mask": ([_P, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(Bytes),
                            ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int),
    "dwpa_scan_load_mask": ([_P, ctypes.c_uint64, ctypes.c_uint32, _P], ctypes.c_int),
    "dwpa_scan_load_hybrid": ([_P, _P, _P, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32,
                               ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, _P], ctypes.c_int),
    "dwpa_crack_hybrid": ([ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_size_t, ctypes.c_char_p,
                           ctypes.POINTER(Bytes), ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(Config),
                           ctypes.POINTER(ctypes.c_int32)], ctypes.c_int),
    "dwpa_scan_load_combinator": ([_P, _P, _P, ctypes.c_uint64, ctypes.c_uint32, _P, _P, ctypes.c_uint64,
                                   ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, _P],
                                  ctypes.c_int),
    "dwpa_crack_combinator": ([ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int,
                               ctypes.c_char_p, ctypes.POINTER(Config), ctypes.POINTER(ctypes.c_int32)], ctypes.c_int),
    "dwpa_scan_set_chain": ([_P, ctypes.POINTER(ChainPart), ctypes.c_uint32, ctypes.POINTER(Bytes),
                             ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int),
    "dwpa_scan_load_chain": ([_P, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _P], ctypes.c_int),
    "dwpa_chain_keyspace": ([ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)],
                            ctypes.c_int),
    "dwpa_chain_split": ([ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32, ctypes.c_uint64,
                          ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int),
    "dwpa_crack_chain": ([ctypes.c_char_p, ctypes.POINTER(ChainSpec), ctypes.c_uint32, ctypes.POINTER(Bytes),
                          ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(Config),
                          ctypes.POINTER(ctypes.c_int32)], ctypes.c_int),
    "dwpa_scan_set_chain_rules": ([_P, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_size_t,
                                   ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int),
    "dwpa_crack_chain_rules": ([ctypes.c_char_p, ctypes.POINTER(ChainSpec), ctypes.c_uint32,
                                ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(Bytes), ctypes.c_uint64,
                                ctypes.c_uint64, ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(Config),
                                ctypes.POINTER(ctypes.c_int32)], ctypes.c_int),
    "dwpa_crack_mask": ([ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(Bytes), ctypes.c_uint64, ctypes.c_uint64,
                         ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(Config)],
                        ctypes.c_int),
    "dwpa_markov_train": ([ctypes.POINTER(ctypes.c_char_p), ctypes.c_size_t, ctypes.c_char_p,
                           ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int),
    "dwpa_markov_load": ([ctypes.c_char_p, _P, ctypes.c_size_t], ctypes.c_int),
    "dwpa_markov_check": ([ctypes.c_char_p, ctypes.c_size_t], ctypes.c_int),
    "dwpa_mask_keyspace_markov": ([ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(Bytes), ctypes.c_uint32,
                                   ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int),
    "dwpa_mask_candidate_markov": ([ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(Bytes), ctypes.c_char_p,
                                    ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint64, _P,
                                    ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
    "dwpa_mask_candidates_markov": ([ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(Bytes), ctypes.c_char_p,
                                     ctypes.c_size_t, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t,
                                     _P, ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
    "dwpa_scan_set_mask_markov": ([_P, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(Bytes), ctypes.c_char_p,
                                   ctypes.c_size_t, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int),
    "dwpa_crack_mask_markov": ([ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(Bytes), ctypes.c_char_p,
                                ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(Config)], ctypes.c_int),
    "dwpa_table_parse": ([ctypes.c_char_p, ctypes.c_size_t, _P, ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
    "dwpa_table_builtin": ([ctypes.c_char_p, _P, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)], ctypes.c_int),
    "dwpa_table_keyspace": ([ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(Bytes), ctypes.c_size_t, ctypes.c_uint32,
                             ctypes.c_uint32, ctypes.c_uint32] + [ctypes.POINTER(ctypes.c_uint64)] * 4, ctypes.c_int),
    "dwpa_table_candidates": ([ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(Bytes), ctypes.c_size_t,
                               ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64),
                               ctypes.c_size_t, _P, ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
    "dwpa_scan_set_table": ([_P, _P, _P, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32,
                             ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64),
                             ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int),
    "dwpa_scan_load_table": ([_P, ctypes.c_uint64, ctypes.c_uint32, _P], ctypes.c_int),
    "dwpa_crack_table": ([ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint64,
                          ctypes.c_uint64, ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(Config)], ctypes.c_int),
    "dwpa_assoc_single": ([ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, _P, ctypes.c_size_t,
                           ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                           ctypes.POINTER(ctypes.c_size_t)], ctypes.c_int),
    "dwpa_assoc_plan": ([ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p,
                         ctypes.POINTER(AssocInfo)], ctypes.c_int),
    "dwpa_assoc_candidates": ([ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p,
                               ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t, _P, ctypes.POINTER(ctypes.c_uint32),
                               ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
    "dwpa_scan_num_nets": ([_P], ctypes.c_int),
    "dwpa_scan_net_of_line": ([_P, ctypes.c_size_t], ctypes.c_int64),
    "dwpa_scan_set_assoc": ([_P, ctypes.POINTER(Bytes), ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t,
                             ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32,
                             ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int),
    "dwpa_scan_load_assoc": ([_P, ctypes.c_uint64, ctypes.c_uint32, _P], ctypes.c_int),
    "dwpa_crack_assoc": ([ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint64,
                          ctypes.c_uint64, ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(Config)], ctypes.c_int),
    "dwpa_scan_pbkdf2": ([_P, ctypes.c_int, _P], ctypes.c_int),
    "dwpa_scan_verify": ([_P, ctypes.c_int, _P], ctypes.c_int),
    "dwpa_scan_run": ([_P, _P], ctypes.c_int),
    "dwpa_scan_hits": ([_P, ctypes.POINTER(Hit), ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), _P], ctypes.c_int),
    "dwpa_scan_loaded": ([_P, ctypes.POINTER(ctypes.c_uint32), _P], ctypes.c_int),
    "dwpa_scan_destroy": ([_P], None),
    "dwpa_dev_alloc": ([ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(_P)], ctypes.c_int),
    "dwpa_dev_free": ([ctypes.c_int, _P], ctypes.c_int),
    "dwpa_dev_upload": ([ctypes.c_int, _P, _P, ctypes.c_size_t], ctypes.c_int),
    "dwpa_dev_download": ([ctypes.c_int, _P, _P, ctypes.c_size_t], ctypes.c_int),
    "dwpa_stream_create": ([ctypes.c_int, ctypes.POINTER(_P)], ctypes.c_int),
    "dwpa_stream_sync": ([_P], ctypes.c_int),
    "dwpa_stream_destroy": ([_P], ctypes.c_int),
    "dwpa_event_create": ([ctypes.c_int, ctypes.POINTER(_P)], ctypes.c_int),
    "dwpa_event_record": ([_P, _P], ctypes.c_int),
    "dwpa_event_elapsed_ms": ([_P, _P, ctypes.POINTER(ctypes.c_float)], ctypes.c_int),
    "dwpa_event_destroy": ([_P], ctypes.c_int),
    "dwpa_debug_pbkdf2_kernels": ([ctypes.c_int], ctypes.c_uint32),  # test hook, not in include/dwpa22000.h
    "dwpa_debug_verify_kernels": ([ctypes.c_int], ctypes.c_uint32),  # test hook, not in include/dwpa22000.h
    "dwpa_debug_check_hit_records": ([ctypes.c_int], ctypes.c_uint64),  # test hook, not in include/dwpa22000.h
    "dwpa_debug_scan_work": ([ctypes.POINTER(ctypes.c_uint64), ctypes.c_int], None),  # test hook, not in the header
    "dwpa_debug_crack_loads": ([ctypes.POINTER(ctypes.c_uint64), ctypes.c_int], None),  # test hook, not in the header
    "dwpa_debug_assoc_work": ([ctypes.POINTER(ctypes.c_uint64), ctypes.c_int], None),  # test hook, not in the header
    "dwpa_debug_assoc_segcap": ([ctypes.c_uint32], ctypes.c_uint32),  # test hook, not in the header
    "dwpa_debug_scan_prepared": ([_P, _P, _P, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), _P, _P],
                                 ctypes.c_int),  # test hook, not in the header
    "dwpa_debug_scan_pmks": ([_P, ctypes.c_int, ctypes.c_int, _P, ctypes.c_uint32, _P],
                             ctypes.c_int),  # test hook, not in the header
}

# Bit i of dwpa_debug_pbkdf2_kernels' mask (csrc/kernels.hpp Pbkdf2Kernel): the hipcc-scheduled kernels of kernels.hip,
# then the issue-pass code object's (one ESSID / per-slot salt / ESSID groups; _p priority, _q work queue).
PBKDF2_KERNEL_NAMES = ("k_pbkdf2", "k_pbkdf2_ms", "k_pbkdf2_mg", "k_pbkdf2_ms_tail",
                       "k_pbkdf2_gfx950", "k_pbkdf2_gfx950_ms", "k_pbkdf2_gfx950_mg",
                       "k_pbkdf2_gfx950_p", "k_pbkdf2_gfx950_ms_p", "k_pbkdf2_gfx950_mg_p",
                       "k_pbkdf2_gfx950_q", "k_pbkdf2_gfx950_mg_q")

# Bit i of dwpa_debug_verify_kernels' mask (csrc/kernels.hpp verify_kernel_bit): the key-parallel kernel's classes
# (PMKID, keyver 1, 2, 3, 1|2 combined, all four: the scan path's mixed launches), then the attempt-parallel pair
# k_eapol_keys + k_verify_att of the same classes (EAPOL lines with >= 64 attempts on the check path).
VERIFY_KERNEL_NAMES = ("k_verify<pmkid>", "k_verify<kv1>", "k_verify<kv2>", "k_verify<kv3>", "k_verify<kv1|kv2>",
                       "k_verify<all>", "k_verify_att<pmkid>", "k_verify_att<kv1>", "k_verify_att<kv2>",
                       "k_verify_att<kv3>", "k_verify_att<kv1|kv2>", "k_verify_att<all>")

_lib = None


def load():
    """Load the shared library (raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DwpaError(DWPA_E_NODEV, f"{LIB_PATH} missing: run `make` (or __graft_entry__.build())")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (args, res) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.argtypes = args
            fn.restype = res
        _lib = lib
    return _lib


def pbkdf2_kernels(reset: bool = False) -> frozenset:
    """Names of the PBKDF2 kernels this process has launched since the last reset (the library's test hook): which
    of pbkdf2_module.cpp's variants a call really ran."""
    mask = int(load().dwpa_debug_pbkdf2_kernels(1 if reset else 0))
    assert mask >> len(PBKDF2_KERNEL_NAMES) == 0, hex(mask)
    return frozenset(n for i, n in enumerate(PBKDF2_KERNEL_NAMES) if mask >> i & 1)


def verify_kernels(reset: bool = False) -> frozenset:
    """Names of the verify kernels this process has launched since the last reset (the library's test hook): which
    verifier, key-parallel k_verify or attempt-parallel k_verify_att, and which class of it a call really ran."""
    mask = int(load().dwpa_debug_verify_kernels(1 if reset else 0))
    assert mask >> len(VERIFY_KERNEL_NAMES) == 0, hex(mask)
    return frozenset(n for i, n in enumerate(VERIFY_KERNEL_NAMES) if mask >> i & 1)


def check_hit_records(reset: bool = False) -> int:
    """Hit records the device check path has read back in this process since the last reset (test hook): every
    matching (key, attempt) item the verify kernels reported, where dwpa_check_stats.hits counts jobs with a hit."""
    return int(load().dwpa_debug_check_hit_records(1 if reset else 0))


SCAN_WORK_NAMES = ("groups_derived", "pbkdf2_launches", "line_rows")


def scan_work(reset: bool = False) -> dict:
    """What the scan path has launched in this process since the last reset (test hook): ESSID groups derived (per
    multi-group launch its groups, plus 1 per dwpa_scan_pbkdf2 that launched), multi-group PBKDF2 launches of
    dwpa_scan_run, and line rows handed to the verify kernels.  A retired line or group adds to none of them."""
    out = (ctypes.c_uint64 * 3)()
    load().dwpa_debug_scan_work(out, 1 if reset else 0)
    return dict(zip(SCAN_WORK_NAMES, (int(v) for v in out)))


CRACK_LOAD_NAMES = ("loads", "overflowed", "empty", "scanned")


def crack_loads(reset: bool = False) -> dict:
    """What the crack loop's load sizing has issued in this process since the last reset (test hook), over the
    dictionary, rules, hybrid and combinator runs: device loads, loads that overflowed the batch and were repeated
    with fewer words, loads that kept nothing (no scan), and loads scanned.  loads = overflowed + empty + scanned."""
    out = (ctypes.c_uint64 * 4)()
    load().dwpa_debug_crack_loads(out, 1 if reset else 0)
    return dict(zip(CRACK_LOAD_NAMES, (int(v) for v in out)))


ASSOC_WORK_NAMES = ("slots_derived", "segments")


def assoc_work(reset: bool = False) -> dict:
    """What association runs (dwpa_scan_run after load_assoc) have launched in this process since the last reset (test
    hook): slots derived -- one PBKDF2 each -- and segments handed to the verify kernels.  A net whose lines are all
    retired adds to neither."""
    out = (ctypes.c_uint64 * 2)()
    load().dwpa_debug_assoc_work(out, 1 if reset else 0)
    return dict(zip(ASSOC_WORK_NAMES, (int(v) for v in out)))


def assoc_segcap(records: int = 0) -> int:
    """Set the number of records a scan's segment lists start with (test hook; 0: the default); returns the previous
    setting.  A list that is too short is grown and its load repeated."""
    return int(load().dwpa_debug_assoc_segcap(int(records)))


def scan_prepared(scan, stream: int = 0, sref: bool = False) -> dict:
    """The batch of a m22000.Scan as its last load_* prepared it (test hook; no kernel runs): {"count": the kept
    counter as the kernel left it, not clamped to the batch; "ids": uint64[n]; "mid": uint32[10][n], the HMAC-SHA1 key
    midstates (ipad h0..h4, opad h0..h4) of slot j in column j; "sref": uint32[n] after an association load when asked
    for, else None}, n = min(count, the scan's batch)."""
    import numpy as np
    cap = int(scan.batch)
    ids = np.zeros(cap, dtype=np.uint64)
    mid = np.zeros(10 * cap, dtype=np.uint32)
    sr = np.zeros(cap, dtype=np.uint32) if sref else None
    count = ctypes.c_uint32(0)
    check(load().dwpa_debug_scan_prepared(scan._h, ids.ctypes.data, mid.ctypes.data, cap, ctypes.byref(count),
                                          sr.ctypes.data if sref else None, stream), "debug_scan_prepared")
    n = min(count.value, cap)
    return {"count": count.value, "ids": ids[:n].copy(), "mid": mid[:10 * n].reshape(10, n).copy(),
            "sref": sr[:n].copy() if sref else None}


def scan_pmks(scan, group=None, run: bool = False, stream: int = 0):
    """The PMKs of a m22000.Scan where its verifier reads them (test hook; no kernel runs): uint32[8][batch], the eight
    big-endian words of slot j in column j, for the whole batch width -- a slot past the loaded count holds what an
    earlier derive left there.  run=False: what pbkdf2(g) of any group or the run() of an association load wrote last;
    run=True: group `group`'s column block of the last run() that was no association run (DwpaError DWPA_E_ARG for a
    group that launch did not hold)."""
    import numpy as np
    if run and group is None:
        raise DwpaError(DWPA_E_ARG, "run=True reads one group's block: name the group")
    cap = int(scan.batch)
    out = np.zeros(8 * cap, dtype=np.uint32)
    check(load().dwpa_debug_scan_pmks(scan._h, 1 if run else 0, int(group or 0), out.ctypes.data, cap, stream),
          "debug_scan_pmks")
    return out.reshape(8, cap)


def check(rc: int, what: str = "") -> int:
    if rc < 0 and rc not in (DWPA_E_FORMAT, DWPA_E_HEX, DWPA_E_TYPE, DWPA_E_KEYVER):
        raise DwpaError(rc, (what + ": " if what else "") + load().dwpa_strerror(rc).decode(errors="replace"))
    return rc


def bytes_array(items):
    """Python sequence of bytes/None -> (ctypes array of Bytes, keep-alive list)."""
    arr = (Bytes * max(1, len(items)))()
    keep = []
    for i, k in enumerate(items):
        if k is None:
            arr[i].ptr, arr[i].len = None, 0
        else:
            k = bytes(k)
            b = ctypes.create_string_buffer(k, len(k) + 1)
            keep.append(b)
            arr[i].ptr, arr[i].len = ctypes.cast(b, ctypes.c_void_p), len(k)
    return arr, keep
