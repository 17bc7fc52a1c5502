/*
 * dwpa22000.h -- C ABI of libdwpa22000.so, the MI355X (gfx950) m22000 PMK derivation + verification engine.
 *
 * Drop-in boundary for dwpa's one data-parallel hot path (PBKDF2-HMAC-SHA1 x4096 over an ESSID salt, then
 * PMKID / EAPOL keyver 1,2,3 checks with nonce-error-correction).  Two callers bind it:
 *
 *   (1) PHP FFI on the server, in place of check_key_m22000()      web/common.php:157-307
 *       call sites common.php:592 (zero PMK), :606 (PMK reuse), :902 (put_work), :919 (PMK propagation),
 *       web/rkg.php:126,147 (router-keygen / single-mode bulk checks)
 *   (2) Python ctypes in help_crack.py, in place of run_cracker()'s hashcat subprocess
 *       help_crack/help_crack.py:765-802 (command line :773, rc handling :776-786, outfile parsed by get_key :804-879)
 *
 * Plain C types only.  The caller owns every buffer; the library keeps no caller pointer after a call returns and
 * returns no heap memory.  All entry points are thread-safe.
 *
 * Two backends answer the check path (dwpa_check_m22000, dwpa_check_batch) and dwpa_pbkdf2_pmk:
 *   - the gfx950 device (the hot path: PBKDF2 and the verifiers as hand-written HIP kernels);
 *   - the library's host backend (its own SHA-1 / SHA-256 / MD5 / AES-128, with SHA-NI / AES-NI where the CPU has
 *     them, over the host pool's threads), the same semantics and the same results, which answers
 *       (a) small calls -- at least one PBKDF2 derive and at most dwpa_config.host_max_pmks PMK-equivalents (put_work
 *           checks one key per call, common.php:902, and one PBKDF2 chain on a lone GPU wave takes ~8 ms), and
 *       (b) every call, when no usable gfx950 device exists or a device call failed, if allow_cpu_fallback is on.
 *   dwpa_check_last_stats().backend says which one answered a call.  The client path (dwpa_crack_files, dwpa_scan_*,
 *   dwpa_rules_expand*) is device-only: without a device it returns DWPA_E_NODEV / DWPA_RC_ERROR.
 *
 * Concurrent check calls (dwpa_check_m22000 / dwpa_check_batch / dwpa_pbkdf2_pmk from several threads) run on up to
 * DWPA_CALLS_PER_DEVICE (default 2) call contexts per device at once and overlap on the GPU; more callers wait for
 * a free context.  Separate processes (PHP-FPM workers) each hold their own contexts.
 */
#ifndef DWPA22000_H
#define DWPA22000_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DWPA_ABI_VERSION 4   /* 2: dwpa_crack_stats.rules / rules_skipped, dwpa_rules_count; 3: dwpa_check_last_stats,
                                dwpa_config.rule_mode, dwpa_rules_count_ex, dwpa_crack_stats.rules_rejmem; 4: the host
                                backend -- dwpa_config.allow_cpu_fallback / host_max_pmks, dwpa_check_stats.backend.
                                Added since without a new version or error code, discoverable by symbol: the mask
                                attack -- dwpa_mask_keyspace, dwpa_mask_candidate, dwpa_scan_set_mask,
                                dwpa_scan_load_mask, dwpa_crack_mask; the hybrid attacks -- dwpa_scan_load_hybrid,
                                dwpa_crack_hybrid; the combinator attack -- dwpa_scan_load_combinator,
                                dwpa_crack_combinator; the mask attack in Markov order -- dwpa_markov_train,
                                dwpa_markov_load, dwpa_markov_check, dwpa_mask_keyspace_markov,
                                dwpa_mask_candidate_markov, dwpa_mask_candidates_markov, dwpa_scan_set_mask_markov,
                                dwpa_crack_mask_markov; the table attack -- dwpa_table_parse, dwpa_table_builtin,
                                dwpa_table_keyspace, dwpa_table_candidates, dwpa_scan_set_table,
                                dwpa_scan_load_table, dwpa_crack_table; the association attack --
                                dwpa_assoc_single, dwpa_assoc_plan, dwpa_assoc_candidates, dwpa_scan_num_nets,
                                dwpa_scan_net_of_line, dwpa_scan_set_assoc, dwpa_scan_load_assoc, dwpa_crack_assoc */

/* ---- return codes ------------------------------------------------------------------------------------------ */
#define DWPA_MISS 0            /* no key matched (PHP: False)                                                 */
#define DWPA_HIT 1             /* a key matched; the result struct is filled (PHP: [PSK, NC, endian, PMK])   */
#define DWPA_E_FORMAT (-1)     /* not 9 '*'-separated fields or signature != "WPA"   (common.php:159-161)     */
#define DWPA_E_HEX (-2)        /* a required field is not valid even-length hex       (common.php:28-36,162-195) */
#define DWPA_E_TYPE (-3)       /* type field is neither 01 nor 02                     (common.php:167,190,306) */
#define DWPA_E_KEYVER (-4)     /* EAPOL key version not 1/2/3 or EAPOL < 49 bytes     (common.php:274-276)     */
#define DWPA_E_NODEV (-10)     /* no usable gfx950 device (and allow_cpu_fallback off)                         */
#define DWPA_E_HIP (-11)       /* HIP runtime error                                                            */
#define DWPA_E_ARG (-12)       /* invalid argument                                                             */
#define DWPA_E_NOMEM (-13)     /* host or device allocation failed                                             */
#define DWPA_E_IO (-14)        /* file could not be read or written                                            */
#define DWPA_E_OVERFLOW (-15)  /* hit buffer overflow                                                          */
#define DWPA_E_RULE (-16)      /* unsupported or malformed rule                                                */
/* -1..-4 are check_key_m22000's own False returns (malformed line).  Codes <= -10 are device/runtime failures:
 * the result is unknown, so wrappers must not turn them into False (put_work, common.php:902,919, would read
 * "wrong PSK"); php/dwpa22000.php hands such jobs to the original PHP check or throws. */

/* hashcat exit codes returned by dwpa_crack_files (help_crack.py:776-786,930 interpret them) */
#define DWPA_RC_CRACKED 0      /* every hashline cracked                                                       */
#define DWPA_RC_EXHAUSTED 1    /* keyspace exhausted, not every hashline cracked                               */
#define DWPA_RC_ERROR (-1)

/* rule-file loading (dwpa_config.rule_mode; dwpa_crack_files' -r rules and dwpa_rules_expand_file) */
#define DWPA_RULES_DEFAULT 0   /* the process's mode: dwpa_init's rule_mode, else DWPA_RULE_MODE=full|hashcat from the
                                  environment, else DWPA_RULES_HASHCAT                                            */
#define DWPA_RULES_HASHCAT 1   /* hashcat's -r loader: a line using a reject function (< > _ ! / ( ) = % Q) or a memory
                                  function (M 4 6 X) is skipped and counted like an invalid one -- those work only
                                  with -j/-k -- so the candidates are the ones hashcat -r tries (default).  Parity
                                  unpinned: hashcat is not in the reference, no reference file shows which lines -r
                                  skips; this follows hashcat's documentation (oracle/rules.py).  Rules relying on
                                  those functions: DWPA_RULES_FULL / DWPA_RULE_MODE=full                          */
#define DWPA_RULES_FULL 2      /* every line of the whole rule language runs, reject and memory functions included (a
                                  superset of hashcat -r's candidates)                                             */

/* nonce-error-correction semantics */
#define DWPA_NC_PHP 0          /* common.php:250-300: N+0, then V+k,V-k,N+k,N-k for k = 1..(nc>>1)+1, $n mutated */
#define DWPA_NC_HASHCAT 1      /* hashcat --nonce-error-corrections=N: N+0, then +-k, k = 1..N, message_pair bits
                                  0x10 (no NC), 0x20 (LE only), 0x40 (BE only) honoured (third-party semantics)   */
#define DWPA_NC_MAX 65664      /* the largest nc / nonce_error_corrections taken (PHP mode: 131,333 attempts per key).
                                  Every reference call site fits, nets.nc being a smallint (db/wpa.sql:165):
                                  common.php:919 passes |nc| * 2 + 128 <= 65,664, :606 (|nc| << 1) + 1 <= 65,537.  A
                                  larger one on an EAPOL line is DWPA_E_ARG for that job (the PHP wrapper then runs
                                  the original check_key_m22000 if it is kept, else throws); dwpa_scan_create /
                                  dwpa_crack_files refuse it.                                                      */

typedef struct {
    const uint8_t *ptr;        /* NULL = PHP null key (skipped, common.php:172,240) */
    size_t len;
} dwpa_bytes;

typedef struct {
    int32_t key_index;         /* index into keys[] of the first matching key (input order), -1 if none    */
    int32_t nc;                /* nonce correction (DB column nets.nc); valid when nc_valid                */
    int8_t endian;             /* 0 = Null, 1 = 'BE', 2 = 'LE'  (DB column nets.endian)                    */
    uint8_t nc_valid;          /* 0 = PHP Null (PMKID lines), 1 = integer                                  */
    uint8_t reserved[2];
    uint8_t pmk[32];           /* PMK used for the hit (DB column nets.pmk)                                */
} dwpa_result;

typedef struct {
    const char *line;          /* one m22000 hashline (WPA*01*... / WPA*02*...), not NUL-terminated needed  */
    size_t line_len;
    const dwpa_bytes *keys;
    size_t nkeys;
    const uint8_t *pmk;        /* NULL, or 32 bytes used for the first non-null key (common.php:157,178)    */
    int32_t nc;                /* PHP $nc (default 128)                                                    */
} dwpa_job;

typedef struct {
    uint32_t struct_size;      /* sizeof(dwpa_config) */
    uint32_t device_mask;      /* bit d = use device d; 0 = all visible devices */
    uint32_t batch;            /* candidate slots per device per launch; 0 = auto */
    int32_t nc_mode;           /* DWPA_NC_PHP or DWPA_NC_HASHCAT (crack_files default: HASHCAT) */
    int32_t rule_mode;         /* DWPA_RULES_DEFAULT (0) / _HASHCAT / _FULL (ABI 3; was reserved[0]) */
    int32_t allow_cpu_fallback; /* ABI 4 (was reserved[1]), dwpa_init only: 1 = without a usable device, or after a
                                  device call failed (DWPA_E_NODEV / _HIP / _NOMEM / _OVERFLOW), check and PBKDF2
                                  calls run on the host backend; -1 = never; 0 = DWPA_CPU_FALLBACK=1 from the
                                  environment, else never.  With it on, dwpa_init returns 0 without probing for a
                                  device: the first call that needs one probes (a process whose calls all stay on the
                                  host backend never starts the HIP runtime) */
    int32_t host_max_pmks;     /* ABI 4 (was reserved[2]), dwpa_init only: a check call with at least one PBKDF2 derive
                                  and at most this many PMK-equivalents (derives + nonce-correction verify work /
                                  16,388 compressions) runs on the host backend, a dwpa_pbkdf2_pmk call of at most this
                                  many keys too; -1 = never (every call on the device); 0 = DWPA_HOST_MAX_PMKS from
                                  the environment (<= 0: never), else the PMKs the library's host pool derives in
                                  2 ms on this CPU (measured at first use; ~460 on 16 threads of an EPYC 9575F, at
                                  least 8).  Until the process's first device call
                                  completes the threshold is 8x this: that call also starts the HIP runtime (0.2-0.7 s
                                  in a fresh PHP-FPM worker) */
    int32_t reserved[1];
} dwpa_config;

typedef struct {
    uint64_t cand;             /* candidate id: dictionary word index, numeric value / mask index, word*nrules+rule */
    uint32_t line;             /* index of the hashline in the scan's line array */
    int32_t nc;
    int8_t endian;
    uint8_t nc_valid;
    uint8_t reserved[2];
    uint8_t pmk[32];
} dwpa_hit;

/* ---- library ------------------------------------------------------------------------------------------------ */
int dwpa_abi_version(void);
/* Optional: select devices / batch size for the whole process (check path, PBKDF2 and scan calls that follow).
 * Lazy and idempotent; every entry point initialises on first use.  dwpa_crack_files' own cfg applies to that call
 * only and leaves this selection unchanged. */
int dwpa_init(const dwpa_config *cfg);
int dwpa_device_count(void);
const char *dwpa_strerror(int code);
void dwpa_shutdown(void);

/* ---- server-side check: PHP FFI replacement of check_key_m22000 (web/common.php:157-307) -------------------- */
/* Returns DWPA_HIT and fills *out, DWPA_MISS, or a negative code (php/dwpa22000.php: MISS and -1..-4 -> False,
 * codes <= -10 -> the original PHP check_key_m22000, never False). */
int dwpa_check_m22000(const char *line, size_t line_len, const dwpa_bytes *keys, size_t nkeys,
                      const uint8_t *pmk /* nullable, 32 bytes */, int nc, dwpa_result *out);
/* Bulk form (put_work's per-candidate loop, rkg.php's per-net loop): jobs grouped by ESSID internally so
 * each (ESSID, key) PMK is derived once.  rcs[i] / out[i] as for dwpa_check_m22000.  Returns 0 or a
 * negative code if the whole batch failed (device error). */
int dwpa_check_batch(const dwpa_job *jobs, size_t njobs, dwpa_result *out, int *rcs);
/* What the calling thread's last dwpa_check_m22000 / dwpa_check_batch call did (ABI 3): which backend answered it
 * (ABI 4), its jobs, the non-null keys of usable lines (slots), the (ESSID, key) PMKs derived after deduplication (on
 * the host backend: by it; the tail fields below stay 0 there), how many of those formed the device call's tail
 * (the remainder under one wave per SIMD: derived by the host backend beside the head when it fits the head's time,
 * tail_waves 0; else by a tail launch beside the head at low wave priority), the tail launch's waves and how many of
 * them saw the head end and raised their priority, the hits, and the call's wall time.
 * Returns 0, or DWPA_E_ARG before any check call in this thread. */
typedef struct {
    uint32_t jobs;
    uint32_t slots;
    uint32_t pmks;
    uint32_t tail_pmks;
    uint32_t tail_waves;
    uint32_t tail_waves_raised;
    uint32_t hits;
    uint32_t backend;          /* ABI 4: DWPA_BACKEND_* -- who answered the call */
    double seconds;
} dwpa_check_stats;
#define DWPA_BACKEND_DEVICE 0         /* the gfx950 device                                                    */
#define DWPA_BACKEND_HOST_SMALL 1     /* the host backend: a small call (dwpa_config.host_max_pmks)           */
#define DWPA_BACKEND_HOST_FALLBACK 2  /* the host backend: no usable device / a failed device call, with
                                         allow_cpu_fallback on                                               */
int dwpa_check_last_stats(dwpa_check_stats *out);
/* What this process's copy of the library holds right now (ABI 3; host only, never initialises a device): device
 * buffers and pinned host memory of every call context, scan and crack call, the host pool's worker threads (grown
 * on demand up to DWPA_HOST_THREADS - 1), and the call contexts (devices x DWPA_CALLS_PER_DEVICE) and how many of them
 * have run a call.  For sizing PHP-FPM pools, where every worker process loads its own copy. */
typedef struct {
    uint64_t device_bytes;
    uint64_t pinned_host_bytes;
    uint32_t host_pool_threads;
    uint32_t devices;
    uint32_t call_contexts;
    uint32_t call_contexts_used;
} dwpa_resources;
int dwpa_resource_stats(dwpa_resources *out);

/* ---- primitives exposed for parity tests and wrappers ------------------------------------------------------ */
/* PMK = PBKDF2-HMAC-SHA1(key, essid, 4096, 32) for every key (raw bytes, no $HEX[] decoding; a NULL key derives as
 * the empty key).  At most host_max_pmks keys: on the host backend, as the check path routes. */
int dwpa_pbkdf2_pmk(const dwpa_bytes *keys, size_t nkeys, const uint8_t *essid, size_t essid_len,
                    uint8_t *pmks_out /* nkeys * 32 */);
/* hashcat $HEX[...] decoding as web/common.php:3-25; *out_len <= in_len. */
int dwpa_hc_unhex(const uint8_t *in, size_t in_len, uint8_t *out, size_t *out_len);
/* Parse one hashline with check_key_m22000's acceptance rules (common.php:157-237) and describe the nonce-
 * correction attempt lists the verifier would run for `nc` (host only, no device needed).  Returns 0 or the
 * negative parse code.  essid holds the first min(essid_len, 32) bytes of the decoded ESSID and essid_len its full
 * length: PHP accepts longer ESSIDs (any even-length hex, common.php:28-36) and the check uses all of them; only
 * this description is cut.  mac_ap / mac_sta likewise hold the first 16 bytes. */
typedef struct {
    int32_t type;              /* 1 PMKID, 2 EAPOL */
    int32_t keyver;            /* EAPOL key version (0 if unknown) */
    uint32_t essid_len, mac_ap_len, mac_sta_len, target_len;
    uint32_t attempts;         /* attempts per key (1 + 4*((nc>>1)+1) in PHP mode) */
    uint32_t lists;            /* distinct attempt lists (> 1 only when PHP's $n grows, short ANONCE) */
    uint32_t never_matches;    /* PMKID/MIC shorter than 16 bytes */
    uint8_t essid[32];
    uint8_t mac_ap[16], mac_sta[16];
    uint8_t hash_m22000[16];   /* common.php:310-315 dedupe key */
} dwpa_line_info;
int dwpa_parse_m22000(const char *line, size_t line_len, int nc, int nc_mode, dwpa_line_info *out);
/* md5 over fields 1..7 (common.php:310-315); DWPA_E_FORMAT if the line has != 9 fields. */
int dwpa_hash_m22000(const char *line, size_t line_len, uint8_t out[16]);

/* ---- client-side: ctypes replacement of run_cracker() (help_crack.py:765-802) ------------------------------ */
/* Reads hash_file (one m22000 line per line), the dictionaries (plain text or .gz, one word per line, $HEX[]
 * decoded), applies rules_file (hashcat rule syntax, may be NULL) and writes one outfile record per cracked line:
 *   <PMKID|MIC hex>:<MAC_AP hex>:<MAC_STA hex>:<ESSID>:<PSK>   (ESSID/PSK as $HEX[..] when not printable)
 * Returns a hashcat exit code (DWPA_RC_*).  nonce_error_corrections as --nonce-error-corrections.  cfg (nullable):
 * device_mask / batch / nc_mode for this call only (device_mask 0 = the dwpa_init selection, default all devices);
 * a field beyond cfg->struct_size keeps its default (0 = the whole current struct).
 * Lines that can never match (PMKID or MIC shorter than 16 bytes, which hashcat does not load) do not count
 * towards "every hashline cracked".  DWPA_CRACK_SHARDS_PER_DEVICE=k runs k shard workers per device. */
int dwpa_crack_files(const char *hash_file, const char *const *dicts, size_t ndicts, const char *rules_file,
                     int nonce_error_corrections, const char *out_file, const dwpa_config *cfg);
/* dwpa_crack_files plus one outcome per dictionary (dict_status[ndicts], nullable):
 *   DWPA_DICT_OK       read to its end (or not needed: every line cracked first)
 *   DWPA_DICT_DAMAGED  corrupt or truncated gzip stream, by zlib's own verdict: scanned up to the damage, and the
 *                      call still returns 0/1 (hashcat reads wordlists through gzread and does the same).  For a
 *                      truncated stream the words are exactly those of the bytes gzread delivers; for a corrupt body
 *                      or CRC they are at least those (the parallel decoder may deliver the bytes before the failing
 *                      check, and how much gzread drops depends on its buffer and read sizes).  The file should be
 *                      fetched again (help_crack.py:530-534 only downloads a missing file)
 *   DWPA_E_IO          cannot be opened or read: the call returns DWPA_RC_ERROR (before any device work when the
 *                      file cannot be opened, as hashcat refuses to start) */
#define DWPA_DICT_OK 0
#define DWPA_DICT_DAMAGED 1
int dwpa_crack_files_ex(const char *hash_file, const char *const *dicts, size_t ndicts, const char *rules_file,
                        int nonce_error_corrections, const char *out_file, const dwpa_config *cfg,
                        int32_t *dict_status);
/* What the calling thread's last dwpa_crack_files(_ex) call did, for a hashcat-style end-of-run summary
 * (help_crack shows hashcat's output, help_crack.py:776): dictionary words read, candidates derived (inside the
 * 8..63 filter, after the rules), hashlines loaded and cracked, wall time, and the rules file's rules loaded and
 * skipped (a line that does not parse is skipped with a stderr message, as hashcat's "Skipping invalid or
 * unsupported rule"; 0 / 0 without a rules file).  Returns 0, or DWPA_E_ARG before any call in this thread. */
typedef struct {
    uint64_t words;
    uint64_t candidates;
    uint32_t hashes;
    uint32_t cracked;
    double seconds;
    uint32_t rules;            /* rules loaded from rules_file (ABI 2) */
    uint32_t rules_skipped;    /* rule lines of rules_file skipped: not parsing, or (DWPA_RULES_HASHCAT) using reject /
                                  memory functions (ABI 2) */
    uint32_t rules_rejmem;     /* of rules_skipped, the lines skipped for reject / memory functions (ABI 3) */
    uint32_t reserved;
} dwpa_crack_stats;
int dwpa_crack_last_stats(dwpa_crack_stats *out);
/* Per shard worker of the calling thread's last dwpa_crack_files(_ex) call (ABI 4): one worker per selected device
 * (DWPA_CRACK_SHARDS_PER_DEVICE per device), each a stager thread uploading work items and a scanner thread running
 * them.  wait_s is the scanner's time waiting for a staged item (the shared dictionary feed not keeping up), scan_s its
 * time scanning.  Copies min(cap, workers) entries, sets *n = workers; returns 0, or DWPA_E_ARG before any call. */
typedef struct {
    int32_t device;
    uint32_t items;            /* work items (contiguous word ranges of the shared feed) scanned */
    uint64_t words;            /* dictionary words of those items */
    uint64_t candidates;       /* candidates derived (after the rules, inside the 8..63 filter) */
    double wait_s;
    double scan_s;
} dwpa_crack_worker;
int dwpa_crack_worker_stats(dwpa_crack_worker *out, size_t cap, size_t *n);

/* ---- mask attack: hashcat -a 3 ------------------------------------------------------------------------------
 * The mask language is hashcat's: ?l a-z, ?u A-Z, ?d 0-9, ?h 0-9a-f, ?H 0-9A-F, ?s the 33 ASCII specials in byte
 * order (0x20-0x2f, 0x3a-0x40, 0x5b-0x60, 0x7b-0x7e), ?a = ?l?u?d?s (95 bytes), ?b 0x00-0xff, ?? a literal '?',
 * ?1..?4 the custom sets, any other byte a literal (a position of radix 1).  1..63 positions (63: m22000's longest
 * PSK).  custom[k] is set ?(k+1) as raw bytes in the same language (so no --hex-charset is needed): built-in
 * references, references to lower-numbered custom sets, ?? and literal bytes; duplicate bytes are dropped, the
 * first occurrence kept, as hashcat does; ptr == NULL = undefined (custom itself may be NULL: none defined).
 * Keyspace K = the product of the positions' set sizes, at most 2^64 - 1.
 * Order -- this library's own: candidate i is the mixed-radix numeral of i with the LAST position fastest, i.e.
 * Python's itertools.product order, and ?d x N at index v is dwpa_scan_load_numeric's candidate v.  Parity with
 * hashcat is unpinned: hashcat walks a mask in Markov order, so its index i (and its --skip / --limit windows) names
 * another candidate; the candidate SET of a mask is the same.
 * DWPA_E_ARG: ?x with an unknown letter, a trailing lone '?', a reference to an undefined custom set (inside a custom
 * set: to one not lower-numbered), an empty set, no position or more than 63, K above 2^64 - 1. */
/* Host only (work without a device): positions and keyspace of a mask (either out pointer may be NULL) ... */
int dwpa_mask_keyspace(const char *mask, size_t mask_len, const dwpa_bytes custom[4], uint32_t *positions,
                       uint64_t *keyspace);
/* ... and candidate `index` (< K, else DWPA_E_ARG): *out_len bytes in out, the rest of the 64 zeroed. */
int dwpa_mask_candidate(const char *mask, size_t mask_len, const dwpa_bytes custom[4], uint64_t index,
                        uint8_t out[64], uint32_t *out_len);
/* hashcat -m 22000 -a 3 hash_file mask [-1..-4 custom] [-s skip -l limit | -i --increment-min --increment-max] -o
 * out_file: dwpa_crack_files' hash file, outfile records (the PSK rebuilt on the host from the hit's index), return
 * codes (DWPA_RC_*), nonce_error_corrections and cfg handling (nc_mode default hashcat).  mask is NUL-terminated.
 * skip / limit select the indices [skip, skip + limit) of [0, K) in this library's order (limit 0 = to the end);
 * skip >= K is DWPA_RC_ERROR, as hashcat refuses it.  increment_min / increment_max: 0 / 0 = off, else the call runs
 * the mask's prefixes of increment_min..increment_max positions (clipped to the mask; a 0 bound = open), shortest
 * first; combined with skip / limit it is DWPA_RC_ERROR, as in hashcat.  A mask length outside 8..63 is skipped with
 * one stderr line, as hashcat skips it; nothing left to run is DWPA_RC_ERROR.
 * Runs on every selected device (cfg->device_mask), DWPA_CRACK_SHARDS_PER_DEVICE workers per device: all workers take
 * batch-sized ascending index ranges from one shared cursor and generate them on their device.
 * dwpa_crack_last_stats afterwards: words 0, candidates as derived; dwpa_crack_worker_stats: one entry per worker
 * (items = batches, words and wait_s 0).  Without a device: DWPA_RC_ERROR. */
int dwpa_crack_mask(const char *hash_file, const char *mask, const dwpa_bytes custom[4], uint64_t skip, uint64_t limit,
                    uint32_t increment_min, uint32_t increment_max, int nonce_error_corrections, const char *out_file,
                    const dwpa_config *cfg);

/* ---- mask attack in Markov order with a per-position threshold: hashcat -a 3 [-t N] ---------------------------
 * (Added without a new ABI version, discoverable by symbol.)
 * Model: position-dependent, first order, over bytes, positions 0..62.  n[p][a][b] = the training words whose byte
 * at position p is b and whose byte at position p - 1 is a (the predecessor of position 0 is byte 0); order[p][a] =
 * the 256 byte values by n[p][a][b] descending, ties by byte value ascending, so an unseen byte ranks after every
 * seen one, in byte order.  A model file (DWPA_MARKOV_BYTES bytes) holds the ranking, not the counts: the 8 bytes
 * "DWPAMKV1", u32 LE 63, u32 LE 0, then order as 63 x 256 rows of 256 bytes.  A model image is such a file in memory;
 * every call that takes one refuses (DWPA_E_ARG) another size, another header, or a row that is no permutation of
 * 0..255.  There are no built-in statistics, and hashcat's own statistics file (hashcat.hcstat2) is not read.
 * Keyspace: for the mask's sets S_p (sizes n_p) and a threshold t (0 = none, else 1..256; above: DWPA_E_ARG), r_p =
 * n_p (t = 0) or min(n_p, t) and K = the product of the r_p, at most 2^64 - 1 (the un-thresholded mask's keyspace
 * may be larger).  K needs no model.
 * Order -- this library's own: the digits d_p of candidate i over the radices r_p, LAST position fastest; bytes c_0 =
 * row(0, 0)[d_0], c_p = row(p, c_{p-1})[d_p], where row(p, a) is order[p][a] filtered to the members of S_p, its
 * first r_p entries.  A literal is a position of radix 1: its own byte whatever the model says, and the predecessor
 * of the next position.  Distinct indices give distinct candidates; with t = 0 the candidate set is the plain mask's,
 * with t > 0 a subset of it.  Parity of the index with hashcat's Markov order is unpinned. */
#define DWPA_MARKOV_BYTES 4128784
/* Host only.  Trains a model from word lists read as every attack reads them (plain or gzip, "\n" or "\r\n", $HEX[]
 * decoded), several lists counting as their concatenation; a word contributes its first 63 bytes, an empty line
 * nothing.  Writes out_file and stores the number of contributing words in *words (nullable).  DWPA_E_IO: a list
 * that cannot be read or a damaged gzip stream (counted up to the damage, no file written), out_file not writable. */
int dwpa_markov_train(const char *const *dicts, size_t ndicts, const char *out_file, uint64_t *words);
/* Host only.  The model file at path, validated, into out (cap >= DWPA_MARKOV_BYTES).  DWPA_E_IO: unreadable;
 * DWPA_E_ARG: not a model file.  dwpa_markov_check validates an image in memory. */
int dwpa_markov_load(const char *path, uint8_t *out, size_t cap);
int dwpa_markov_check(const uint8_t *model, size_t model_len);
/* Host only: dwpa_mask_keyspace / dwpa_mask_candidate under a threshold and a model image.
 * dwpa_mask_candidates_markov: n indices at once (the image is validated once), out = n x 64 bytes. */
int dwpa_mask_keyspace_markov(const char *mask, size_t mask_len, const dwpa_bytes custom[4], uint32_t threshold,
                              uint32_t *positions, uint64_t *keyspace);
int dwpa_mask_candidate_markov(const char *mask, size_t mask_len, const dwpa_bytes custom[4], const uint8_t *model,
                               size_t model_len, uint32_t threshold, uint64_t index, uint8_t out[64],
                               uint32_t *out_len);
int dwpa_mask_candidates_markov(const char *mask, size_t mask_len, const dwpa_bytes custom[4], const uint8_t *model,
                                size_t model_len, uint32_t threshold, const uint64_t *indices, size_t n,
                                uint8_t *out, uint32_t *out_len);
/* dwpa_crack_mask in Markov order: markov_file is a model file, skip / limit index the thresholded keyspace, and
 * with increment one model serves every prefix.  A missing or damaged model file, or a threshold above 256, is
 * DWPA_RC_ERROR before any device is touched.  In every other respect dwpa_crack_mask. */
int dwpa_crack_mask_markov(const char *hash_file, const char *mask, const dwpa_bytes custom[4],
                           const char *markov_file, uint32_t threshold, uint64_t skip, uint64_t limit,
                           uint32_t increment_min, uint32_t increment_max, int nonce_error_corrections,
                           const char *out_file, const dwpa_config *cfg);

/* ---- table attack: per-byte substitution tables, every combination (hashcat-legacy -a 5 --table-file) ----------
 * (Added without a new ABI version, discoverable by symbol.)
 * Table: for every byte value c a list alt[c] of 1..DWPA_TABLE_MAX_ALT distinct replacement bytes, in the order of the
 * text.  A byte the text never names as a key has alt[c] = [c]; a key keeps its original only if the text says so
 * ("a=a"), as in hashcat-legacy.  Text, strict: every non-empty line, after one trailing CR is removed, is K=V, K and
 * V each one literal byte or \xHH (so "===" maps '=' to '=' and "#=#" is a mapping, not a comment); a repeated (K, V)
 * line is ignored; any other line, a 17th alternative for one key, or a text without any mapping is DWPA_E_ARG.
 * Replacements are one byte each (multi-byte replacements are not supported), so a candidate has its word's length.
 * Filter: a word of L bytes is kept iff minlen <= L <= maxlen (maxlen is clamped to 63) and its count k_w = the
 * product of the alternative counts of its bytes is at most word_max (1..2^32 - 1; 0 means 2^32 - 1).  The product
 * saturates: a word of 2^64 combinations is dropped, never counted as 0 or 1.  Dropped words own no indices.
 * Order -- this library's own: kept words in list order, start[j] = the sum of the counts of the kept words before
 * word j, K = start[nkept] <= 2^64 - 1 (above: DWPA_E_ARG).  Candidate id belongs to the kept word j with start[j] <=
 * id < start[j + 1]; id - start[j] is the mixed-radix numeral over the word's positions, LAST position fastest
 * (itertools.product over the positions' alternative lists).  Parity of the index with hashcat-legacy is unpinned. */
#define DWPA_TABLE_MAX_ALT 16
#define DWPA_TABLE_IMAGE_BYTES 4352 /* u8 nalt[256], then u8 alt[256][16] */
/* Host only.  Parses a table text; image (nullable, DWPA_TABLE_IMAGE_BYTES) receives the table.  Returns the number of
 * mappings kept (>= 1), or DWPA_E_ARG with *bad_line (nullable) = the 1-based number of the line at fault (a text
 * without any mapping: its number of lines + 1). */
int dwpa_table_parse(const char *text, size_t len, uint8_t *image, uint32_t *bad_line);
/* Host only.  The text of a built-in table: "toggle" maps every ASCII letter to [itself, the other case] (hashcat
 * -a 2).  *len = its length; copied into out when cap suffices (out nullable: ask for the length).  DWPA_E_ARG: no
 * such table. */
int dwpa_table_builtin(const char *name, char *out, size_t cap, size_t *len);
/* Host only.  K, the number of kept words and the words dropped for their length and for word_max (all nullable) of
 * the list words[0..nwords) under the table text.  DWPA_E_ARG: an invalid table, nwords >= 2^32, K above 2^64 - 1. */
int dwpa_table_keyspace(const char *table_text, size_t table_len, const dwpa_bytes *words, size_t nwords,
                        uint32_t minlen, uint32_t maxlen, uint32_t word_max, uint64_t *keyspace, uint64_t *kept,
                        uint64_t *dropped_len, uint64_t *dropped_max);
/* Host only.  Candidates indices[0..n) in one call: out = n x 64 bytes (candidate k at out + 64 k, zero beyond its
 * length), out_len = n lengths.  DWPA_E_ARG also for an index >= K. */
int dwpa_table_candidates(const char *table_text, size_t table_len, const dwpa_bytes *words, size_t nwords,
                          uint32_t minlen, uint32_t maxlen, uint32_t word_max, const uint64_t *indices, size_t n,
                          uint8_t *out, uint32_t *out_len);
/* The table attack over hash_file, on every selected device: dwpa_crack_chain's hash file, outfile records, return
 * codes (DWPA_RC_*), nonce_error_corrections and cfg handling.  dict is one plain or gzip word list ($HEX[] words
 * decoded), read whole and held in device memory with the chain lists' limits; table_file holds the table text; the
 * filter is 8..63 bytes and word_max; skip / limit name the indices [skip, skip + limit) (limit 0 = to the end).  A
 * hit's PSK is rebuilt on the host from its index.  One stderr line states the words dropped for length and for
 * word_max.  DWPA_RC_ERROR before any device is touched, one stderr line each: an unreadable or invalid table, an
 * unreadable or oversized list, K above 2^64 - 1, skip >= K with K > 0, a missing hash file.  K = 0 exhausts. */
int dwpa_crack_table(const char *hash_file, const char *dict, const char *table_file, uint32_t word_max,
                     uint64_t skip, uint64_t limit, int nonce_error_corrections, const char *out_file,
                     const dwpa_config *cfg);

/* ---- association attack: every net against its own words (hashcat -a 9; web/rkg.php's per-net pass) -------------
 * Every other attack tries one candidate stream against every net of the hash file; this one tries each net's own
 * words against that net only.
 * Net.  The pair (ESSID bytes, MAC_AP bytes) of a usable hashline.  Nets are numbered by first appearance in the hash
 *   file; all usable lines with that pair belong to the net: PMKID and EAPOL of any keyver, any MAC_STA.
 * Entries.  A net's word list comes from its sources, in order: first the lines of the association file whose key is
 *   the net's MAC_AP, in file order; then, with DWPA_ASSOC_SINGLE, the built-in generator's words.  Within a net a word
 *   equal byte for byte to an earlier one is dropped (the first stays); a word of 0 bytes or more than 256 bytes is
 *   dropped.  W_n words are left; a net with W_n = 0 owns no indices.
 * Association file.  Read through the dictionary reader: plain or gzip, CRLF accepted.  Each line is MAC_AP:WORD --
 *   12 hex digits in either case, one ':', then the word; $HEX[...] is decoded for the WORD part only.  A line of
 *   another shape is skipped with one stderr line and counted (malformed); a line whose MAC matches no net is counted
 *   (unmatched) and skipped.  A MAC that occurs under two ESSIDs feeds both nets.
 * Single generator (after web/rkg.php:48-77).  From the BSSID as a 48-bit integer b (a MAC_AP of 6 bytes; another
 *   length gives no BSSID words): for i in -1, 0, +1 and j in 12, 10, 8 the last j hex digits of (b + i) mod 2^48,
 *   zero-padded to j, lowercase, then uppercase.  From the ESSID e: for each suffix in "", "1", "123", "!" c = e +
 *   suffix; c, then its ASCII uppercase if that differs, then its ASCII lowercase if that differs.  ESSID-derived
 *   words shorter than minlen are omitted: 8 without rules, 1 with rules (so that linksys + $1 is reachable).
 * Keyspace.  R = the number of loaded rules, 1 (the identity) without a rules file.  Net n owns W_n x R consecutive
 *   indices from start[n], rule-major with the word fastest: sub = id - start[n], rule = sub / W_n, word = sub % W_n.
 *   K = start[N]; K above 2^64 - 1 and W_n x R >= 2^32 are refused.  skip / limit name windows of these indices.
 * Candidate.  The rule applied to the word by the rule engine; a rules file loads as every -r file does.  A rejected
 *   result, or one outside 8..63 bytes, gives no candidate.
 * Association.  A candidate of net n is derived with net n's ESSID and verified against the not-yet-cracked lines of
 *   net n and against nothing else -- not against a line of another net with the same ESSID, though that line would
 *   accept the same PMK.  A net whose lines are all cracked, or can never match, yields no slots from then on; its
 *   indices stay in the keyspace.  Two nets that share an ESSID and a word derive that PMK twice, as hashcat -a 9. */
#define DWPA_ASSOC_SINGLE 1u /* flags: add the single generator's words to every net */
typedef struct {
    uint64_t keyspace;   /* K                                                              */
    uint64_t nets;       /* N                                                              */
    uint64_t entries;    /* the sum of W_n                                                 */
    uint64_t file_lines; /* lines of the association file                                  */
    uint64_t unmatched;  /* of them, well-formed lines whose MAC matches no net            */
    uint64_t malformed;  /* of them, lines that are not MAC_AP:WORD                        */
    uint64_t dropped;    /* words dropped: duplicates within a net, 0 bytes, above 256     */
    uint32_t rules;      /* R                                                              */
    uint32_t reserved;
} dwpa_assoc_info;
/* Host only.  The single generator's words for one hashline (its MAC_AP and ESSID), in order, duplicates included:
 * word k is lens[k] bytes, the words lie back to back in out.  *nwords and *nbytes (both required) always receive the
 * totals; DWPA_E_OVERFLOW when out_cap or lens_cap is too small (nothing is written).  A line that does not parse
 * returns its DWPA_E_* code. */
int dwpa_assoc_single(const char *line, size_t line_len, uint32_t minlen, uint8_t *out, size_t out_cap,
                      uint32_t *lens, size_t lens_cap, size_t *nwords, size_t *nbytes);
/* Host only; reads the hash file (the nets come from it) but needs no device.  assoc_file and rules_file are nullable;
 * at least one of assoc_file and DWPA_ASSOC_SINGLE is required.  DWPA_E_IO: a file cannot be read; DWPA_E_RULE: no rule
 * of rules_file loads; DWPA_E_ARG: no source, K above 2^64 - 1, a net with W_n x R >= 2^32. */
int dwpa_assoc_plan(const char *hash_file, const char *assoc_file, uint32_t flags, const char *rules_file,
                    dwpa_assoc_info *out);
/* Host only.  Candidates indices[0..n) of that plan: out = n x 64 bytes (candidate k at out + 64 k, zero beyond its
 * length), out_len[k] its length or 0xFFFFFFFF where the index gives no candidate (rejected, outside 8..63 bytes),
 * first_line[k] (nullable) the first input line of its net.  DWPA_E_ARG also for an index >= K. */
int dwpa_assoc_candidates(const char *hash_file, const char *assoc_file, uint32_t flags, const char *rules_file,
                          const uint64_t *indices, size_t n, uint8_t *out, uint32_t *out_len, uint32_t *first_line);
/* The association attack over hash_file, on every selected device: dwpa_crack_table's hash file, outfile records,
 * return codes (DWPA_RC_*), nonce_error_corrections and cfg handling; skip / limit name the indices [skip, skip +
 * limit) (limit 0 = to the end).  One stderr line states the nets, entries, unmatched and malformed counts.
 * DWPA_RC_ERROR before any device is touched, one stderr line each: no source, an unreadable association, rules or
 * hash file, no rule left, a refused keyspace, skip >= K with K > 0.  K = 0 exhausts. */
int dwpa_crack_assoc(const char *hash_file, const char *assoc_file /* nullable */, uint32_t flags,
                     const char *rules_file /* nullable */, uint64_t skip, uint64_t limit,
                     int nonce_error_corrections, const char *out_file, const dwpa_config *cfg);

/* ---- hybrid attacks: hashcat -a 6 (wordlist || mask) and -a 7 (mask || wordlist) ------------------------------
 * Candidate: mode 6 = word || m, mode 7 = m || word, m a candidate of the mask (the mask language above, 1..63
 * positions, keyspace K).
 * Order and id -- word-major, mask index fastest: id = word_index * K + mask_index, word_index indexing the words as
 * handed over (the d_offsets array of a scan load, as dwpa_scan_load_dict's ids do), mask_index in this library's own
 * mask order (last position fastest).  Parity with hashcat's order is unpinned, as for -a 3; the candidate set is
 * the same.
 * Filter: a word of L bytes with a mask of P positions is kept iff minlen <= L + P <= maxlen (the crack call uses
 * 8..63; a scan load treats maxlen above 64 as 64, one HMAC key block).  All K candidates of a word are kept or
 * dropped together.  An empty word is an ordinary word, kept when P >= minlen (parity with hashcat for empty lines is
 * unpinned).  Words longer than 63 bytes always drop.  Dropped words leave no slots. */
#define DWPA_HYBRID_WORD_MASK 6
#define DWPA_HYBRID_MASK_WORD 7
/* hashcat -m 22000 -a 6 hash_file dicts... mask / -a 7 hash_file mask dicts... [-1..-4 custom] -o out_file, with
 * everything dwpa_crack_files_ex does for a dictionary run: hash file, outfile records (the PSK rebuilt on the host
 * from the word and the mask index), return codes, nonce_error_corrections, cfg (nc_mode default hashcat), plain or
 * gzip dictionaries with $HEX[] words, dict_status (nullable, one per dictionary), every selected device with
 * DWPA_CRACK_SHARDS_PER_DEVICE workers each, stop when every line is cracked.  mask is NUL-terminated; mode is
 * DWPA_HYBRID_WORD_MASK or DWPA_HYBRID_MASK_WORD.  K <= batch: a launch holds whole words x the whole mask; K > batch:
 * one word x consecutive mask ranges of `batch` (a word the filter drops costs no launch).
 * DWPA_RC_ERROR before any device is touched: an invalid mask, an unknown mode, an unreadable dictionary (its
 * dict_status is DWPA_E_IO, whatever else is wrong with the call).  A mask that no word can complete to 8..63
 * characters (P > 63 cannot be written; P = 63 keeps only empty words) simply exhausts.
 * dwpa_crack_last_stats afterwards: words = words read, candidates = kept words x K derived;
 * dwpa_crack_worker_stats as for dwpa_crack_files. */
int dwpa_crack_hybrid(const char *hash_file, const char *const *dicts, size_t ndicts, const char *mask,
                      const dwpa_bytes custom[4], int mode, int nonce_error_corrections, const char *out_file,
                      const dwpa_config *cfg, int32_t *dict_status /* nullable */);

/* ---- combinator attack: hashcat -a 1 (word of one list || word of another) -------------------------------------
 * Candidate: left || right, left a word of the first list and right a word of the second, as `hashcat -a 1 left
 * right` joins them.
 * Amplifier and base -- the amplifier list is held whole in device memory, the base list is streamed through the
 * dictionary feed.  DWPA_COMBI_AMP_RIGHT (the default): the right list is the amplifier.  DWPA_COMBI_AMP_LEFT: the left
 * list is the amplifier, for a right list too big to hold.  The side changes which list is resident and the order of
 * the candidates, never the join: it is always left || right.
 * Order and id -- base-major, amplifier index fastest: id = base_index * A + amp_index.  A is the amplifier's word
 * count as read: every line counts, empty and overlong ones included, so an index names a line.  Parity with
 * hashcat's order is unpinned, as for -a 3 / 6 / 7; the candidate set is the same.
 * Filter: a pair is kept iff both words are <= 63 bytes and minlen <= L + R <= maxlen (the crack call uses 8..63; a
 * scan load treats maxlen above 64 as 64, one HMAC key block).  The decision is per pair.  An empty word is an
 * ordinary word.  Dropped pairs leave no slots.  Two different pairs can be the same string (a || bc, ab || c): both
 * are candidates with their own ids, and the crack call reports a line once, lowest id first. */
#define DWPA_COMBI_AMP_RIGHT 0
#define DWPA_COMBI_AMP_LEFT  1
/* The amplifier list of dwpa_crack_combinator: fewer than 2^32 words, and decoded text plus 8-byte offsets of at most
 * this many bytes (it is held once on the host and once per worker on its device). */
#define DWPA_COMBI_AMP_MAX_BYTES (1ull << 30)
/* hashcat -m 22000 -a 1 hash_file left_dict right_dict -o out_file, with everything dwpa_crack_hybrid does, the
 * amplifier list standing where the mask does: hash file, outfile records (the PSK rebuilt on the host from the two
 * words), return codes, nonce_error_corrections, cfg, plain or gzip lists with $HEX[] words and CRLF, every selected
 * device with DWPA_CRACK_SHARDS_PER_DEVICE workers each, cross-worker retirement, stop when every line is cracked.
 * The amplifier list (amp_side: DWPA_COMBI_AMP_RIGHT or DWPA_COMBI_AMP_LEFT) is read whole into host memory once and
 * uploaded once per worker; the base list is streamed.  Loads are sized from the two lists' lengths, not by trial:
 * A <= batch: a launch holds whole base words x the whole amplifier, as many as fill the batch exactly; A > batch: one
 * base word x consecutive amplifier ranges of `batch` (a range that keeps no pair costs no launch).
 * DWPA_RC_ERROR before any device is touched: an unknown amp_side, a missing hash file, an unreadable list (its
 * dict_status entry is DWPA_E_IO, whatever else is wrong with the call), an amplifier list above the limit
 * (DWPA_COMBI_AMP_MAX_BYTES or 2^32 - 1 words: the message names the other amp_side).
 * dict_status (nullable): [0] the left list, [1] the right list.
 * dwpa_crack_last_stats afterwards: words = base words read, candidates = kept pairs derived (for an exhausted run the
 * exact count that follows from the two lists' lengths); dwpa_crack_worker_stats as for dwpa_crack_files. */
int dwpa_crack_combinator(const char *hash_file, const char *left_dict, const char *right_dict, int amp_side,
                          int nonce_error_corrections, const char *out_file, const dwpa_config *cfg,
                          int32_t dict_status[2] /* nullable: left, right */);

/* ---- chain attack: up to four word lists and masks joined left to right ------------------------------------------
 * A chain is 1..DWPA_CHAIN_MAX_PARTS parts; each part is a word list held whole in device memory or a mask (the mask
 * language above, 1..63 positions); a candidate is one choice of every part, concatenated in the order of the parts.
 * It generalises the mask attack (one mask part), the hybrid attacks (list + mask, mask + list) and the combinator
 * attack (list + list).  The custom sets ?1..?4 are shared by all mask parts of a chain.
 * Radix and keyspace -- part p has N_p choices: a list's word count as read (every line counts, empty and overlong
 * ones included, so an index names a line; N_p < 2^32, and text plus 8-byte offsets of at most
 * DWPA_COMBI_AMP_MAX_BYTES per list), a mask's keyspace.  K = the product of the N_p, at most 2^64 - 1.  A part with
 * N_p = 0 gives K = 0, which simply exhausts.
 * Order and id -- candidate i is the mixed-radix numeral of i over the parts' radices with the LAST part fastest
 * (itertools.product order); a mask part's own index is in this library's mask order.  Candidate id = i.  Parity with
 * any hashcat order is unpinned, as for the other attacks.
 * Filter: a candidate is kept iff every list word in it is <= 63 bytes and minlen <= total length <= maxlen (the
 * crack call uses 8..63; a scan load treats maxlen above 64 as 64, one HMAC key block).  The decision is per
 * candidate.  An empty word is an ordinary word.  Dropped candidates leave no slots.  Two ids can be the same string;
 * both are candidates, and the crack call reports a line once, lowest id first.
 * Rules on list parts (dwpa_scan_set_chain_rules, dwpa_crack_chain_rules) -- a list part may carry a rule set of
 * R >= 1 parsed rules.  Its choices are then the (rule, word) pairs: N_p = nwords * R, which must stay below 2^32,
 * ordered RULE-MAJOR with the word fastest: choice c = rule * nwords + word.  (This is not the word * nrules + rule id
 * of the word list x rules attack: with the word fastest, 64 consecutive indices share one rule, or two at a wrap,
 * whenever nwords >= 64, so the GPU's rule dispatch stays uniform across a wave.)  The piece is rule(word) by the
 * interpreter of "hashcat rules" below: the input word is rejected at 0 bytes or above 256, reject and memory
 * functions work as there, and a rejected choice drops the candidate.  A result of 0 bytes is an ordinary empty piece.
 * For a ruled part the "<= 63 bytes" test applies to the RESULT: a 100-byte word under '8 is legal, a 40-byte word
 * under d drops.  Un-ruled parts of the same chain are unchanged (an empty word is ordinary, a raw length above 63
 * drops), and so are the order of the parts, id = raw index, the filter and K <= 2^64 - 1.  Rules *files* load under
 * the process's rule mode as dwpa_crack_files' do (hashcat's -r loader unless DWPA_RULES_FULL), rule *text* takes the
 * whole language; lines that do not parse are skipped with one stderr line each, a set with no valid rule is an error.
 * Left out: streaming a list too big to hold, rules on mask parts or over the whole joined candidate, increment, and
 * filling a batch from several raw ranges -- a load is `batch` raw indices, so a chain whose filter drops most
 * candidates runs short launches. */
#define DWPA_CHAIN_LIST 0
#define DWPA_CHAIN_MASK 1
#define DWPA_CHAIN_MAX_PARTS 4
/* Host only, no device.  dwpa_chain_keyspace: *keyspace = the product of radix[0..nparts) (0 if any radix is 0);
 * DWPA_E_ARG: nparts outside 1..4, the product above 2^64 - 1.  dwpa_chain_split: digits[p] = the digit of `index`
 * at part p (a list's word index, a mask part's own index), last part fastest; DWPA_E_ARG also for index >= K. */
int dwpa_chain_keyspace(const uint64_t *radix, uint32_t nparts, uint64_t *keyspace);
int dwpa_chain_split(const uint64_t *radix, uint32_t nparts, uint64_t index, uint64_t *digits);
/* One part of dwpa_crack_chain.  DWPA_CHAIN_LIST: text is the path of a plain or gzip word list ($HEX[] words and
 * CRLF as everywhere).  DWPA_CHAIN_MASK: text is a NUL-terminated mask. */
typedef struct {
    int kind;
    const char *text;
} dwpa_chain_spec;
/* The chain over an m22000 hash file, with dwpa_crack_mask's hash file, rc convention, outfile records (the PSK
 * rebuilt on the host from the id), nc-mode default and cfg handling.  Every list is read whole once, kept on the
 * host and uploaded once per worker.  The workers (DWPA_CRACK_SHARDS_PER_DEVICE per selected device) take
 * batch-sized ascending ranges of the raw indices [skip, skip + limit) (limit 0: to the end) from one shared cursor;
 * lines cracked anywhere are retired on every worker, and the run stops when every line is cracked.
 * DWPA_RC_ERROR before any device is touched: nparts outside 1..4, an unknown kind, an invalid mask, an unreadable
 * list (its part_status entry is DWPA_E_IO), a list above the limits, K above 2^64 - 1, a missing hash file,
 * skip >= K with K > 0.  part_status (nullable, nparts entries): DWPA_DICT_OK, DWPA_DICT_DAMAGED or DWPA_E_IO for a
 * list, DWPA_DICT_OK for a mask.
 * dwpa_crack_last_stats afterwards: words = the sum of the lists' word counts, candidates = kept candidates derived;
 * dwpa_crack_worker_stats as for dwpa_crack_mask. */
int dwpa_crack_chain(const char *hash_file, const dwpa_chain_spec *parts, uint32_t nparts, const dwpa_bytes custom[4],
                     uint64_t skip, uint64_t limit, int nonce_error_corrections, const char *out_file,
                     const dwpa_config *cfg, int32_t *part_status /* nullable, nparts entries */);
/* dwpa_crack_chain with rules on list parts ("Rules on list parts" above).  part_rules: nparts entries, each NULL
 * (no rules) or the path of a rules file for that part; part_rules == NULL or every entry NULL is dwpa_crack_chain.
 * A hit's PSK is rebuilt on the host from its id: the digits, a ruled part's digit split into (rule, word), the rule
 * applied by the interpreter the GPU runs.  DWPA_RC_ERROR before any device is touched, besides dwpa_crack_chain's
 * reasons: an unreadable rules file, a rules file with no valid rule, rules on a mask part, nwords * R >= 2^32.
 * dwpa_crack_last_stats afterwards: rules, rules_skipped and rules_rejmem are sums over the parts; candidates = kept
 * candidates derived. */
int dwpa_crack_chain_rules(const char *hash_file, const dwpa_chain_spec *parts, uint32_t nparts,
                           const char *const *part_rules /* nullable; nparts entries, NULL = no rules */,
                           const dwpa_bytes custom[4], uint64_t skip, uint64_t limit, int nonce_error_corrections,
                           const char *out_file, const dwpa_config *cfg,
                           int32_t *part_status /* nullable, nparts entries */);

/* hashcat rules (the whole rule language of hashcat >= 6.2.6: every mangling, reject and memory function; one
 * rule per line, '#' comments; semantics in dwpa_amd/csrc/rules.hpp and oracle/rules.py).  The text entry points
 * below (dwpa_rules_expand, dwpa_rules_apply_host, dwpa_rules_count, dwpa_scan_set_rules) are the interpreter and
 * take every function; the rules *files* of dwpa_crack_files and dwpa_rules_expand_file go through hashcat's -r
 * loader rule unless DWPA_RULES_FULL (dwpa_config.rule_mode / dwpa_init / DWPA_RULE_MODE=full) is selected.
 * GPU rule application (replaces `hashcat --stdout -r rules words`, help_crack.py:508,575): out holds
 * nwords*nrules candidates of 256 bytes (word-major), out_len their lengths (0xFFFFFFFF = the input word or a
 * reject / memory function rejected it).  With out == NULL only *nrules_out is set (number of rules that parse).
 * Rule lines that do not parse are skipped with a stderr message each (out != NULL). */
int dwpa_rules_expand(int device, const char *rules_text, size_t rules_len, const dwpa_bytes *words, size_t nwords,
                      uint8_t *out, uint32_t *out_len, uint32_t *nrules_out);
/* `hashcat --stdout -r rules_file sources... -o out_path` (help_crack.py:508 expandcracked, :575 prdict): every word of
 * the sources (plain or gzip, one per line, $HEX[] decoded) x every rule of rules_file (loaded under the process's
 * rule mode, DWPA_RULES_HASHCAT unless dwpa_init / DWPA_RULE_MODE chose full), expanded on `device`, written to
 * out_path one candidate per line in word-major order, rejected candidates skipped, raw bytes as hashcat's --stdout
 * writes them -- except a candidate holding '\n' or '\r', which would not survive as one line and is written as
 * $HEX[..] (the dictionary readers decode it; hashcat would have split it); gzip_level 0 = plain text (what hashcat
 * writes), 1..9 = gzip.
 * Counts the words read and the candidates written.  Returns 0 or a negative code (DWPA_E_IO: a source cannot be
 * opened or the output cannot be written; DWPA_E_RULE: no valid rule). */
int dwpa_rules_expand_file(int device, const char *rules_file, const char *const *sources, size_t nsources,
                           const char *out_path, int gzip_level, uint64_t *words_out, uint64_t *cands_out);
/* Host only: rule `rule_index` (0-based among the rules that parse) applied to one word by the same interpreter the
 * GPU runs, compiled for the host; *out_len = 0xFFFFFFFF when rejected.  out holds 256 bytes. */
int dwpa_rules_apply_host(const char *rules_text, size_t rules_len, uint32_t rule_index, const uint8_t *word,
                          size_t word_len, uint8_t *out, uint32_t *out_len);
/* Host only: rule lines present (neither empty nor '#' comments), how many of them parse, and the 1-based line
 * number of the first one that does not (0 = none). */
int dwpa_rules_count(const char *rules_text, size_t rules_len, uint32_t *nrules_present, uint32_t *nrules_parsed,
                     uint32_t *first_skipped_line);
/* Host only (ABI 3): both loaders' counts for one rules text -- what DWPA_RULES_FULL loads (parsed) and what
 * hashcat's -r loader (DWPA_RULES_HASHCAT) keeps (loaded_hashcat = parsed - rejmem). */
typedef struct {
    uint32_t present;             /* rule lines (neither empty nor '#' comments)                               */
    uint32_t parsed;              /* lines that parse in the whole language: DWPA_RULES_FULL loads these        */
    uint32_t loaded_hashcat;      /* parsed lines free of reject / memory functions: DWPA_RULES_HASHCAT loads these */
    uint32_t rejmem;              /* parsed lines using a reject or memory function                            */
    uint32_t invalid;             /* lines that do not parse (skipped in both modes)                           */
    uint32_t first_invalid_line;  /* 1-based line numbers, 0 = none                                            */
    uint32_t first_rejmem_line;
    uint32_t reserved;
} dwpa_rules_counts;
int dwpa_rules_count_ex(const char *rules_text, size_t rules_len, dwpa_rules_counts *out);

/* ---- device-resident scan API (inputs already in HBM; used by the client loop and bench.py) --------------- */
typedef struct dwpa_scan dwpa_scan;
/* Upload a work unit's hashlines (any number of ESSIDs) to `device` with a batch of `batch` candidate slots. */
int dwpa_scan_create(int device, const char *const *lines, const size_t *line_lens, size_t nlines, int nc,
                     int nc_mode, uint32_t batch, dwpa_scan **out);
int dwpa_scan_num_groups(const dwpa_scan *scan);              /* number of distinct ESSIDs */
int dwpa_scan_line_status(const dwpa_scan *scan, size_t line); /* 0 usable, or the negative parse code */
/* Stage 1: candidates into the batch.  Dictionary words [first, first+count) of an HBM-resident dictionary
 * (d_offsets: count+1 uint64 byte offsets into d_bytes).  Words outside [minlen, maxlen] are dropped
 * (hashcat m22000 accepts 8..63).  count <= batch. */
int dwpa_scan_load_dict(dwpa_scan *scan, const uint64_t *d_offsets, const uint8_t *d_bytes, uint64_t first,
                        uint32_t count, uint32_t minlen, uint32_t maxlen, void *hip_stream);
/* Rule amplification on the GPU: set the scan's rules once (hashcat rule syntax, one per line), then load
 * words [first_word, first_word+nwords) x every rule; candidate id = word * nrules + rule, 8..63 filter applied.
 * nwords * nrules must be <= batch.  Returns the number of rules that parsed (set) or 0 (load). */
int dwpa_scan_set_rules(dwpa_scan *scan, const char *rules_text, size_t rules_len);
int dwpa_scan_load_rules(dwpa_scan *scan, const uint64_t *d_offsets, const uint8_t *d_bytes, uint64_t first_word,
                         uint32_t nwords, void *hip_stream);
/* Decimal keyspace first..first+count-1, zero-padded to `digits` characters. */
int dwpa_scan_load_numeric(dwpa_scan *scan, uint64_t first, uint32_t count, uint32_t digits, void *hip_stream);
/* Mask keyspace (the language and the order: "mask attack" above), generated in-kernel.  Set the scan's mask once
 * (uploads one 16 KiB table; setting it again replaces the previous one; *keyspace, nullable, receives K), then load
 * candidates [first, first + count): candidate id = its index, slot s holds index first + s (no filter, no
 * compaction), and dwpa_scan_loaded then equals count.  A load does not synchronise with the host.  DWPA_E_ARG:
 * count > batch, first + count > K (also when the sum wraps), no mask set.  Without a device: DWPA_E_NODEV. */
int dwpa_scan_set_mask(dwpa_scan *scan, const char *mask, size_t mask_len, const dwpa_bytes custom[4],
                       uint64_t *keyspace);
int dwpa_scan_load_mask(dwpa_scan *scan, uint64_t first, uint32_t count, void *hip_stream);
/* The scan's mask in Markov order under a threshold ("mask attack in Markov order" above): uploads one table of
 * 256 B + 64 KiB per position, *keyspace (nullable) receives the thresholded K, and dwpa_scan_load_mask then generates
 * that order's candidates [first, first + count) (first + count <= K).  It replaces a mask set by either call, and
 * dwpa_scan_set_mask replaces it; while it is set the scan has no mask for dwpa_scan_load_hybrid.  DWPA_E_ARG (the
 * mask set before stays): an invalid mask, threshold above 256, K above 2^64 - 1, not a model image. */
int dwpa_scan_set_mask_markov(dwpa_scan *scan, const char *mask, size_t mask_len, const dwpa_bytes custom[4],
                              const uint8_t *model, size_t model_len, uint32_t threshold, uint64_t *keyspace);
/* Hybrid candidates ("hybrid attacks" above) of words [first_word, first_word + nwords) of an HBM-resident dictionary
 * (d_offsets: at least first_word + nwords + 1 offsets) x the indices [mask_first, mask_first + mask_count) of the
 * mask set by dwpa_scan_set_mask, word-major: nwords * mask_count raw candidates, the kept ones compacted into slots
 * in that order, ids[slot] = word_index * K + mask_index, dwpa_scan_loaded = the kept count.  A load does not
 * synchronise with the host.  DWPA_E_ARG (the scan stays usable): no mask set, mode not 6 or 7, nwords * mask_count >
 * batch, mask_first + mask_count > K (wrap included), (first_word + nwords) * K beyond 64 bits.  Without a device:
 * DWPA_E_NODEV. */
int dwpa_scan_load_hybrid(dwpa_scan *scan, const uint64_t *d_offsets, const uint8_t *d_bytes, uint64_t first_word,
                          uint32_t nwords, uint64_t mask_first, uint32_t mask_count, int mode, uint32_t minlen,
                          uint32_t maxlen, void *hip_stream);
/* Combinator candidates ("combinator attack" above) of base words [first_base, first_base + nbase) of one
 * HBM-resident list (d_base_off: at least first_base + nbase + 1 offsets) x the words [amp_first, amp_first +
 * amp_count) of another (d_amp_off: at least amp_first + amp_count + 1 offsets; amp_words = A, the word count its ids
 * are formed with), base-major: nbase * amp_count raw pairs, the kept ones compacted into slots in that order,
 * ids[slot] = base_index * A + amp_index, dwpa_scan_loaded = the kept count.  amp_side says which list stands left:
 * DWPA_COMBI_AMP_RIGHT joins base || amplifier, DWPA_COMBI_AMP_LEFT amplifier || base.  The call is stateless (both
 * lists are passed each time) and does not synchronise with the host.  A byte buffer needs no padding: only dwords
 * that hold a byte of a kept word are read.  nbase == 0 or amp_count == 0 loads nothing.  DWPA_E_ARG (the scan stays
 * usable): amp_side not 0 or 1, nbase * amp_count > batch, amp_first + amp_count > A (wrap included; so A == 0 with
 * amp_count > 0), (first_base + nbase) * A beyond 64 bits (wrap of the sum included).  Without a device:
 * DWPA_E_NODEV. */
int dwpa_scan_load_combinator(dwpa_scan *scan, const uint64_t *d_base_off, const uint8_t *d_base_bytes,
                              uint64_t first_base, uint32_t nbase, const uint64_t *d_amp_off,
                              const uint8_t *d_amp_bytes, uint64_t amp_words /* A */, uint64_t amp_first,
                              uint32_t amp_count, int amp_side, uint32_t minlen, uint32_t maxlen, void *hip_stream);
/* Chain candidates ("chain attack" above).  A list part names an HBM-resident list (d_offsets: nwords + 1 byte
 * offsets into d_bytes); a mask part names its mask text.  dwpa_scan_set_chain keeps the device pointers (the caller
 * keeps the lists alive while the chain is set), uploads one 16 KiB table per mask part and stores K in *keyspace
 * (nullable).  It leaves the mask of dwpa_scan_set_mask alone: a scan can hold both.  Setting a chain again replaces
 * the previous one.  DWPA_E_ARG (the scan stays usable and keeps its previous chain): nparts 0 or above 4, an unknown
 * kind, an invalid mask, nwords >= 2^32, K above 2^64 - 1.
 * dwpa_scan_load_chain loads the raw indices [first, first + count): the kept ones compacted into slots in index
 * order, ids[slot] = the raw index, dwpa_scan_loaded = the kept count.  A load does not synchronise with the host.
 * A byte buffer needs no padding: only dwords that hold a byte of a kept word are read.  count == 0 loads nothing.
 * DWPA_E_ARG: count > batch, first + count > K (wrap included), no chain set.  Without a device: DWPA_E_NODEV. */
typedef struct {
    int kind;                  /* DWPA_CHAIN_LIST or DWPA_CHAIN_MASK */
    const uint64_t *d_offsets; /* list, in HBM */
    const uint8_t *d_bytes;
    uint64_t nwords;
    const char *mask;          /* mask */
    size_t mask_len;
} dwpa_chain_part;
int dwpa_scan_set_chain(dwpa_scan *scan, const dwpa_chain_part *parts, uint32_t nparts, const dwpa_bytes custom[4],
                        uint64_t *keyspace);
int dwpa_scan_load_chain(dwpa_scan *scan, uint64_t first, uint32_t count, uint32_t minlen, uint32_t maxlen,
                         void *hip_stream);
/* Rules on list part `part` of the chain set by dwpa_scan_set_chain ("Rules on list parts" above): rules_text is
 * parsed as dwpa_scan_set_rules parses it (the whole language) and uploaded; rules_len == 0 takes the part's rules
 * off.  K is recomputed and stored in *keyspace (nullable); dwpa_scan_load_chain then runs k_prep_chain_rules when
 * any part is ruled and k_prep_chain otherwise.  Returns the number of rules parsed.  DWPA_E_ARG: no chain set, part
 * out of range or a mask part, nwords * R >= 2^32, K above 2^64 - 1; DWPA_E_RULE: no rule parses.  A refused call
 * leaves the scan usable with its previous chain and rules; every check is made before anything is read on the
 * device, so an nwords that overstates the list is refused without touching it.  A later dwpa_scan_set_chain clears
 * the rules of every part. */
int dwpa_scan_set_chain_rules(dwpa_scan *scan, uint32_t part, const char *rules_text, size_t rules_len,
                              uint64_t *keyspace /* nullable */);
/* Table candidates ("table attack" above) of an HBM-resident list (d_offsets: nwords + 1 byte offsets into d_bytes),
 * which stays the caller's and must stay alive while the table is set.  dwpa_scan_set_table counts every word on the
 * GPU, builds the kept-word index and keeps it with the table image (the scan owns and frees both); *keyspace and
 * *kept (nullable) receive K and the number of kept words.  It leaves the scan's mask and chain alone, and they leave
 * it alone.  Setting a table again replaces the previous one.  Every check on the call and on the table text comes
 * before anything on the device is touched.  DWPA_E_ARG (the scan stays usable and keeps its previous table): an
 * invalid table, nwords >= 2^32, a null list with nwords > 0, K above 2^64 - 1.
 * dwpa_scan_load_table loads candidates [first, first + count): slot s holds index first + s (no compaction), the
 * candidate id is its index and dwpa_scan_loaded then equals count.  A load does not synchronise with the host.
 * DWPA_E_ARG: count > batch, first + count > K (also when the sum wraps), no table set.  Without a device:
 * DWPA_E_NODEV. */
int dwpa_scan_set_table(dwpa_scan *scan, const uint64_t *d_offsets, const uint8_t *d_bytes, uint64_t nwords,
                        const char *table_text, size_t table_len, uint32_t minlen, uint32_t maxlen,
                        uint32_t word_max, uint64_t *keyspace /* nullable */, uint64_t *kept /* nullable */);
int dwpa_scan_load_table(dwpa_scan *scan, uint64_t first, uint32_t count, void *hip_stream);
/* The scan's nets ("association attack" above): their number, and the net of an input line (DWPA_E_ARG for a line
 * that is not usable). */
int dwpa_scan_num_nets(const dwpa_scan *scan);
int64_t dwpa_scan_net_of_line(const dwpa_scan *scan, size_t line);
/* Association candidates.  dwpa_scan_set_assoc takes the entries of all nets, net-major: words[i] (1..256 bytes)
 * belongs to net net_of_word[i], which never decreases with i; the caller has dropped duplicates.  The scan copies
 * them, builds the index over the nets that own indices and one salt entry per ESSID, and owns all of it.  rules_text
 * (rules_len 0: none, R = 1) takes the whole rule language; a candidate is kept when its length is in minlen..
 * min(maxlen, 63).  *keyspace (nullable) receives K.  DWPA_E_ARG (the previous association stays): a net number out of
 * range or decreasing, a word of 0 or more than 256 bytes, count >= 2^32, W_n x R >= 2^32, K above 2^64 - 1;
 * DWPA_E_RULE: no rule parses.
 * dwpa_scan_load_assoc generates indices [first, first + count): the kept candidates of nets that still have an
 * uncracked line take compacted slots in index order, the candidate id is its index.  dwpa_scan_run then derives every
 * slot with its own net's ESSID and verifies it against that net's uncracked lines only; dwpa_scan_pbkdf2 /
 * dwpa_scan_verify return DWPA_E_ARG until another kind of load.  DWPA_E_ARG: count > batch, first + count > K (also
 * when the sum wraps), no association set.  Without a device: DWPA_E_NODEV. */
int dwpa_scan_set_assoc(dwpa_scan *scan, const dwpa_bytes *words, const uint32_t *net_of_word, size_t count,
                        const char *rules_text, size_t rules_len, uint32_t minlen, uint32_t maxlen,
                        uint64_t *keyspace /* nullable */);
int dwpa_scan_load_assoc(dwpa_scan *scan, uint64_t first, uint32_t count, void *hip_stream);
/* Stages 2 and 3 for ESSID group g (PMKs of the loaded batch, then every uncracked line of that ESSID). */
int dwpa_scan_pbkdf2(dwpa_scan *scan, int group, void *hip_stream);
int dwpa_scan_verify(dwpa_scan *scan, int group, void *hip_stream);
/* Stages 2 and 3 for every ESSID group that still has an uncracked line: one PBKDF2 launch covers as many groups
 * x the loaded batch as fit 16M candidate slots (the ESSID salt is wave-uniform), followed by one verify launch
 * over all of their uncracked lines.  Hits are the same as the per-group calls'.  batch must be a multiple of
 * 64 (dwpa_scan_create rounds it up). */
int dwpa_scan_run(dwpa_scan *scan, void *hip_stream);
/* Synchronises the stream and copies the hits found since the last call into out[0..min(*nhits, cap)).  *nhits is
 * the number found, which can exceed cap; the hits beyond cap are lost, because the call also clears the device's
 * hit buffer.  A cap of at least the scan's batch size always suffices: a batch yields at most one hit per
 * candidate slot and line. */
int dwpa_scan_hits(dwpa_scan *scan, dwpa_hit *out, size_t cap, size_t *nhits, void *hip_stream);
/* Candidate slots filled by the last load (synchronises). */
int dwpa_scan_loaded(dwpa_scan *scan, uint32_t *count, void *hip_stream);
void dwpa_scan_destroy(dwpa_scan *scan);

/* ---- device plumbing for callers without their own HIP runtime (ctypes/PHP) ---------------------------------
 * Buffers, streams and events of the runtime the kernels run on.  Callers that already hold HIP objects from a
 * different HIP runtime instance (e.g. a framework bundling its own libamdhip64) must not pass them here. */
int dwpa_dev_alloc(int device, size_t bytes, void **out);
int dwpa_dev_free(int device, void *p);
int dwpa_dev_upload(int device, void *dst, const void *src, size_t bytes);
int dwpa_dev_download(int device, void *dst, const void *src, size_t bytes);
int dwpa_stream_create(int device, void **out);
int dwpa_stream_sync(void *stream);
int dwpa_stream_destroy(void *stream);
int dwpa_event_create(int device, void **out);
int dwpa_event_record(void *event, void *stream);
int dwpa_event_elapsed_ms(void *start, void *stop, float *ms); /* synchronises on stop */
int dwpa_event_destroy(void *event);

#ifdef __cplusplus
}
#endif
#endif /* DWPA22000_H */
