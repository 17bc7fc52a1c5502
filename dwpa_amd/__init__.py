"""dwpa_amd -- MI355X-native m22000 PMK derivation + verification engine (drop-in for dwpa's hot path).

The product is ``lib/libdwpa22000.so`` (HIP kernels for gfx950 behind the C ABI in ``include/dwpa22000.h``);
this package is its Python host side:

* :func:`check_key_m22000` -- PHP-shaped mirror of ``web/common.php:157-307`` (server key check)
* :func:`check_batch`      -- bulk form (put_work / rkg loops)
* :func:`pbkdf2_pmk`       -- PMK derivation
* :class:`Scan`            -- device-resident scan of HBM dictionaries / keyspaces (client hot loop, bench)
* :func:`crack_mask`       -- hashcat ``-a 3`` mask attack (``python -m dwpa_amd.mask`` is its command line);
  :func:`mask_keyspace` / :func:`mask_candidate` are its host-only helpers
  (``markov=`` / ``threshold=``: the Markov order under hashcat's ``-t``; :func:`markov_train` / :func:`markov_load`
  make and read its model, ``python -m dwpa_amd.markov`` is their command line)
* :func:`crack_hybrid`     -- hashcat ``-a 6`` / ``-a 7`` hybrid attacks, wordlist + mask and mask + wordlist
  (``python -m dwpa_amd.mask -a 6|7``); :meth:`Scan.load_hybrid` is their scan-path load
* :func:`crack_combinator` -- hashcat ``-a 1`` combinator attack, word of one list + word of another
  (``python -m dwpa_amd.mask -a 1``); :meth:`Scan.load_combinator` is its scan-path load
* :func:`crack_chain`      -- chain attack, up to four word lists and masks joined left to right
  (``python -m dwpa_amd.chain``); :meth:`Scan.set_chain` / :meth:`Scan.load_chain` are its scan-path calls,
  :func:`chain_keyspace` / :func:`chain_split` / :func:`chain_candidate` its host-only helpers; a list part may
  carry hashcat rules (``crack_chain(..., rules=)``, :meth:`Scan.set_chain_rules`, ``chain_candidate(..., rules=)``)
* :func:`crack_table`      -- table attack (hashcat-legacy ``-a 5 --table-file``, toggle-case ``-a 2``): every
  combination of per-byte alternatives of every word (``python -m dwpa_amd.table``); :meth:`Scan.set_table` /
  :meth:`Scan.load_table` are its scan-path calls, :func:`table_parse` / :func:`table_builtin` /
  :func:`table_keyspace` / :func:`table_candidates` its host-only helpers
* :func:`crack_assoc`      -- association attack (hashcat ``-a 9``, ``web/rkg.php``'s per-net pass): every net of the
  hash file against its own words -- an association file's ``MAC_AP:WORD`` lines, the built-in single generator, rules
  on top (``python -m dwpa_amd.assoc``); :meth:`Scan.set_assoc` / :meth:`Scan.load_assoc` are its scan-path calls,
  :func:`assoc_single` / :func:`assoc_plan` / :func:`assoc_candidates` its host-only helpers
* :mod:`dwpa_amd.help_crack` -- ``run_cracker`` replacement for help_crack.py
"""
from ._lib import (DWPA_ASSOC_SINGLE, DWPA_CHAIN_LIST, DWPA_CHAIN_MASK, DWPA_CHAIN_MAX_PARTS, DWPA_COMBI_AMP_LEFT,  # noqa: F401
                   DWPA_COMBI_AMP_RIGHT, DWPA_HYBRID_MASK_WORD, DWPA_HYBRID_WORD_MASK, DwpaError, load)
from .m22000 import (BatchJobs, chain_candidate, chain_keyspace, chain_split, check_batch,  # noqa: F401
                     check_key_m22000, crack_chain, crack_combinator, crack_files, crack_hybrid, crack_mask,
                     device_count, group_by_essid, markov_load, markov_train, mask_candidate, mask_candidates, mask_keyspace, check_stats, hash_m22000, hc_unhex, init,
                     parse_m22000, pbkdf2_pmk, rules_count, rules_count_ex, rules_expand, Scan, crack_table, table_builtin,
                     table_candidates, table_keyspace, table_parse, assoc_candidates, assoc_plan, assoc_single,
                     crack_assoc)

__all__ = ["DwpaError", "load", "BatchJobs", "check_key_m22000", "check_batch", "pbkdf2_pmk", "hc_unhex", "hash_m22000",
           "crack_files", "rules_count", "rules_count_ex", "check_stats", "rules_expand", "device_count", "Scan",
           "parse_m22000", "group_by_essid", "init", "crack_mask", "mask_keyspace", "mask_candidate", "mask_candidates", "markov_train", "markov_load",
           "crack_hybrid", "DWPA_HYBRID_WORD_MASK", "DWPA_HYBRID_MASK_WORD",
           "crack_combinator", "DWPA_COMBI_AMP_RIGHT", "DWPA_COMBI_AMP_LEFT",
           "crack_chain", "chain_keyspace", "chain_split", "chain_candidate", "DWPA_CHAIN_LIST", "DWPA_CHAIN_MASK",
           "DWPA_CHAIN_MAX_PARTS", "crack_table", "table_parse", "table_builtin", "table_keyspace", "table_candidates",
           "crack_assoc", "assoc_single", "assoc_plan", "assoc_candidates", "DWPA_ASSOC_SINGLE"]
