// assoc.hpp -- the association attack (hashcat -a 9; web/rkg.php's per-net pass): every net of the hash file is tried
// against ITS OWN words, not against one stream shared by all nets.  Host only: nothing here touches a device, so the
// whole file builds into a stand-alone program (tools/assoc_fuzz.cpp).
//
// Net.      The pair (ESSID bytes, MAC_AP bytes) of a usable hashline (the parser's status 0).  Nets are numbered by
//           first appearance in the hash file; all usable lines with that pair belong to the net, PMKID and EAPOL of any
//           keyver, any MAC_STA.
// Entries.  A net's words, in order: the association file's lines whose key is the net's MAC_AP, in file order; then,
//           with `single`, the built-in generator's words.  A word equal byte for byte to an earlier word of the same
//           net is dropped (the first stays); a word of 0 bytes or above 256 is dropped, as the rule engine's load_word
//           rejects it.  W_n words are left; a net with W_n = 0 owns no indices.
// File.     Through the dictionary reader (plain or gzip, CRLF).  A line is MAC_AP:WORD -- 12 hex digits in either case,
//           one ':', the word; $HEX[...] is decoded for the WORD part only.  A line of another shape is skipped with one
//           stderr line and counted (malformed); a line whose MAC matches no net is counted (unmatched) and skipped.  A
//           MAC that occurs under two ESSIDs feeds both nets.
// Single.   The library's own restatement of rkg.php:48-77.  From the BSSID as a 48-bit integer b (a MAC_AP of 6
//           bytes; any other length gives no BSSID words): for i in -1, 0, +1 and j in 12, 10, 8 the last j hex digits of
//           (b + i) mod 2^48, zero-padded to j, lowercase then uppercase.  From the ESSID e: for each suffix in "", "1",
//           "123", "!" c = e + suffix; c, then its ASCII uppercase if that differs, then its ASCII lowercase if that
//           differs.  ESSID-derived words shorter than minlen are omitted (8 without rules, 1 with rules, so that
//           linksys + $1 is reachable).
// Keyspace. R = the number of rules, 1 (the identity) without a rules file.  Net n owns W_n x R consecutive indices from
//           start[n], RULE-MAJOR with the word fastest (a ruled chain part's order): sub = id - start[n], rule = sub /
//           W_n, word = sub % W_n.  K = start[N] <= 2^64 - 1 and every W_n x R < 2^32, or the plan is refused.
// Candidate. The rule applied to the word by the shared interpreter (rules_apply.hpp); a rejected result, or one outside
//           8..63 bytes, gives no candidate.
// Association.  A candidate of net n is derived with net n's ESSID and verified against the not-yet-cracked lines of
//           net n and nothing else -- not against a line of another net with the same ESSID, though that line would
//           accept the same PMK.  Two nets that share an ESSID and a word derive that PMK twice (hashcat -a 9 does too).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "m22000_host.hpp"
#include "rules.hpp"

namespace dwpa {

constexpr uint32_t ASSOC_WORD_MAX = 256;  // RULE_RP: what load_word takes

struct AssocNet {
    std::string essid, mac_ap;
    std::vector<uint32_t> lines;  // input lines, ascending; lines[0] is the net's first
};

struct AssocNets {
    std::vector<AssocNet> nets;
    std::vector<int32_t> net_of_line;  // per input line; -1: not usable
};
void assoc_nets(const std::vector<ParsedLine>& parsed, AssocNets* out);

// The single generator's words for one net, in order, duplicates included (entry building drops them).
void assoc_single(const std::string& mac_ap, const std::string& essid, uint32_t minlen, std::vector<std::string>* out);

// One line of the association file (without its line end).  False: not MAC_AP:WORD.
bool assoc_parse_line(const char* p, size_t n, std::string* mac, std::string* word);

struct AssocPlan {
    AssocNets nets;
    std::vector<uint64_t> woff{0};  // entries of all nets, net-major: entries + 1 offsets into wbytes
    std::string wbytes;
    std::vector<uint32_t> wnet;     // per entry: its net
    std::vector<uint64_t> wfirst;   // per net: its first entry; nets + 1
    std::vector<uint64_t> start;    // per net: its first index; nets + 1
    uint32_t R = 1;
    const RuleSet* rules = nullptr;  // null: the identity
    uint64_t file_lines = 0, unmatched = 0, malformed = 0, dropped = 0;

    uint64_t entries() const { return woff.size() - 1; }
    uint64_t keyspace() const { return start.empty() ? 0 : start.back(); }
    uint32_t words_of(size_t net) const { return (uint32_t)(wfirst[net + 1] - wfirst[net]); }
    std::string word(uint64_t e) const { return wbytes.substr((size_t)woff[e], (size_t)(woff[e + 1] - woff[e])); }
    // Index id (< K) -> its net, rule and entry.
    void split(uint64_t id, size_t* net, uint32_t* rule, uint64_t* entry) const;
    // The candidate of index id; false: id >= K, the rule rejects, or the result is outside minlen..maxlen.
    bool candidate(uint64_t id, std::string* out, size_t* net = nullptr, uint32_t minlen = 8, uint32_t maxlen = 63) const;
};

// Entries and start[] from per-net word lists (sources already in order); drops duplicates and words of 0 or more than
// ASSOC_WORD_MAX bytes.  DWPA_E_ARG: K above 2^64 - 1 or a net with W_n x R >= 2^32.
int assoc_build(AssocNets nets, const std::vector<std::vector<std::string>>& words, const RuleSet* rules, AssocPlan* plan);

// The whole plan from parsed hashlines: assoc_file (nullable) read through the dictionary reader, `single` adds the
// generator's words with `single_minlen`.  DWPA_E_IO: the file cannot be read; DWPA_E_ARG as assoc_build.
int assoc_plan(const std::vector<ParsedLine>& parsed, const char* assoc_file, bool single, uint32_t single_minlen,
               const RuleSet* rules, AssocPlan* plan);

}  // namespace dwpa
