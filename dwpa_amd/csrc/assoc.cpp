// assoc.cpp -- the association attack on the host (assoc.hpp has the contract): nets from parsed hashlines, the
// association file, the single generator, entries with their de-duplication, start[] and candidate(id).
#include "assoc.hpp"

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <unordered_set>

#include "dict_reader.hpp"
#include "dwpa22000.h"

namespace dwpa {

void assoc_nets(const std::vector<ParsedLine>& parsed, AssocNets* out) {
    out->nets.clear();
    out->net_of_line.assign(parsed.size(), -1);
    std::map<std::pair<std::string, std::string>, uint32_t> seen;
    for (size_t i = 0; i < parsed.size(); i++) {
        if (parsed[i].status) continue;
        auto key = std::make_pair(parsed[i].essid, parsed[i].mac_ap);
        auto it = seen.find(key);
        if (it == seen.end()) {
            it = seen.emplace(key, (uint32_t)out->nets.size()).first;
            out->nets.push_back(AssocNet{parsed[i].essid, parsed[i].mac_ap, {}});
        }
        out->nets[it->second].lines.push_back((uint32_t)i);
        out->net_of_line[i] = (int32_t)it->second;
    }
}

static std::string ascii_upper(std::string s) {
    for (char& c : s)
        if (c >= 'a' && c <= 'z') c = (char)(c - 32);
    return s;
}
static std::string ascii_lower(std::string s) {
    for (char& c : s)
        if (c >= 'A' && c <= 'Z') c = (char)(c + 32);
    return s;
}

void assoc_single(const std::string& mac_ap, const std::string& essid, uint32_t minlen, std::vector<std::string>* out) {
    if (mac_ap.size() == 6) {
        uint64_t b = 0;
        for (unsigned char c : mac_ap) b = b << 8 | c;
        for (int i = -1; i <= 1; i++) {
            const uint64_t v = (b + (uint64_t)(int64_t)i) & 0xffffffffffffull;
            char hex[13];
            snprintf(hex, sizeof hex, "%012llx", (unsigned long long)v);
            for (int j : {12, 10, 8}) {
                const std::string lo(hex + 12 - j, (size_t)j);
                out->push_back(lo);
                out->push_back(ascii_upper(lo));
            }
        }
    }
    for (const char* suffix : {"", "1", "123", "!"}) {
        const std::string c = essid + suffix;
        if (c.size() < minlen) continue;
        out->push_back(c);
        const std::string up = ascii_upper(c), lo = ascii_lower(c);
        if (up != c) out->push_back(up);
        if (lo != c) out->push_back(lo);
    }
}

static int xd(char c) {
    return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
}

bool assoc_parse_line(const char* p, size_t n, std::string* mac, std::string* word) {
    if (n < 13 || p[12] != ':') return false;
    mac->resize(6);
    for (int i = 0; i < 6; i++) {
        const int h = xd(p[2 * i]), l = xd(p[2 * i + 1]);
        if (h < 0 || l < 0) return false;
        (*mac)[i] = (char)(h << 4 | l);
    }
    word->assign(p + 13, n - 13);
    if (starts_hex((const uint8_t*)word->data(), word->size())) *word = hc_unhex(*word);
    return true;
}

void AssocPlan::split(uint64_t id, size_t* net, uint32_t* rule, uint64_t* entry) const {
    // the last net whose start is <= id: nets without indices repeat their successor's start and are stepped over
    const size_t n = (size_t)(std::upper_bound(start.begin(), start.end(), id) - start.begin()) - 1;
    const uint32_t W = words_of(n);
    const uint32_t sub = (uint32_t)(id - start[n]);
    *net = n;
    *rule = sub / W;
    *entry = wfirst[n] + sub % W;
}

bool AssocPlan::candidate(uint64_t id, std::string* out, size_t* net, uint32_t minlen, uint32_t maxlen) const {
    if (id >= keyspace()) return false;
    size_t n;
    uint32_t rule;
    uint64_t e;
    split(id, &n, &rule, &e);
    if (net) *net = n;
    if (rules) {
        if (!rules->apply_host(rule, word(e), out)) return false;
    } else {
        *out = word(e);
    }
    return out->size() >= minlen && out->size() <= std::min<uint32_t>(maxlen, 63);
}

int assoc_build(AssocNets nets, const std::vector<std::vector<std::string>>& words, const RuleSet* rules,
                AssocPlan* plan) {
    if (words.size() != nets.nets.size() || (rules && rules->size() == 0)) return DWPA_E_ARG;
    plan->nets = std::move(nets);
    plan->rules = rules;
    plan->R = rules ? (uint32_t)std::min<size_t>(rules->size(), UINT32_MAX) : 1u;
    if (rules && rules->size() > UINT32_MAX) return DWPA_E_ARG;
    plan->woff.assign(1, 0);
    plan->wbytes.clear();
    plan->wnet.clear();
    plan->wfirst.assign(1, 0);
    plan->start.assign(1, 0);
    plan->dropped = 0;
    uint64_t K = 0;
    for (size_t n = 0; n < words.size(); n++) {
        std::unordered_set<std::string> seen;
        uint64_t W = 0;
        for (const std::string& w : words[n]) {
            if (w.empty() || w.size() > ASSOC_WORD_MAX || !seen.insert(w).second) {
                plan->dropped++;
                continue;
            }
            plan->wbytes += w;
            plan->woff.push_back(plan->wbytes.size());
            plan->wnet.push_back((uint32_t)n);
            W++;
        }
        const uint64_t own = W * plan->R;  // W <= 2^32 - 1 words would need 4 GiB of host entries per net: no wrap
        if (W > UINT32_MAX || own > UINT32_MAX) return DWPA_E_ARG;
        if (__builtin_add_overflow(K, own, &K)) return DWPA_E_ARG;
        plan->wfirst.push_back(plan->entries());
        plan->start.push_back(K);
    }
    return 0;
}

int assoc_plan(const std::vector<ParsedLine>& parsed, const char* assoc_file, bool single, uint32_t single_minlen,
               const RuleSet* rules, AssocPlan* plan) {
    AssocNets nets;
    assoc_nets(parsed, &nets);
    std::vector<std::vector<std::string>> words(nets.nets.size());
    plan->file_lines = plan->unmatched = plan->malformed = 0;
    if (assoc_file) {
        std::map<std::string, std::vector<uint32_t>> by_mac;  // a MAC under two ESSIDs feeds both nets
        for (size_t n = 0; n < nets.nets.size(); n++) by_mac[nets.nets[n].mac_ap].push_back((uint32_t)n);
        {
            FILE* f = fopen(assoc_file, "rb");
            if (!f) return DWPA_E_IO;
            fclose(f);
        }
        DictReader rd({std::string(assoc_file)});
        Chunk c;
        bool err = false;
        std::string mac, word;
        // the reader decodes a line that is $HEX[...] as a whole; such a line is judged by what it decodes to
        while (rd.next(c, (size_t)1 << 16, (size_t)16 << 20, err)) {
            for (size_t i = 0; i + 1 < c.off.size(); i++) {
                plan->file_lines++;
                const char* p = c.bytes.data() + c.off[i];
                const size_t len = (size_t)(c.off[i + 1] - c.off[i]);
                if (!assoc_parse_line(p, len, &mac, &word)) {
                    plan->malformed++;
                    fprintf(stderr, "[dwpa] %s: line %llu is not MAC_AP:WORD, skipped\n", assoc_file,
                            (unsigned long long)plan->file_lines);
                    continue;
                }
                auto it = by_mac.find(mac);
                if (it == by_mac.end()) {
                    plan->unmatched++;
                    continue;
                }
                for (uint32_t n : it->second) words[n].push_back(word);
            }
        }
        if (err) return DWPA_E_IO;
    }
    if (single)
        for (size_t n = 0; n < nets.nets.size(); n++)
            assoc_single(nets.nets[n].mac_ap, nets.nets[n].essid, single_minlen, &words[n]);
    return assoc_build(std::move(nets), words, rules, plan);
}

}  // namespace dwpa
