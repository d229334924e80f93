// CPU model of td_ngrams.hip's decomposition over tokendagger_amd/csrc/td_ngram_args.h (the hash, the slot layout and the probe are
// the kernel's own): tiles with a halo of 64 starts in front and 63 ids behind, every start attributed to exactly one tile, the
// window hash rolled over runs of sixteen starts (and held against the recomputed one for every window), the bounded probe with the
// id compare, the reach prefix maximum seeded from the halo, and the per-(document, tile) partial sums.  The tile size is an argument.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <vector>

#include "../../tokendagger_amd/csrc/td_ngram_args.h"

using namespace td;

namespace {

struct Set {
    std::vector<NgSlot> slots;
    std::vector<int32_t> ids;
    std::vector<uint32_t> off, orig;
    NgTable tab{};
};

// The set as td_ngram_set_create builds it: the distinct patterns in the list's order, each under its lowest index.
bool build(const int32_t* pat_ids, const int64_t* pat_off, int64_t n_pats, Set& s) {
    std::map<std::vector<int32_t>, uint32_t> first;
    bool seen[NG_MAX_LEN + 1] = {};
    for (int64_t p = 0; p < n_pats; ++p) {
        const int64_t k = pat_off[p + 1] - pat_off[p];
        if (k < 1 || k > NG_MAX_LEN) return false;
        seen[k] = true;
        first.emplace(std::vector<int32_t>(pat_ids + pat_off[p], pat_ids + pat_off[p + 1]), (uint32_t)p);
    }
    for (const auto& kv : first) s.orig.push_back(kv.second);
    std::sort(s.orig.begin(), s.orig.end());
    s.off.push_back(0);
    for (const uint32_t p : s.orig) {
        s.ids.insert(s.ids.end(), pat_ids + pat_off[p], pat_ids + pat_off[p + 1]);
        s.off.push_back((uint32_t)s.ids.size());
    }
    size_t n = 16;
    while (n < 2 * s.orig.size()) n <<= 1;
    s.slots.assign(n, NgSlot{0, 0});
    const uint32_t mask = (uint32_t)(n - 1);
    uint32_t max_probe = 0;
    for (size_t p = 0; p < s.orig.size(); ++p) {
        const int k = (int)(s.off[p + 1] - s.off[p]);
        const int32_t* w = s.ids.data() + s.off[p];
        const uint32_t x = ng_finish(ng_hash_full([w](int j) { return w[j]; }, k), k);
        uint32_t d = 0;
        while (s.slots[(x + d) & mask].pat1) ++d;
        s.slots[(x + d) & mask] = NgSlot{x, (uint32_t)p + 1};
        max_probe = std::max(max_probe, d);
    }
    s.tab.slots = s.slots.data();
    s.tab.pat_ids = s.ids.data();
    s.tab.pat_off = s.off.data();
    s.tab.pat_orig = s.orig.data();
    s.tab.slot_mask = mask;
    s.tab.max_probe = max_probe;
    for (int k = 1; k <= NG_MAX_LEN; ++k)
        if (seen[k]) {
            if (s.tab.n_lengths == NG_MAX_LENGTHS) return false;
            s.tab.lengths8 |= (uint64_t)k << (8 * s.tab.n_lengths++);
        }
    return true;
}

}  // namespace

// stats[6]: tag matches whose ids differed, the longest probe distance, slots, adds to doc_stats, tiles, windows hashed.
// Returns 0, 1 for a bad list, 2 when a rolled hash differed from the recomputed one.
extern "C" int ngram_model(const int32_t* pat_ids, const int64_t* pat_off, int64_t n_pats, const int32_t* ids, const int64_t* tok_off,
                           int64_t n_docs, int tile, int tag_bits, int32_t ignore, uint8_t* cover, int32_t* labels, int64_t* doc_stats,
                           int64_t* pat_counts, int64_t* counts, int64_t* stats) {
    Set set;
    if (tile < NG_PER || tile % NG_PER || !build(pat_ids, pat_off, n_pats, set)) return 1;
    const NgTable& T = set.tab;
    const uint32_t tag_mask = ng_tag_mask(tag_bits);
    const int64_t total = tok_off[n_docs];
    long long failed = 0;
    memset(stats, 0, 6 * sizeof(int64_t));
    memset(counts, 0, 4 * sizeof(int64_t));
    for (int64_t i = 0; i < 2 * n_docs; ++i) doc_stats[i] = 0;
    const auto id_at = [&](int64_t p) { return p >= 0 && p < total ? ids[p] : -1; };  // (what the tile's LDS holds)
    const auto doc_of = [&](int64_t q) { return (int64_t)(std::upper_bound(tok_off, tok_off + n_docs + 1, q) - tok_off) - 1; };
    const int span = NG_FRONT + tile;
    std::vector<int> longest(span), matches(span);
    for (int64_t t0 = 0; t0 < total; t0 += tile) {
        ++stats[4];
        const int64_t base = t0 - NG_FRONT, s0 = std::max<int64_t>(base, 0), s1 = std::min<int64_t>(t0 + tile, total);
        std::fill(longest.begin(), longest.end(), 0);
        std::fill(matches.begin(), matches.end(), 0);
        for (int l = 0; l < T.n_lengths; ++l) {
            const int k = T.length(l);
            const uint32_t bk = ng_base_pow(k);
            uint32_t h = 0;
            for (int j = 0; j < span; ++j) {
                const int64_t q = base + j;
                if (j % NG_PER == 0) h = ng_hash_full([&](int i) { return id_at(q + i); }, k);  // a lane's run begins
                else h = ng_hash_roll(h, id_at(q - 1), id_at(q - 1 + k), bk);
                ++stats[5];
                if (h != ng_hash_full([&](int i) { return id_at(q + i); }, k)) return 2;
                if (q < s0 || q >= s1) continue;
                const int64_t room = std::min<int64_t>(tok_off[doc_of(q) + 1] - q, NG_MAX_LEN);
                if (room < k) continue;
                const int32_t p = ng_probe(T, ng_finish(h, k), k, tag_mask, [&](int i) { return id_at(q + i); }, &failed);
                if (p < 0) continue;
                longest[j] = k;
                ++matches[j];
                if (j >= NG_FRONT && pat_counts) ++pat_counts[T.pat_orig[p]];  // (the halo's starts belong to the tile before)
            }
        }
        int run = 0;  // reach, in the tile's positions; the halo seeds it
        for (int j = 0; j < NG_FRONT; ++j)
            if (longest[j]) run = std::max(run, j + longest[j]);
        std::map<int64_t, std::pair<int64_t, int64_t>> part;  // document -> (occurrences, covered ids) of this tile
        for (int j = NG_FRONT; j < span && base + j < total; ++j) {
            const int64_t q = base + j;
            if (longest[j]) run = std::max(run, j + longest[j]);
            const bool c = run > j;
            if (cover) cover[q] = c;
            if (labels && c) labels[q] = ignore;
            auto& pr = part[doc_of(q)];
            pr.first += matches[j];
            pr.second += c;
        }
        for (const auto& kv : part) {
            if (kv.second.first == 0 && kv.second.second == 0) continue;
            doc_stats[2 * kv.first] += kv.second.first;
            doc_stats[2 * kv.first + 1] += kv.second.second;
            counts[0] += kv.second.first;
            counts[1] += kv.second.second;
            ++stats[3];
        }
    }
    for (int64_t d = 0; d < n_docs; ++d) counts[2] += doc_stats[2 * d] > 0;
    stats[0] = failed;
    stats[1] = T.max_probe;
    stats[2] = (int64_t)set.slots.size();
    return 0;
}
