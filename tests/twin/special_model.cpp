// CPU model of td_special.hip's decomposition over tokendagger_amd/csrc/td_special_dev.h (the candidate test, the match, the document
// limit and the cluster walk are the kernels' own) and td_special_table.h (the table is the handle's own): candidates per 32-byte
// word onto a list of bounded capacity, a match per listed candidate into the hit bitmap, heads and their cluster walks into the
// accept bitmap, and the document bits td_special_mark sets at both ends of every accepted literal.  The stage rewrite of
// td_special_ids is not modelled.
//
// SP_MODEL_CAND_EXTRA (build time): the list holds n / 32 + SP_MODEL_CAND_EXTRA candidates, 4096 in the product
// (special_search_prepare); a smaller value brings the overflow exit within reach of small texts.
// SP_MODEL_MAIN (build time): a stand-alone program that runs seeded cases against a brute-force statement of the rule.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../../tokendagger_amd/csrc/td_special_table.h"

#ifndef SP_MODEL_CAND_EXTRA
#define SP_MODEL_CAND_EXTRA 4096
#endif

using namespace td;

namespace {

enum { SPM_OK = 0, SPM_BAD_INPUT = 1, SPM_SCRATCH = 2, SPM_LOADS_DIFFER = 3 };
// stats
enum { SPM_S_CANDIDATES = 0, SPM_S_CAP = 1, SPM_S_FIRST_LOST = 2, SPM_S_HITS = 3, SPM_S_HEADS = 4, SPM_S_REMATCHES = 5, SPM_S_CLIMBS = 6, SPM_S_MAXLEN = 7, SPM_N_STATS = 8 };

}  // namespace

// text[0, n) cut into n_docs documents by doc_off; literal k = lit_bytes[lit_off[k], lit_off[k + 1]) with id lit_ids[k], in any
// order, a string twice counts once (the first in sorted order).  aligned: the scan takes its words by the 16-byte loads of an
// aligned text where the kernel does (both loads are held against each other everywhere).
// -> out_pos / out_len / out_id [*n_out]: the literals cut out, ascending; hitbits, accbits [(n + 31) / 32], docbits [(n + 31) / 32 + 1]
//    (after td_special_mark); stats[SPM_N_STATS].
// Returns SPM_OK; SPM_SCRATCH when the candidates did not fit their list: the kernel raises TD_E_SCRATCH at one of the candidates
// that found no room (stats[SPM_S_FIRST_LOST]: the first of them in text order), and the outputs are those of the listed ones.
extern "C" int special_model(const uint8_t* text, int64_t n, const int64_t* doc_off, int64_t n_docs, const uint8_t* lit_bytes,
                             const int64_t* lit_off, const int32_t* lit_ids, int64_t n_lits, int aligned, int64_t* out_pos,
                             int32_t* out_len, int32_t* out_id, int64_t* n_out, uint32_t* hitbits, uint32_t* accbits, uint32_t* docbits,
                             int64_t* stats) {
    memset(stats, 0, SPM_N_STATS * sizeof(int64_t));
    *n_out = 0;
    if (n < 0 || n_docs < 0 || doc_off[0] != 0 || doc_off[n_docs] != n) return SPM_BAD_INPUT;
    std::vector<std::pair<std::string, int32_t>> lits;
    for (int64_t k = 0; k < n_lits; ++k) {
        const int64_t len = lit_off[k + 1] - lit_off[k];
        if (len < 1 || len > (int64_t)SP_MAXLEN) return SPM_BAD_INPUT;
        lits.emplace_back(std::string((const char*)lit_bytes + lit_off[k], (size_t)len), lit_ids[k]);
    }
    std::sort(lits.begin(), lits.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
    lits.erase(std::unique(lits.begin(), lits.end(), [](const auto& x, const auto& y) { return x.first == y.first; }), lits.end());
    const SpecialTableHost T = special_table_build(lits);
    const int64_t nw = (n + 31) >> 5;
    const uint32_t cap = (uint32_t)(n / 32 + SP_MODEL_CAND_EXTRA);
    std::vector<int64_t> cand_pos(std::max<uint32_t>(cap, 1));
    std::vector<int32_t> cand_lit(std::max<uint32_t>(cap, 1), -1);
    uint32_t count = 0;
    SpecialTable S;
    memset(&S, 0, sizeof S);
    S.bytes = T.bytes.data();
    S.off = T.off.data();
    S.len = T.len.data();
    S.id = T.id.data();
    S.parent = T.parent.data();
    S.first2 = T.first2.data();
    S.cand_pos = cand_pos.data();
    S.cand_lit = cand_lit.data();
    S.cand_count = &count;
    S.cand_cap = cap;
    S.hitbits = hitbits;
    S.accbits = accbits;
    S.n = (uint32_t)lits.size();
    S.maxlen = T.maxlen;
    stats[SPM_S_CAP] = cap;
    stats[SPM_S_MAXLEN] = T.maxlen;
    stats[SPM_S_FIRST_LOST] = -1;
    // td_mark_docs: a bit where a document starts
    for (int64_t w = 0; w < nw + 1; ++w) docbits[w] = 0;
    for (int64_t d = 0; d < n_docs; ++d) {
        if (doc_off[d + 1] < doc_off[d]) return SPM_BAD_INPUT;
        if (doc_off[d] < n) docbits[doc_off[d] >> 5] |= 1u << (doc_off[d] & 31);
    }
    if (S.n == 0 || n == 0) return SPM_OK;
    // td_special_scan: a lane per 32 bytes
    for (int64_t w = 0; w < nw; ++w) {
        const int64_t p0 = w << 5;
        uint32_t tw[9], tb[9];
        sp_words_bytewise(text, n, p0, tb);
        if (aligned && p0 + 36 <= n) {
            memcpy(tw, text + p0, 32);  // (two 16-byte loads: little-endian words)
            tw[8] = text[p0 + 32];
            if (memcmp(tw, tb, sizeof tw)) return SPM_LOADS_DIFFER;
        } else {
            memcpy(tw, tb, sizeof tw);
        }
        const uint32_t cand = sp_word_candidates(tw, S.first2, p0, n);
        hitbits[w] = 0;
        accbits[w] = 0;
        for (uint32_t m = cand; m; m &= m - 1u) {
            const int64_t cp = p0 + sp_low_bit(m);
            if (count < cap) cand_pos[count] = cp;
            else if (stats[SPM_S_FIRST_LOST] < 0) stats[SPM_S_FIRST_LOST] = cp;
            ++count;
        }
    }
    stats[SPM_S_CANDIDATES] = count;
    const uint32_t nc = count < cap ? count : cap;
    // td_special_match: a lane per candidate
    for (uint32_t j = 0; j < nc; ++j) {
        const int64_t p = cand_pos[j];
        const int i = sp_match(S, text, p, sp_doc_limit(docbits, n, p, S.maxlen));
        cand_lit[j] = i;
        if (i >= 0) {
            hitbits[p >> 5] |= 1u << (p & 31);
            ++stats[SPM_S_HITS];
        }
    }
    // td_special_accept: the head of every cluster walks it
    for (uint32_t j = 0; j < nc; ++j) {
        const int i = cand_lit[j];
        if (i < 0) continue;
        const int64_t p = cand_pos[j];
        if (!sp_is_head(S, p)) continue;
        ++stats[SPM_S_HEADS];
        sp_cluster_walk(
            S, n, p, i, [&](int64_t cur) { accbits[cur >> 5] |= 1u << (cur & 31); },
            [&](int64_t cur) {
                ++stats[SPM_S_REMATCHES];
                return sp_match(S, text, cur, sp_doc_limit(docbits, n, cur, S.maxlen));
            });
    }
    // td_special_mark (it reads the document bits the match read: taken from a copy here, the kernel runs behind the walks)
    std::vector<uint32_t> marked(docbits, docbits + nw + 1);
    for (uint32_t j = 0; j < nc; ++j) {
        const int i = cand_lit[j];
        const int64_t p = cand_pos[j];
        if (i < 0 || !((accbits[p >> 5] >> (p & 31)) & 1u)) continue;
        const int64_t e = p + (int64_t)S.len[i];
        marked[p >> 5] |= 1u << (p & 31);
        if (e < n) marked[e >> 5] |= 1u << (e & 31);
        int climbs = 0;
        for (int q = S.parent[i]; q >= 0; q = S.parent[q]) ++climbs;
        stats[SPM_S_CLIMBS] = std::max<int64_t>(stats[SPM_S_CLIMBS], climbs);  // (the depth of the deepest literal cut out)
        out_pos[*n_out] = p;
        out_len[*n_out] = (int32_t)S.len[i];
        out_id[*n_out] = S.id[i];
        ++*n_out;
    }
    memcpy(docbits, marked.data(), (size_t)(nw + 1) * 4);
    return count > cap ? SPM_SCRATCH : SPM_OK;
}

#ifdef SP_MODEL_MAIN
// Stand-alone: seeded cases (literal sets from strings of 1 to 6 letters over {a,b,c,d}, the same stretched to 48 bytes by a shared
// prefix; texts that are soups of literals, their prefixes and other bytes; documents cut anywhere) against the rule stated plainly.
#include <stdio.h>
#include <stdlib.h>

#include <random>

namespace {

struct Cut { int64_t pos; int32_t len, id; };

std::vector<Cut> brute(const std::string& text, const std::vector<int64_t>& offs, const std::vector<std::pair<std::string, int32_t>>& lits) {
    std::vector<Cut> out;
    for (size_t d = 0; d + 1 < offs.size(); ++d)
        for (int64_t p = offs[d]; p < offs[d + 1];) {
            int best = -1;
            for (size_t k = 0; k < lits.size(); ++k) {
                const std::string& s = lits[k].first;
                if (p + (int64_t)s.size() <= offs[d + 1] && text.compare((size_t)p, s.size(), s) == 0 &&
                    (best < 0 || s.size() > lits[(size_t)best].first.size()))
                    best = (int)k;
            }
            if (best < 0) { ++p; continue; }
            out.push_back({p, (int32_t)lits[(size_t)best].first.size(), lits[(size_t)best].second});
            p += (int64_t)lits[(size_t)best].first.size();
        }
    return out;
}

}  // namespace

int main(int argc, char** argv) {
    const int cases = argc > 1 ? atoi(argv[1]) : 4000;
    std::mt19937_64 rng(20240607);
    const auto below = [&](uint64_t k) { return (int64_t)(rng() % k); };
    const std::string stretch = "abcdabcdabcdabcdabcdabcdabcdabcdabcdabcdabcdabcd";  // (stretched literals are 48 bytes, 40 of them shared by all)
    int64_t cuts = 0, overflowed = 0, bytes = 0;
    for (int c = 0; c < cases; ++c) {
        const bool longs = c % 3 == 2;
        std::vector<std::pair<std::string, int32_t>> lits;
        const int n_lits = 1 + (int)below(8);
        for (int k = 0; k < n_lits; ++k) {
            std::string s;
            const int len = 1 + (int)below(6);
            for (int j = 0; j < len; ++j) s.push_back((char)('a' + below(4)));
            if (longs && below(4)) s = stretch.substr(0, (size_t)(48 - len)) + s;
            bool dup = false;
            for (const auto& l : lits) dup |= l.first == s;
            if (!dup) lits.emplace_back(s, 200000 + k);
        }
        std::string text;
        const int parts = (int)below(60);
        for (int k = 0; k < parts; ++k) {
            const std::string& s = lits[(size_t)below(lits.size())].first;
            switch (below(4)) {
                case 0: text += s; break;
                case 1: text += s.substr(0, (size_t)below(s.size() + 1)); break;
                case 2: text.push_back((char)('a' + below(5))); break;
                default: text.push_back((char)below(256)); break;
            }
        }
        const int64_t n = (int64_t)text.size();
        std::vector<int64_t> offs{0, n};
        for (int k = (int)below(5); k > 0; --k) offs.push_back(below((uint64_t)n + 1));
        std::sort(offs.begin(), offs.end());
        std::string lb;
        std::vector<int64_t> lo{0};
        std::vector<int32_t> li;
        for (const auto& l : lits) { lb += l.first; lo.push_back((int64_t)lb.size()); li.push_back(l.second); }
        const int64_t nw = (n + 31) / 32;
        // (every buffer at its exact size: a read or write past an end is the sanitizer's to see)
        std::vector<uint8_t> tbuf(text.begin(), text.end());
        std::vector<int64_t> pos((size_t)n + 1);
        std::vector<int32_t> len((size_t)n + 1), id((size_t)n + 1);
        std::vector<uint32_t> hit((size_t)nw), acc((size_t)nw), doc((size_t)nw + 1);
        int64_t n_out = 0, stats[SPM_N_STATS];
        const int rc = special_model(tbuf.data(), n, offs.data(), (int64_t)offs.size() - 1, (const uint8_t*)lb.data(), lo.data(), li.data(),
                                     (int64_t)li.size(), c & 1, pos.data(), len.data(), id.data(), &n_out, hit.data(), acc.data(), doc.data(), stats);
        bytes += n;
        if (rc == SPM_SCRATCH) { ++overflowed; continue; }
        if (rc != SPM_OK) { printf("case %d: the model returned %d\n", c, rc); return 1; }
        const std::vector<Cut> want = brute(text, offs, lits);
        bool same = (int64_t)want.size() == n_out;
        for (size_t k = 0; same && k < want.size(); ++k) same = want[k].pos == pos[k] && want[k].len == len[k] && want[k].id == id[k];
        if (!same) { printf("case %d: the model's cuts differ from the rule's (%lld against %zu)\n", c, (long long)n_out, want.size()); return 1; }
        cuts += n_out;
    }
    printf("special_model: %d cases, %lld bytes, %lld cuts, %lld overflowed their list (capacity n/32 + %d): all equal the rule\n", cases,
           (long long)bytes, (long long)cuts, (long long)overflowed, (int)SP_MODEL_CAND_EXTRA);
    return 0;
}
#endif
