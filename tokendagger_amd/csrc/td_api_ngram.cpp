// N-gram matches (td_ngrams.hip): the list's checks, the set (de-duplicated list + lookup table, built on the host), the contract's
// host statement and the entry points.
#include <numeric>
#include <unordered_map>

#include "td_handle.h"
#include "td_ngrams.h"

struct td_ngram_set {
    int device = 0;
    NgTable tab{};                 // device pointers
    void* allocs[4] = {};          // slots, pat_ids, pat_off, pat_orig
    int64_t n_pats = 0, n_distinct = 0, n_lengths = 0, max_len = 0, slots = 0, max_probe = 0, device_bytes = 0;
    ~td_ngram_set() {
        DeviceGuard dg(device);
        for (void* p : allocs)
            if (p) (void)hipFree(p);
    }
};

namespace {

struct NgSpec {
    int32_t ignore;
    bool accumulate;
};

const char* ngram_spec_error(const td_ngram_spec* sp, NgSpec& out) {
    if (!sp) return "null td_ngram_spec";
    if (sp->flags & ~(int64_t)TD_NGRAM_ACCUMULATE) return "flags must be 0 or TD_NGRAM_ACCUMULATE";
    if (sp->ignore_index < INT32_MIN || sp->ignore_index > INT32_MAX) return "ignore_index must be an int32";
    out.ignore = (int32_t)sp->ignore_index;
    out.accumulate = (sp->flags & TD_NGRAM_ACCUMULATE) != 0;
    return nullptr;
}

// The checks of a list (no handle, no device); lengths: the distinct ones, ascending.
const char* ngram_list_error(const int32_t* pat_ids, const int64_t* pat_offsets, int64_t n_pats, std::vector<int>& lengths) {
    if (n_pats < 1 || n_pats > NG_MAX_PATS) return "n_pats must be in 1 .. 2^24";
    if (!pat_offsets) return "null pat_offsets";
    if (pat_offsets[0] != 0) return "pat_offsets must start at 0";
    bool seen[NG_MAX_LEN + 1] = {};
    for (int64_t p = 0; p < n_pats; ++p) {
        const int64_t k = pat_offsets[p + 1] - pat_offsets[p];
        if (k < 1 || k > NG_MAX_LEN) return "every pattern's length must be in 1 .. 64";
        if (pat_offsets[p + 1] > NG_MAX_IDS) return "the patterns hold more than 2^28 ids";
        seen[k] = true;
    }
    lengths.clear();
    for (int k = 1; k <= NG_MAX_LEN; ++k)
        if (seen[k]) lengths.push_back(k);
    if ((int)lengths.size() > NG_MAX_LENGTHS) return "more than 8 distinct pattern lengths";
    if (!pat_ids) return "null pat_ids";
    for (int64_t i = 0; i < pat_offsets[n_pats]; ++i)
        if (pat_ids[i] < 0) return "a pattern id is negative";
    return nullptr;
}

int ngram_matches_locked(td_tokenizer* t, const td_ngram_set* set, const void* d_ids, int64_t n_tokens, const void* d_toff, int64_t n_docs,
                         const NgSpec& sp, void* d_cover, void* d_labels, void* d_doc_stats, void* d_pat_counts, void* d_counts, hipStream_t s) {
    int rc;
    if ((rc = order_before(t, s))) return rc;
    if ((rc = ensure(t, t->ng_head, NG_H_WORDS * 8))) return rc;
    if (!d_doc_stats) {
        if ((rc = ensure(t, t->ng_stats, (size_t)std::max<int64_t>(n_docs, 1) * 16))) return rc;
        d_doc_stats = t->ng_stats.p;
    }
    NgramArgs a;
    memset(&a, 0, sizeof a);
    a.ids = (const int32_t*)d_ids;
    a.n_tokens = n_tokens;
    a.tok_off = (const int64_t*)d_toff;
    a.n_docs = n_docs;
    a.tab = set->tab;
    a.tag_mask = ng_tag_mask(t->opt.ngram_tag_bits);
    a.ignore = sp.ignore;
    a.cover = (uint8_t*)d_cover;
    a.labels = (int32_t*)d_labels;
    a.doc_stats = (unsigned long long*)d_doc_stats;
    a.pat_counts = (unsigned long long*)d_pat_counts;
    a.counts = (unsigned long long*)d_counts;
    a.head = (unsigned long long*)t->ng_head.p;
    Ctl* ctl = (Ctl*)t->ctl.p;
    a.err = &ctl->err;
    a.err_pos = &ctl->err_pos;
    HIP_TRY(t, hipMemsetAsync(a.head, 0, NG_H_WORDS * 8, s));
    HIP_TRY(t, launch_ngram_matches(a, set->n_pats, !sp.accumulate, s));
    return order_after(t, s);
}

// The host forms' end: `total` ids on the device with their offsets on `s` -> the handle's buffers -> the caller's.  labels (host, may
// be null) goes up first; with TD_NGRAM_ACCUMULATE the device's pattern counts are added to the caller's on the host.
int ngram_to_host(td_tokenizer* t, const td_ngram_set* set, const void* d_ids, int64_t total, const void* d_toff, int64_t n_docs,
                  const NgSpec& sp, uint8_t* cover, int32_t* labels, int64_t* doc_stats, int64_t* pattern_counts, int64_t* counts,
                  hipStream_t s) {
    int rc;
    const size_t n1 = (size_t)std::max<int64_t>(total, 1), pats = (size_t)set->n_pats;
    if (cover && (rc = ensure(t, t->ng_cover, n1))) return rc;
    if (labels && (rc = ensure(t, t->ng_labels, n1 * 4))) return rc;
    if (doc_stats && (rc = ensure(t, t->ng_doc_stats, (size_t)std::max<int64_t>(n_docs, 1) * 16))) return rc;
    if (pattern_counts && (rc = ensure(t, t->ng_pats, pats * 8))) return rc;
    if ((rc = ensure(t, t->ng_counts, 4 * sizeof(int64_t)))) return rc;
    if (labels && total > 0) HIP_TRY(t, hipMemcpyAsync(t->ng_labels.p, labels, (size_t)total * 4, hipMemcpyHostToDevice, s));
    NgSpec fresh = sp;
    fresh.accumulate = false;
    if ((rc = ngram_matches_locked(t, set, d_ids, total, d_toff, n_docs, fresh, cover ? t->ng_cover.p : nullptr, labels ? t->ng_labels.p : nullptr,
                                   doc_stats ? t->ng_doc_stats.p : nullptr, pattern_counts ? t->ng_pats.p : nullptr, t->ng_counts.p, s)))
        return rc;
    if ((rc = device_status_locked(t, s, nullptr))) return rc;
    if ((rc = copy_wait(t, counts, t->ng_counts.p, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, s))) return rc;
    if (doc_stats && (rc = copy_wait(t, doc_stats, t->ng_doc_stats.p, (size_t)n_docs * 16, hipMemcpyDeviceToHost, s))) return rc;
    if (pattern_counts) {
        if (!sp.accumulate) {
            if ((rc = copy_wait(t, pattern_counts, t->ng_pats.p, pats * 8, hipMemcpyDeviceToHost, s))) return rc;
        } else {
            std::unique_ptr<int64_t[]> got(new int64_t[pats]);
            if ((rc = copy_wait(t, got.get(), t->ng_pats.p, pats * 8, hipMemcpyDeviceToHost, s))) return rc;
            for (size_t p = 0; p < pats; ++p) pattern_counts[p] += got[p];
        }
    }
    if (total == 0) return TD_OK;
    if (cover && (rc = copy_wait(t, cover, t->ng_cover.p, (size_t)total, hipMemcpyDeviceToHost, s))) return rc;
    if (labels && (rc = copy_wait(t, labels, t->ng_labels.p, (size_t)total * 4, hipMemcpyDeviceToHost, s))) return rc;
    return TD_OK;
}

int ngram_set_check(td_tokenizer* t, const char* fn, const td_ngram_set* set) {
    if (set->device != t->device) return fail_unlocked(t, TD_E_INVALID, std::string(fn) + ": the set lives on another device");
    return TD_OK;
}

}  // namespace

extern "C" {

int td_ngram_set_create(td_tokenizer* t, const int32_t* pat_ids, const int64_t* pat_offsets, int64_t n_pats, td_ngram_set** out) {
    if (!t || !out) return TD_E_INVALID;
    *out = nullptr;
    std::vector<int> lengths;
    if (const char* m = ngram_list_error(pat_ids, pat_offsets, n_pats, lengths))
        return fail_unlocked(t, TD_E_INVALID, std::string("td_ngram_set_create: ") + m);
    // ---- the distinct patterns: sorted by (length, ids, index), the first of every run of equal ones ---------------------------------
    std::vector<uint32_t> order((size_t)n_pats);
    std::iota(order.begin(), order.end(), 0u);
    const auto len_of = [&](uint32_t p) { return (int)(pat_offsets[p + 1] - pat_offsets[p]); };
    const auto cmp_ids = [&](uint32_t x, uint32_t y) {  // (equal lengths)
        return memcmp(pat_ids + pat_offsets[x], pat_ids + pat_offsets[y], (size_t)len_of(x) * 4);
    };
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        if (len_of(x) != len_of(y)) return len_of(x) < len_of(y);
        const int c = cmp_ids(x, y);
        return c != 0 ? c < 0 : x < y;
    });
    std::vector<uint32_t> orig;
    for (size_t i = 0; i < order.size(); ++i)
        if (i == 0 || len_of(order[i]) != len_of(order[i - 1]) || cmp_ids(order[i], order[i - 1]) != 0) orig.push_back(order[i]);
    std::sort(orig.begin(), orig.end());  // (the distinct patterns in the list's order)
    const size_t nd = orig.size();
    std::vector<int32_t> ids;
    std::vector<uint32_t> off(nd + 1, 0);
    for (size_t p = 0; p < nd; ++p) {
        ids.insert(ids.end(), pat_ids + pat_offsets[orig[p]], pat_ids + pat_offsets[orig[p] + 1]);
        off[p + 1] = (uint32_t)ids.size();
    }
    // ---- the table ---------------------------------------------------------------------------------------------------------------------
    size_t slots = 16;
    while (slots < 2 * nd) slots <<= 1;
    std::vector<NgSlot> table(slots, NgSlot{0, 0});
    const uint32_t mask = (uint32_t)(slots - 1);
    uint32_t max_probe = 0;
    for (size_t p = 0; p < nd; ++p) {
        const int k = (int)(off[p + 1] - off[p]);
        const int32_t* w = ids.data() + off[p];
        const uint32_t x = ng_finish(ng_hash_full([w](int j) { return w[j]; }, k), k);
        uint32_t d = 0;
        while (table[(x + d) & mask].pat1) ++d;  // (at most half the slots are taken)
        table[(x + d) & mask] = NgSlot{x, (uint32_t)p + 1};
        max_probe = std::max(max_probe, d);
    }
    // ---- to the device -----------------------------------------------------------------------------------------------------------------
    std::unique_ptr<td_ngram_set> set(new td_ngram_set);
    set->device = t->device;
    const int rc = locked(t, [&] {
        int rc;
        if ((rc = own_streams(t))) return rc;
        const void* src[4] = {table.data(), ids.data(), off.data(), orig.data()};
        const size_t bytes[4] = {slots * sizeof(NgSlot), ids.size() * 4, off.size() * 4, orig.size() * 4};
        for (int i = 0; i < 4; ++i) {
            HIP_TRY(t, hipMalloc(&set->allocs[i], bytes[i]));
            set->device_bytes += (int64_t)bytes[i];
            if ((rc = copy_wait(t, set->allocs[i], src[i], bytes[i], hipMemcpyHostToDevice, t->s_own))) return rc;
        }
        return (int)TD_OK;
    });
    if (rc) return rc;
    set->tab.slots = (const NgSlot*)set->allocs[0];
    set->tab.pat_ids = (const int32_t*)set->allocs[1];
    set->tab.pat_off = (const uint32_t*)set->allocs[2];
    set->tab.pat_orig = (const uint32_t*)set->allocs[3];
    set->tab.slot_mask = mask;
    set->tab.max_probe = max_probe;
    set->tab.n_lengths = (int32_t)lengths.size();
    for (size_t l = 0; l < lengths.size(); ++l) set->tab.lengths8 |= (uint64_t)lengths[l] << (8 * l);
    set->n_pats = n_pats;
    set->n_distinct = (int64_t)nd;
    set->n_lengths = (int64_t)lengths.size();
    set->max_len = lengths.back();
    set->slots = (int64_t)slots;
    set->max_probe = max_probe;
    *out = set.release();
    return TD_OK;
}

void td_ngram_set_destroy(td_ngram_set* set) { delete set; }

int64_t td_ngram_set_info(const td_ngram_set* set, int what) {
    if (!set) return -1;
    switch (what) {
        case TD_NGRAM_INFO_PATTERNS: return set->n_pats;
        case TD_NGRAM_INFO_DISTINCT: return set->n_distinct;
        case TD_NGRAM_INFO_LENGTHS: return set->n_lengths;
        case TD_NGRAM_INFO_MAX_LEN: return set->max_len;
        case TD_NGRAM_INFO_SLOTS: return set->slots;
        case TD_NGRAM_INFO_MAX_PROBE: return set->max_probe;
        case TD_NGRAM_INFO_DEVICE_BYTES: return set->device_bytes;
    }
    return -1;
}

int td_ngram_matches_host(const int32_t* pat_ids, const int64_t* pat_offsets, int64_t n_pats, const int32_t* ids, int64_t n_tokens,
                          const int64_t* tok_offsets, int64_t n_docs, const td_ngram_spec* spec, uint8_t* cover, int32_t* labels,
                          int64_t* doc_stats, int64_t* pattern_counts, int64_t* counts) {
    NgSpec sp;
    std::vector<int> lengths;
    if (!counts || !tok_offsets || n_tokens < 0 || n_docs < 0 || ngram_spec_error(spec, sp) || ngram_list_error(pat_ids, pat_offsets, n_pats, lengths))
        return TD_E_INVALID;
    if (tok_offsets[0] != 0) return TD_E_INVALID;
    for (int64_t d = 0; d < n_docs; ++d)
        if (tok_offsets[d + 1] < tok_offsets[d]) return TD_E_INVALID;
    if (tok_offsets[n_docs] > n_tokens || (tok_offsets[n_docs] > 0 && !ids)) return TD_E_INVALID;
    // a sequence's ids as a string of bytes -> its lowest index
    std::unordered_map<std::string, int64_t> first;
    for (int64_t p = n_pats - 1; p >= 0; --p)
        first[std::string((const char*)(pat_ids + pat_offsets[p]), (size_t)(pat_offsets[p + 1] - pat_offsets[p]) * 4)] = p;
    if (pattern_counts && !sp.accumulate) memset(pattern_counts, 0, (size_t)n_pats * 8);
    memset(counts, 0, 4 * sizeof(int64_t));
    for (int64_t d = 0; d < n_docs; ++d) {
        const int64_t a = tok_offsets[d], z = tok_offsets[d + 1];
        int64_t occ = 0, cov = 0, reach = a;  // reach: the furthest end of the occurrences that start at or below the position
        for (int64_t q = a; q < z; ++q) {
            for (const int k : lengths) {
                if (q + k > z) break;
                const auto it = first.find(std::string((const char*)(ids + q), (size_t)k * 4));
                if (it == first.end()) continue;
                ++occ;
                if (pattern_counts) ++pattern_counts[it->second];
                reach = std::max(reach, q + k);
            }
            const bool c = reach > q;
            cov += c;
            if (cover) cover[q] = c;
            if (labels && c) labels[q] = sp.ignore;
        }
        if (doc_stats) {
            doc_stats[2 * d] = occ;
            doc_stats[2 * d + 1] = cov;
        }
        counts[0] += occ;
        counts[1] += cov;
        counts[2] += occ > 0;
    }
    return TD_OK;
}

int td_ngram_matches_device(td_tokenizer* t, const td_ngram_set* set, const void* d_ids, int64_t n_tokens, const void* d_tok_offsets,
                            int64_t n_docs, const td_ngram_spec* spec, void* d_cover, void* d_labels, void* d_doc_stats,
                            void* d_pattern_counts, void* d_counts, void* hip_stream) {
    if (!t || !set || n_tokens < 0 || n_docs < 0 || !d_tok_offsets || (n_tokens > 0 && !d_ids) || !d_counts ||
        ((((uintptr_t)d_counts) | ((uintptr_t)d_doc_stats) | ((uintptr_t)d_pattern_counts)) & 7))
        return TD_E_INVALID;
    NgSpec sp;
    if (const char* m = ngram_spec_error(spec, sp)) return fail_unlocked(t, TD_E_INVALID, std::string("td_ngram_matches_device: ") + m);
    if (int rc = ngram_set_check(t, "td_ngram_matches_device", set)) return rc;
    return locked(t, [&] {
        return ngram_matches_locked(t, set, d_ids, n_tokens, d_tok_offsets, n_docs, sp, d_cover, d_labels, d_doc_stats, d_pattern_counts, d_counts,
                                    (hipStream_t)hip_stream);
    });
}

int td_ngram_matches(td_tokenizer* t, const td_ngram_set* set, const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets,
                     int64_t n_docs, const td_ngram_spec* spec, uint8_t* cover, int32_t* labels, int64_t* doc_stats,
                     int64_t* pattern_counts, int64_t* counts) {
    if (!t || !set || n_tokens < 0 || n_docs < 0 || !tok_offsets || !counts) return TD_E_INVALID;
    NgSpec sp;
    if (const char* m = ngram_spec_error(spec, sp)) return fail_unlocked(t, TD_E_INVALID, std::string("td_ngram_matches: ") + m);
    if (int rc = ngram_set_check(t, "td_ngram_matches", set)) return rc;
    return locked(t, [&] {
        int rc;
        if ((rc = rows_check_host_ids(t, ids, n_tokens, tok_offsets, n_docs))) return rc;
        hipStream_t s;
        if ((rc = rows_stage_host_ids(t, ids, tok_offsets, n_docs, s))) return rc;
        return ngram_to_host(t, set, t->dec_tokens.p, tok_offsets[n_docs], t->d_offsets.p, n_docs, sp, cover, labels, doc_stats, pattern_counts,
                             counts, s);
    });
}

int td_encode_batch_ngram_matches(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode,
                                  const td_ngram_set* set, const td_ngram_spec* spec, int64_t* doc_stats, int64_t* pattern_counts,
                                  int64_t* counts, int64_t* n_tokens_out) {
    if (!t || !set || !doc_offsets || n_docs < 0 || !counts || (mode != TD_MODE_ENCODE && mode != TD_MODE_ORDINARY)) return TD_E_INVALID;
    NgSpec sp;
    if (const char* m = ngram_spec_error(spec, sp)) return fail_unlocked(t, TD_E_INVALID, std::string("td_encode_batch_ngram_matches: ") + m);
    if (int rc = ngram_set_check(t, "td_encode_batch_ngram_matches", set)) return rc;
    return locked(t, [&] {
        int rc;
        int64_t dev_cap;
        hipStream_t s;
        if ((rc = rows_encode_locked(t, text, doc_offsets, n_docs, mode, dev_cap, s))) return rc;
        // the ids made: eight bytes come back, they size the grid and are the caller's total
        int64_t total = 0;
        if ((rc = copy_wait(t, &total, (const int64_t*)t->d_offsets.p + n_docs, 8, hipMemcpyDeviceToHost, s))) return rc;
        if (n_tokens_out) *n_tokens_out = total;
        if (total < 0 || total > dev_cap) { t->err = "the encode's token total is outside its buffer"; return (int)TD_E_INVALID; }
        return ngram_to_host(t, set, t->d_tokens.p, total, t->d_offsets.p, n_docs, sp, nullptr, nullptr, doc_stats, pattern_counts, counts, s);
    });
}

}  // extern "C"
