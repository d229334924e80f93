// Token counts (td_counts.hip): the spec's checks, the contract's host statement and the entry points.
#include "td_counts.h"
#include "td_handle.h"

namespace {

struct CntSpec {
    int64_t n_bins, n_groups;
    bool accumulate;
    int64_t keys() const { return n_bins * n_groups; }
};

// (has: the caller gave tok_offsets and doc_group)
const char* counts_spec_error(const td_counts_spec* sp, bool has_docs, int64_t n_tokens, int64_t n_docs, CntSpec& out) {
    if (!sp) return "null td_counts_spec";
    if (sp->n_bins < 1) return "n_bins must be at least 1";
    if (sp->n_groups < 1) return "n_groups must be at least 1";
    if (sp->n_bins > CNT_MAX_KEYS || sp->n_groups > CNT_MAX_KEYS || sp->n_bins * sp->n_groups > CNT_MAX_KEYS)
        return "n_groups * n_bins must be at most 2^28";
    if (sp->flags & ~(int64_t)TD_COUNTS_ACCUMULATE) return "flags must be 0 or TD_COUNTS_ACCUMULATE";
    if (n_tokens < 0 || n_docs < 0) return "negative n_tokens or n_docs";
    if (sp->n_groups > 1 && !has_docs) return "n_groups > 1 needs tok_offsets and doc_group";
    out.n_bins = sp->n_bins;
    out.n_groups = sp->n_groups;
    out.accumulate = (sp->flags & TD_COUNTS_ACCUMULATE) != 0;
    return nullptr;
}

// the lowest document whose group is outside [0, n_groups), or -1
int64_t first_bad_group(const int32_t* doc_group, int64_t n_docs, int64_t n_groups) {
    for (int64_t d = 0; d < n_docs; ++d)
        if (doc_group[d] < 0 || doc_group[d] >= n_groups) return d;
    return -1;
}

// Enqueues the zeroing and the kernel on `s`.  d_toff and d_group: both null = one group, positions [0, n_tokens); else both given.
int counts_launch_locked(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_toff, int64_t n_docs, const void* d_group,
                         const CntSpec& sp, void* d_counts, void* d_info, hipStream_t s) {
    int rc;
    if ((rc = order_before(t, s))) return rc;
    CountsArgs a;
    memset(&a, 0, sizeof a);
    a.ids = (const int32_t*)d_ids;
    a.n_tokens = n_tokens;
    a.tok_off = (const int64_t*)d_toff;
    a.n_docs = n_docs;
    a.doc_group = (const int32_t*)d_group;
    a.n_bins = sp.n_bins;
    a.n_groups = sp.n_groups;
    int bits = 0;
    while ((1 << bits) < CNT_SEATS) ++bits;
    a.seat_bits = t->opt.counts_seat_bits ? t->opt.counts_seat_bits : bits;
    a.flush_tiles = t->opt.counts_flush_tiles ? t->opt.counts_flush_tiles : CNT_FLUSH_TILES;
    a.counts = (unsigned long long*)d_counts;
    a.info = (unsigned long long*)d_info;
    Ctl* ctl = (Ctl*)t->ctl.p;
    a.err = &ctl->err;
    a.err_pos = &ctl->err_pos;
    if (!sp.accumulate) HIP_TRY(t, hipMemsetAsync(d_counts, 0, (size_t)sp.keys() * 8, s));
    HIP_TRY(t, hipMemsetAsync(d_info, 0, 4 * sizeof(int64_t), s));
    HIP_TRY(t, launch_token_counts(a, s));
    return order_after(t, s);
}

// The host forms' end: the kernel into the handle's counts and info (zeroed), its status, then both to the caller; with
// TD_COUNTS_ACCUMULATE the counts are added to the caller's on the host.
int counts_to_host(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_toff, int64_t n_docs, const void* d_group,
                   const CntSpec& sp, int64_t* counts, int64_t* info, hipStream_t s) {
    int rc;
    const size_t bytes = (size_t)sp.keys() * 8;
    if ((rc = ensure(t, t->cnt_counts, bytes))) return rc;
    if ((rc = ensure(t, t->cnt_info, 4 * sizeof(int64_t)))) return rc;
    CntSpec fresh = sp;
    fresh.accumulate = false;
    if ((rc = counts_launch_locked(t, d_ids, n_tokens, d_toff, n_docs, d_group, fresh, t->cnt_counts.p, t->cnt_info.p, s))) return rc;
    if ((rc = device_status_locked(t, s, nullptr))) return rc;
    if ((rc = copy_wait(t, info, t->cnt_info.p, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, s))) return rc;
    if (!sp.accumulate) return copy_wait(t, counts, t->cnt_counts.p, bytes, hipMemcpyDeviceToHost, s);
    std::unique_ptr<int64_t[]> got(new int64_t[(size_t)sp.keys()]);
    if ((rc = copy_wait(t, got.get(), t->cnt_counts.p, bytes, hipMemcpyDeviceToHost, s))) return rc;
    for (int64_t k = 0; k < sp.keys(); ++k) counts[k] += got[(size_t)k];
    return TD_OK;
}

// the caller's groups behind its ids and offsets, on the same stream
int counts_stage_groups(td_tokenizer* t, const int32_t* doc_group, int64_t n_docs, hipStream_t s) {
    int rc;
    if ((rc = ensure(t, t->cnt_groups, (size_t)std::max<int64_t>(n_docs, 1) * 4))) return rc;
    if (n_docs > 0) HIP_TRY(t, hipMemcpyAsync(t->cnt_groups.p, doc_group, (size_t)n_docs * 4, hipMemcpyHostToDevice, s));
    return TD_OK;
}

int counts_bad_group_locked(td_tokenizer* t, const int32_t* doc_group, int64_t n_docs, int64_t n_groups) {
    const int64_t d = first_bad_group(doc_group, n_docs, n_groups);
    if (d < 0) return TD_OK;
    t->err = "doc_group[" + std::to_string(d) + "] = " + std::to_string(doc_group[d]) + " is outside [0, n_groups)";
    return TD_E_INVALID;
}

}  // namespace

extern "C" {

int td_token_counts_host(const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets, int64_t n_docs, const int32_t* doc_group,
                         const td_counts_spec* spec, int64_t* counts, int64_t* info) {
    if (!info) return TD_E_INVALID;
    info[0] = -1;
    info[1] = info[2] = info[3] = 0;
    CntSpec sp;
    if (!counts || counts_spec_error(spec, tok_offsets && doc_group, n_tokens, n_docs, sp)) return TD_E_INVALID;
    const bool groups = sp.n_groups > 1;
    int64_t lo = 0, hi = n_tokens;
    if (groups) {
        if (tok_offsets[0] < 0) return TD_E_INVALID;
        for (int64_t d = 0; d < n_docs; ++d)
            if (tok_offsets[d + 1] < tok_offsets[d]) return TD_E_INVALID;
        if (tok_offsets[n_docs] > n_tokens) return TD_E_INVALID;
        lo = tok_offsets[0];
        hi = tok_offsets[n_docs];
        const int64_t bad = first_bad_group(doc_group, n_docs, sp.n_groups);
        if (bad >= 0) {
            info[0] = bad;
            return TD_E_INVALID;
        }
    }
    if (hi > lo && !ids) return TD_E_INVALID;
    if (!sp.accumulate) memset(counts, 0, (size_t)sp.keys() * 8);
    int64_t counted = 0, negative = 0, too_large = 0;
    const auto visit = [&](int64_t from, int64_t to, int64_t g) {
        for (int64_t i = from; i < to; ++i) {
            const int32_t v = ids[i];
            if (v < 0) ++negative;
            else if (v >= sp.n_bins) ++too_large;
            else {
                ++counted;
                ++counts[g * sp.n_bins + v];
            }
        }
    };
    if (groups)
        for (int64_t d = 0; d < n_docs; ++d) visit(tok_offsets[d], tok_offsets[d + 1], doc_group[d]);
    else
        visit(lo, hi, 0);
    info[0] = counted;
    info[1] = negative;
    info[2] = too_large;
    info[3] = 0;  // (a bad group is an error here)
    return TD_OK;
}

int td_token_counts_device(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_tok_offsets, int64_t n_docs,
                           const void* d_doc_group, const td_counts_spec* spec, void* d_counts, void* d_info, void* hip_stream) {
    if (!t || !d_counts || !d_info || ((((uintptr_t)d_counts) | ((uintptr_t)d_info)) & 7) || (n_tokens > 0 && !d_ids)) return TD_E_INVALID;
    CntSpec sp;
    if (const char* m = counts_spec_error(spec, d_tok_offsets && d_doc_group, n_tokens, n_docs, sp))
        return fail_unlocked(t, TD_E_INVALID, std::string("td_token_counts_device: ") + m);
    const bool groups = sp.n_groups > 1;
    return locked(t, [&] {
        return counts_launch_locked(t, d_ids, n_tokens, groups ? d_tok_offsets : nullptr, groups ? n_docs : 0, groups ? d_doc_group : nullptr, sp,
                                    d_counts, d_info, (hipStream_t)hip_stream);
    });
}

int td_token_counts(td_tokenizer* t, const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets, int64_t n_docs,
                    const int32_t* doc_group, const td_counts_spec* spec, int64_t* counts, int64_t* info) {
    if (!t || !counts || !info) return TD_E_INVALID;
    CntSpec sp;
    if (const char* m = counts_spec_error(spec, tok_offsets && doc_group, n_tokens, n_docs, sp))
        return fail_unlocked(t, TD_E_INVALID, std::string("td_token_counts: ") + m);
    if (n_tokens > 0 && !ids) return fail_unlocked(t, TD_E_INVALID, "td_token_counts: null ids");
    const bool groups = sp.n_groups > 1;
    return locked(t, [&] {
        int rc;
        const int64_t whole[2] = {0, n_tokens};  // one group: every position, as one document
        const int64_t* offs = groups ? tok_offsets : whole;
        const int64_t docs = groups ? n_docs : 1;
        if ((rc = rows_check_host_ids(t, ids, n_tokens, offs, docs))) return rc;
        if (groups && (rc = counts_bad_group_locked(t, doc_group, n_docs, sp.n_groups))) return rc;
        hipStream_t s;
        if ((rc = rows_stage_host_ids(t, ids, offs, docs, s))) return rc;
        if (groups && (rc = counts_stage_groups(t, doc_group, n_docs, s))) return rc;
        return counts_to_host(t, t->dec_tokens.p, offs[docs], groups ? t->d_offsets.p : nullptr, groups ? n_docs : 0,
                              groups ? t->cnt_groups.p : nullptr, sp, counts, info, s);
    });
}

int td_encode_batch_token_counts(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode,
                                 const int32_t* doc_group, const td_counts_spec* spec, int64_t* counts, int64_t* info,
                                 int64_t* n_tokens_out) {
    if (!t || !doc_offsets || n_docs < 0 || !counts || !info || (mode != TD_MODE_ENCODE && mode != TD_MODE_ORDINARY)) return TD_E_INVALID;
    CntSpec sp;
    if (const char* m = counts_spec_error(spec, doc_group != nullptr, 0, n_docs, sp))
        return fail_unlocked(t, TD_E_INVALID, std::string("td_encode_batch_token_counts: ") + m);
    const bool groups = sp.n_groups > 1;
    return locked(t, [&] {
        int rc;
        if (groups && (rc = counts_bad_group_locked(t, doc_group, n_docs, sp.n_groups))) return rc;
        int64_t dev_cap;
        hipStream_t s;
        if ((rc = rows_encode_locked(t, text, doc_offsets, n_docs, mode, dev_cap, s))) return rc;
        // the ids made: eight bytes come back, they size the grid and are the caller's total
        int64_t total = 0;
        if ((rc = copy_wait(t, &total, (const int64_t*)t->d_offsets.p + n_docs, 8, hipMemcpyDeviceToHost, s))) return rc;
        if (n_tokens_out) *n_tokens_out = total;
        if (total < 0 || total > dev_cap) { t->err = "the encode's token total is outside its buffer"; return (int)TD_E_INVALID; }
        if (groups && (rc = counts_stage_groups(t, doc_group, n_docs, s))) return rc;
        // (the encode's buffer is larger than its ids: `total` bounds the positions, with one group as with several)
        return counts_to_host(t, t->d_tokens.p, total, groups ? t->d_offsets.p : nullptr, groups ? n_docs : 0,
                              groups ? t->cnt_groups.p : nullptr, sp, counts, info, s);
    });
}

}  // extern "C"
