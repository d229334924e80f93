// Address masking (td_mask.hip): the contract's host statement and the entry points.
#include "td_handle.h"
#include "td_mask.h"

namespace {

// One launch sequence on `s`.  d_out null: nothing is held against a capacity and no byte is written; d_out_off null: the offsets go
// to the handle's own; with both null and the write phase asked for, that phase is left out.
int mask_locked(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_off, int64_t n_docs, const td_mask_rules* rules,
                void* d_out, int64_t out_capacity, void* d_out_off, void* d_stats, void* d_totals, void* d_counts, hipStream_t s, int phases) {
    int rc;
    if ((rc = ensure(t, t->ma_dirty, (size_t)((n_bytes + 16 + RW_TILE - 1) / RW_TILE + 1) * sizeof(uint32_t)))) return rc;
    if (!d_out && !d_out_off) phases &= ~RW_RUN_WRITE;
    if (!d_out_off) {
        if ((rc = ensure(t, t->mask.out_off, (size_t)(n_docs + 1) * 8))) return rc;
        d_out_off = t->mask.out_off.p;
    }
    MaArgs a;
    memset(&a, 0, sizeof a);
    a.rules = *rules;
    a.stats = (unsigned long long*)d_stats;
    a.totals = (unsigned long long*)d_totals;
    a.dirty = (uint32_t*)t->ma_dirty.p;
    return rewrite_locked(t, t->mask, a, {d_text, n_bytes, d_off, n_docs, nullptr, d_counts, d_out, d_out ? out_capacity : INT64_MAX, d_out_off},
                          phases, s, [&]() -> int {
                              HIP_TRY(t, launch_mask(a, s, phases));
                              return (int)TD_OK;
                          });
}

}  // namespace

extern "C" {

int td_mask_addresses_host(const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, const td_mask_rules* rules, uint8_t* out,
                           int64_t out_capacity, int64_t* out_doc_offsets, int64_t* stats, int64_t* totals) {
    if (!out && out_capacity != 0) return TD_E_INVALID;
    const int rc = ma_host(text, doc_offsets, n_docs, rules, out, out_capacity, out_doc_offsets, stats, totals, nullptr);
    return rc == MA_HOST_OK ? TD_OK : rc == MA_HOST_CAPACITY ? TD_E_CAPACITY : TD_E_INVALID;
}

int td_mask_addresses_device(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_doc_offsets, int64_t n_docs,
                             const td_mask_rules* rules, void* d_out, int64_t out_capacity, void* d_out_doc_offsets, void* d_stats,
                             void* d_totals, void* d_counts, void* hip_stream) {
    if (!t || n_bytes < 0 || n_docs < 0 || out_capacity < 0 || !d_doc_offsets || (n_bytes > 0 && !d_text) || (out_capacity > 0 && !d_out) ||
        (n_docs > 0 && !d_stats) || !d_counts ||
        ((((uintptr_t)d_counts) | ((uintptr_t)d_doc_offsets) | ((uintptr_t)d_out_doc_offsets) | ((uintptr_t)d_stats) | ((uintptr_t)d_totals)) & 7))
        return TD_E_INVALID;
    if (!ma_rules_ok(rules)) return fail_unlocked(t, TD_E_INVALID, "td_mask_addresses_device: the rules are not valid");
    if (rewrite_overlap(d_text, n_bytes, d_out, out_capacity))
        return fail_unlocked(t, TD_E_INVALID, "td_mask_addresses_device: d_out overlaps d_text");
    if (!hip_stream) return fail_unlocked(t, TD_E_INVALID, "td_mask_addresses_device: hip_stream must not be the null stream");
    return locked(t, [&] {
        return mask_locked(t, d_text, n_bytes, d_doc_offsets, n_docs, rules, d_out, out_capacity, d_out_doc_offsets, d_stats, d_totals,
                           d_counts, (hipStream_t)hip_stream, RW_RUN_MEASURE | RW_RUN_WRITE);
    });
}

int td_mask_addresses(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, const td_mask_rules* rules,
                      uint8_t* out, int64_t out_capacity, int64_t* out_doc_offsets, int64_t* stats, int64_t* totals) {
    if (!t || !doc_offsets || n_docs < 0 || out_capacity < 0 || (!out && out_capacity != 0) || (n_docs > 0 && !stats)) return TD_E_INVALID;
    if (!ma_rules_ok(rules)) return fail_unlocked(t, TD_E_INVALID, "td_mask_addresses: the rules are not valid");
    return locked(t, [&] {
        int rc;
        hipStream_t s;
        if ((rc = stage_host_text(t, text, doc_offsets, n_docs, s))) return rc;
        const int64_t n = doc_offsets[n_docs];
        if (rewrite_overlap(text, n, out, out_capacity)) { t->err = "td_mask_addresses: out overlaps text"; return (int)TD_E_INVALID; }
        const size_t docs = (size_t)n_docs, row = MA_COLS * 8;
        if ((rc = ensure(t, t->ma_stats, std::max<size_t>(docs, 1) * row))) return rc;
        if ((rc = ensure(t, t->ma_totals, row))) return rc;
        if ((rc = ensure(t, t->mask.out_off, (docs + 1) * 8))) return rc;
        const auto run = [&](void* d_out, int64_t cap, int phases) {
            return mask_locked(t, t->h2d_text.p, n, t->h2d_offs.p, n_docs, rules, d_out, cap, t->mask.out_off.p, t->ma_stats.p, t->ma_totals.p,
                               t->mask.counts.p, s, phases);
        };
        // measured first; the output is sized from the bytes the text needs.  (Not rewrite_staged: its bound, three times the input, is
        // the other rewrites'.  Here a match of 6 bytes can become a literal of 32.)
        int64_t counts[RW_C_WORDS];
        if ((rc = rewrite_check_staged(t, t->mask, n_docs, counts, s, [&] { return run(nullptr, INT64_MAX, RW_RUN_MEASURE); }))) return rc;
        const int64_t need = counts[RW_C_BYTES];
        if (need < 0 || need > n / MA_MATCH_MIN * TD_MA_LITERAL_BYTES + n) { t->err = "the mask's byte total is outside its bound"; return (int)TD_E_INVALID; }
        if (out && need > out_capacity) {
            t->err = "output capacity too small: " + std::to_string(need) + " bytes needed";
            return (int)TD_E_CAPACITY;
        }
        if (out || out_doc_offsets) {
            if ((rc = ensure(t, t->mask.out, (size_t)need + 64))) return rc;
            if ((rc = run(t->mask.out.p, need, RW_RUN_WRITE))) return rc;
        }
        if (docs && (rc = copy_wait(t, stats, t->ma_stats.p, docs * row, hipMemcpyDeviceToHost, s))) return rc;
        if (totals && (rc = copy_wait(t, totals, t->ma_totals.p, row, hipMemcpyDeviceToHost, s))) return rc;
        if (out_doc_offsets && (rc = copy_wait(t, out_doc_offsets, t->mask.out_off.p, (docs + 1) * 8, hipMemcpyDeviceToHost, s))) return rc;
        if (!out) return (int)TD_OK;
        return copy_wait(t, out, t->mask.out.p, (size_t)need, hipMemcpyDeviceToHost, s);
    });
}

}  // extern "C"
