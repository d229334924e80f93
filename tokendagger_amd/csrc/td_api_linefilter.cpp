// Line filtering (td_linefilter.hip): the contract's host statement and the entry points.
#include "td_handle.h"
#include "td_linefilter.h"

namespace {

// One launch sequence on `s`.  d_out null: nothing is held against a capacity and no byte is written; d_out_off null: the offsets go
// to the handle's own; with both null and the write phase asked for, that phase is left out.
int filter_locked(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_off, int64_t n_docs, const td_line_rules* rules,
                  void* d_out, int64_t out_capacity, void* d_out_off, void* d_stats, void* d_totals, void* d_counts, hipStream_t s, int phases) {
    int rc;
    const size_t tiles1 = (size_t)((n_bytes + 16 + RW_TILE - 1) / RW_TILE + 1);
    if ((rc = ensure(t, t->lf_elems, tiles1 * sizeof(LfElem<int64_t>)))) return rc;
    if ((rc = ensure(t, t->lf_carry, tiles1 * 2 * sizeof(LfPiece<int64_t>)))) return rc;
    if ((rc = ensure(t, t->lf_masks, tiles1 * RW_THREADS * sizeof(uint16_t)))) return rc;
    if (!d_out && !d_out_off) phases &= ~RW_RUN_WRITE;
    if (!d_out_off) {
        if ((rc = ensure(t, t->linefilter.out_off, (size_t)(n_docs + 1) * 8))) return rc;
        d_out_off = t->linefilter.out_off.p;
    }
    LfArgs a;
    memset(&a, 0, sizeof a);
    a.rules = *rules;
    a.stats = (unsigned long long*)d_stats;
    a.totals = (unsigned long long*)d_totals;
    a.elems = (LfElem<int64_t>*)t->lf_elems.p;
    a.carry = (LfPiece<int64_t>*)t->lf_carry.p;
    a.masks = (uint16_t*)t->lf_masks.p;
    return rewrite_locked(t, t->linefilter, a, {d_text, n_bytes, d_off, n_docs, nullptr, d_counts, d_out, d_out ? out_capacity : INT64_MAX, d_out_off},
                          phases, s, [&]() -> int {
                              HIP_TRY(t, launch_linefilter(a, s, phases));
                              return (int)TD_OK;
                          });
}

}  // namespace

extern "C" {

int td_line_filter_host(const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, const td_line_rules* rules, uint8_t* out,
                        int64_t out_capacity, int64_t* out_doc_offsets, int64_t* stats, int64_t* totals) {
    if (!out && out_capacity != 0) return TD_E_INVALID;
    const int rc = lf_host(text, doc_offsets, n_docs, rules, out, out_capacity, out_doc_offsets, stats, totals, nullptr);
    return rc == LF_HOST_OK ? TD_OK : rc == LF_HOST_CAPACITY ? TD_E_CAPACITY : TD_E_INVALID;
}

int td_line_filter_device(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_doc_offsets, int64_t n_docs,
                          const td_line_rules* rules, void* d_out, int64_t out_capacity, void* d_out_doc_offsets, void* d_stats,
                          void* d_totals, void* d_counts, void* hip_stream) {
    if (!t || n_bytes < 0 || n_docs < 0 || out_capacity < 0 || !d_doc_offsets || (n_bytes > 0 && !d_text) || (out_capacity > 0 && !d_out) ||
        (n_docs > 0 && !d_stats) || !d_counts ||
        ((((uintptr_t)d_counts) | ((uintptr_t)d_doc_offsets) | ((uintptr_t)d_out_doc_offsets) | ((uintptr_t)d_stats) | ((uintptr_t)d_totals)) & 7))
        return TD_E_INVALID;
    if (!lf_rules_ok(rules)) return fail_unlocked(t, TD_E_INVALID, "td_line_filter_device: the rules are not valid");
    if (rewrite_overlap(d_text, n_bytes, d_out, out_capacity)) return fail_unlocked(t, TD_E_INVALID, "td_line_filter_device: d_out overlaps d_text");
    if (!hip_stream) return fail_unlocked(t, TD_E_INVALID, "td_line_filter_device: hip_stream must not be the null stream");
    return locked(t, [&] {
        return filter_locked(t, d_text, n_bytes, d_doc_offsets, n_docs, rules, d_out, out_capacity, d_out_doc_offsets, d_stats, d_totals,
                             d_counts, (hipStream_t)hip_stream, RW_RUN_MEASURE | RW_RUN_WRITE);
    });
}

int td_line_filter(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, const td_line_rules* rules, uint8_t* out,
                   int64_t out_capacity, int64_t* out_doc_offsets, int64_t* stats, int64_t* totals) {
    if (!t || !doc_offsets || n_docs < 0 || out_capacity < 0 || (!out && out_capacity != 0) || (n_docs > 0 && !stats)) return TD_E_INVALID;
    if (!lf_rules_ok(rules)) return fail_unlocked(t, TD_E_INVALID, "td_line_filter: the rules are not valid");
    return locked(t, [&] {
        int rc;
        hipStream_t s;
        if ((rc = stage_host_text(t, text, doc_offsets, n_docs, s))) return rc;
        const int64_t n = doc_offsets[n_docs];
        if (rewrite_overlap(text, n, out, out_capacity)) { t->err = "td_line_filter: out overlaps text"; return (int)TD_E_INVALID; }
        const size_t docs = (size_t)n_docs, row = LF_COLS * 8;
        if ((rc = ensure(t, t->lf_stats, std::max<size_t>(docs, 1) * row))) return rc;
        if ((rc = ensure(t, t->lf_totals, row))) return rc;
        int64_t counts[RW_C_WORDS];
        if ((rc = rewrite_staged(t, t->linefilter, n, n_docs, counts, out || out_doc_offsets, "line filter", s,
                                 [&](void* d_out, int64_t cap, int phases) {
                                     return filter_locked(t, t->h2d_text.p, n, t->h2d_offs.p, n_docs, rules, d_out, cap, t->linefilter.out_off.p,
                                                          t->lf_stats.p, t->lf_totals.p, t->linefilter.counts.p, s, phases);
                                 })))
            return rc;
        if (out && counts[RW_C_BYTES] > out_capacity) {
            t->err = "output capacity too small: " + std::to_string(counts[RW_C_BYTES]) + " bytes needed";
            return (int)TD_E_CAPACITY;
        }
        if (docs && (rc = copy_wait(t, stats, t->lf_stats.p, docs * row, hipMemcpyDeviceToHost, s))) return rc;
        if (totals && (rc = copy_wait(t, totals, t->lf_totals.p, row, hipMemcpyDeviceToHost, s))) return rc;
        if (out_doc_offsets && (rc = copy_wait(t, out_doc_offsets, t->linefilter.out_off.p, (docs + 1) * 8, hipMemcpyDeviceToHost, s))) return rc;
        if (!out) return (int)TD_OK;
        return copy_wait(t, out, t->linefilter.out.p, (size_t)counts[RW_C_BYTES], hipMemcpyDeviceToHost, s);
    });
}

}  // extern "C"
