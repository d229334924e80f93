// Per-document text statistics (td_textstats.hip): the contract's host statement and the entry points.
#include "td_handle.h"
#include "td_textstats.h"

namespace {

static_assert(TD_TS_COLS == TS_COLS && TD_TS_LOCAL == TS_LOCAL && TD_TS_RUNS == TS_RUNS, "the header's constants are the kernels'");

int stats_locked(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_off, int64_t n_docs, int groups, void* d_stats,
                 void* d_totals, hipStream_t s) {
    int rc;
    // (td_create uploads the class tables for every pattern kind, the generic one included: a handle without them is not one of its)
    if (!t->dT.ascii_cls || !t->dT.ucls1 || !t->dT.ucls2) { t->err = "the handle has no class tables on the device"; return TD_E_INVALID; }
    TsArgs a;
    memset(&a, 0, sizeof a);
    a.ascii_cls = t->dT.ascii_cls;
    a.ucls1 = t->dT.ucls1;
    a.ucls2 = t->dT.ucls2;
    a.groups = groups;
    a.stats = (unsigned long long*)d_stats;
    a.totals = (unsigned long long*)d_totals;
    if (groups & TS_RUNS) {
        if ((rc = ensure(t, t->ts_carry, (size_t)((n_bytes + 16 + RW_TILE - 1) / RW_TILE + 1) * 32))) return rc;
        a.carry = (long long*)t->ts_carry.p;
    }
    return rewrite_check_locked(t, t->textstats, a, {d_text, n_bytes, d_off, n_docs, nullptr, nullptr, nullptr, 0, nullptr}, s, [&]() -> int {
        // (debugging, TD_OPT_WS_FILL: a carry nobody wrote reads as the chosen byte)
        if (t->opt.ws_fill >= 0 && a.carry) {
            HIP_TRY(t, hipMemsetAsync(t->ts_carry.p, t->opt.ws_fill, t->ts_carry.cap, s));
            t->ws_filled += (int64_t)t->ts_carry.cap;
        }
        HIP_TRY(t, launch_textstats(a, s));
        return (int)TD_OK;
    });
}

// h2d_text / h2d_offs into ts_stats and ts_totals, the status, then both to the caller
int stats_staged(td_tokenizer* t, int64_t n, int64_t n_docs, int groups, int64_t* stats, int64_t* totals, hipStream_t s) {
    int rc;
    const size_t row = TS_COLS * 8;
    if ((rc = ensure(t, t->ts_stats, (size_t)std::max<int64_t>(n_docs, 1) * row))) return rc;
    if ((rc = ensure(t, t->ts_totals, row))) return rc;
    if ((rc = stats_locked(t, t->h2d_text.p, n, t->h2d_offs.p, n_docs, groups, t->ts_stats.p, t->ts_totals.p, s))) return rc;
    if ((rc = device_status_locked(t, s, nullptr))) return rc;
    if (n_docs > 0 && (rc = copy_wait(t, stats, t->ts_stats.p, (size_t)n_docs * row, hipMemcpyDeviceToHost, s))) return rc;
    return totals ? copy_wait(t, totals, t->ts_totals.p, row, hipMemcpyDeviceToHost, s) : (int)TD_OK;
}

}  // namespace

extern "C" {

int td_text_stats_host(const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int groups, int64_t* stats, int64_t* totals) {
    return ts_host(class_tables(), text, doc_offsets, n_docs, groups, stats, totals) ? TD_E_INVALID : TD_OK;
}

int td_text_stats_device(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_doc_offsets, int64_t n_docs, int groups,
                         void* d_stats, void* d_totals, void* hip_stream) {
    if (!t || n_bytes < 0 || n_docs < 0 || !d_doc_offsets || (n_bytes > 0 && !d_text) || (n_docs > 0 && !d_stats) ||
        ((((uintptr_t)d_stats) | ((uintptr_t)d_doc_offsets) | ((uintptr_t)d_totals)) & 7))
        return TD_E_INVALID;
    if (!ts_groups_ok(groups)) return fail_unlocked(t, TD_E_INVALID, "td_text_stats_device: groups must be TD_TS_LOCAL, TD_TS_RUNS or both");
    if (!hip_stream) return fail_unlocked(t, TD_E_INVALID, "td_text_stats_device: hip_stream must not be the null stream");
    return locked(t, [&] { return stats_locked(t, d_text, n_bytes, d_doc_offsets, n_docs, groups, d_stats, d_totals, (hipStream_t)hip_stream); });
}

int td_text_stats(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int groups, int64_t* stats, int64_t* totals) {
    if (!t || !doc_offsets || n_docs < 0 || (n_docs > 0 && !stats)) return TD_E_INVALID;
    if (!ts_groups_ok(groups)) return fail_unlocked(t, TD_E_INVALID, "td_text_stats: groups must be TD_TS_LOCAL, TD_TS_RUNS or both");
    return locked(t, [&] {
        int rc;
        hipStream_t s;
        if ((rc = stage_host_text(t, text, doc_offsets, n_docs, s))) return rc;
        return stats_staged(t, doc_offsets[n_docs], n_docs, groups, stats, totals, s);
    });
}

int td_encode_batch_text_stats(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode, int groups,
                               int32_t* out_ids, int64_t ids_capacity, int64_t* out_tok_offsets, int64_t* stats, int64_t* totals) {
    if (!t || !doc_offsets || !out_tok_offsets || n_docs < 0 || ids_capacity < 0 || (n_docs > 0 && !stats) ||
        (mode != TD_MODE_ENCODE && mode != TD_MODE_ORDINARY))
        return TD_E_INVALID;
    if (!ts_groups_ok(groups)) return fail_unlocked(t, TD_E_INVALID, "td_encode_batch_text_stats: groups must be TD_TS_LOCAL, TD_TS_RUNS or both");
    return locked(t, [&] {
        int rc;
        hipStream_t s;
        if ((rc = stage_host_text(t, text, doc_offsets, n_docs, s))) return rc;
        const int64_t n = doc_offsets[n_docs];
        if ((rc = stats_staged(t, n, n_docs, groups, stats, totals, s))) return rc;
        return encode_rewritten(t, text, t->h2d_text.p, t->h2d_offs.p, n, n_docs, mode, "text", nullptr, 0, out_ids, ids_capacity, out_tok_offsets, s);
    });
}

}  // extern "C"
