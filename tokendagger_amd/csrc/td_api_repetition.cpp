// Per-document duplicate-line and duplicate-paragraph statistics (td_repetition.hip): the contract's host statement and the entry points.
#include "td_handle.h"
#include "td_repetition.h"

namespace {

static_assert(TD_RP_COLS == RP_COLS && TD_RP_LINES == RP_LINES && TD_RP_PARAS == RP_PARAS, "the header's constants are the kernels'");

int repetition_locked(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_off, int64_t n_docs, int groups, int64_t max_units,
                      void* d_stats, void* d_totals, hipStream_t s) {
    int rc;
    RpArgs a;
    memset(&a, 0, sizeof a);
    a.groups = groups;
    a.max_units = max_units > 0 ? max_units : rp_default_units(n_bytes, n_docs);
    a.stats = (unsigned long long*)d_stats;
    a.totals = (unsigned long long*)d_totals;
    if ((rc = ensure(t, t->rp_carry, (size_t)((n_bytes + 16 + RW_TILE - 1) / RW_TILE + 1) * 2 * sizeof(RpElem)))) return rc;
    if ((rc = ensure(t, t->rp_table, (size_t)rp_slots(a.max_units) * 8))) return rc;
    a.carry = (RpElem*)t->rp_carry.p;
    a.table = (unsigned long long*)t->rp_table.p;
    return rewrite_check_locked(t, t->repetition, a, {d_text, n_bytes, d_off, n_docs, nullptr, nullptr, nullptr, 0, nullptr}, s, [&]() -> int {
        // (debugging, TD_OPT_WS_FILL: a carry or a slot nobody wrote reads as the chosen byte)
        if (t->opt.ws_fill >= 0) {
            HIP_TRY(t, hipMemsetAsync(t->rp_carry.p, t->opt.ws_fill, t->rp_carry.cap, s));
            HIP_TRY(t, hipMemsetAsync(t->rp_table.p, t->opt.ws_fill, t->rp_table.cap, s));
            t->ws_filled += (int64_t)(t->rp_carry.cap + t->rp_table.cap);
        }
        HIP_TRY(t, launch_repetition(a, s));
        return (int)TD_OK;
    });
}

const char* check_call(int64_t n_bytes, int groups, int64_t max_units) {
    if (!rp_groups_ok(groups)) return "groups must be TD_RP_LINES, TD_RP_PARAS or both";
    if (n_bytes >= RP_MAX_BYTES) return "the text must be shorter than 2^40 bytes";
    if (max_units < 0 || max_units > RP_MAX_BYTES) return "max_units must be 0 or a count of units";
    return nullptr;
}

}  // namespace

extern "C" {

int td_repetition_host(const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int groups, int64_t* stats, int64_t* totals) {
    return rp_host(text, doc_offsets, n_docs, groups, stats, totals) ? TD_E_INVALID : TD_OK;
}

int td_repetition_device(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_doc_offsets, int64_t n_docs, int groups,
                         int64_t max_units, void* d_stats, void* d_totals, void* hip_stream) {
    if (!t || n_bytes < 0 || n_docs < 0 || !d_doc_offsets || (n_bytes > 0 && !d_text) || (n_docs > 0 && !d_stats) ||
        ((((uintptr_t)d_stats) | ((uintptr_t)d_doc_offsets) | ((uintptr_t)d_totals)) & 7))
        return TD_E_INVALID;
    if (const char* why = check_call(n_bytes, groups, max_units)) return fail_unlocked(t, TD_E_INVALID, std::string("td_repetition_device: ") + why);
    if (!hip_stream) return fail_unlocked(t, TD_E_INVALID, "td_repetition_device: hip_stream must not be the null stream");
    return locked(t, [&] {
        return repetition_locked(t, d_text, n_bytes, d_doc_offsets, n_docs, groups, max_units, d_stats, d_totals, (hipStream_t)hip_stream);
    });
}

int td_repetition(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int groups, int64_t* stats, int64_t* totals) {
    if (!t || !doc_offsets || n_docs < 0 || (n_docs > 0 && !stats)) return TD_E_INVALID;
    if (const char* why = check_call(0, groups, 0)) return fail_unlocked(t, TD_E_INVALID, std::string("td_repetition: ") + why);
    return locked(t, [&] {
        int rc;
        hipStream_t s;
        if ((rc = stage_host_text(t, text, doc_offsets, n_docs, s))) return rc;
        const int64_t n = doc_offsets[n_docs];
        if (const char* why = check_call(n, groups, 0)) { t->err = std::string("td_repetition: ") + why; return (int)TD_E_INVALID; }
        const size_t row = RP_COLS * 8;
        if ((rc = ensure(t, t->rp_stats, (size_t)std::max<int64_t>(n_docs, 1) * row))) return rc;
        if ((rc = ensure(t, t->rp_totals, row))) return rc;
        int64_t max_units = 0, need = 0;
        for (int round = 0;; ++round) {  // once more with the need the first call reported
            if ((rc = repetition_locked(t, t->h2d_text.p, n, t->h2d_offs.p, n_docs, groups, max_units, t->rp_stats.p, t->rp_totals.p, s))) return rc;
            rc = device_status_locked(t, s, &need);
            if (rc != TD_E_CAPACITY || round > 0 || need <= 0) break;
            max_units = need;
        }
        if (rc) return rc;
        if (n_docs > 0 && (rc = copy_wait(t, stats, t->rp_stats.p, (size_t)n_docs * row, hipMemcpyDeviceToHost, s))) return rc;
        return totals ? copy_wait(t, totals, t->rp_totals.p, row, hipMemcpyDeviceToHost, s) : (int)TD_OK;
    });
}

}  // extern "C"
