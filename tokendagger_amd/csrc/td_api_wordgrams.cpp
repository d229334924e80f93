// Per-document word n-gram repetition statistics (td_wordgrams.hip): the contract's host statement and the entry points.
#include "td_handle.h"
#include "td_wordgrams.h"

namespace {

static_assert(TD_WG_COLS == WG_COLS && TD_WG_TOP == WG_TOP && TD_WG_DUP == WG_DUP && TD_WG_NO_LDS == WG_NO_LDS,
              "the header's constants are the kernels'");

int word_ngrams_locked(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_off, int64_t n_docs, int groups, int flags,
                       int64_t max_words, void* d_stats, void* d_totals, hipStream_t s) {
    int rc;
    WgArgs a;
    memset(&a, 0, sizeof a);
    a.groups = groups;
    a.wflags = flags;
    a.max_units = max_words > 0 ? max_words : wg_default_words(n_bytes, n_docs);
    a.stats = (unsigned long long*)d_stats;
    a.totals = (unsigned long long*)d_totals;
    const size_t words = (size_t)a.max_units, slots = (size_t)rp_slots(a.max_units), docs = (size_t)n_docs + 1;
    struct { DevBuf* b; size_t bytes; } const bufs[] = {
        {&t->wg_carry, (size_t)((n_bytes + 16 + RW_TILE - 1) / RW_TILE + 1) * 2 * sizeof(RpElem)},
        {&t->wg_rec, words * sizeof(WgWord)}, {&t->wg_cum, (words + 1) * 8}, {&t->wg_first, docs * 8}, {&t->wg_table, slots * 8},
        {&t->wg_cnt, slots * 8}, {&t->wg_occ, words * 8}, {&t->wg_flag, words}, {&t->wg_long_doc, docs * 8},
        {&t->wg_long_first, docs * 8}, {&t->wg_lhead, WG_L_HEAD * 8}};
    for (const auto& x : bufs)
        if ((rc = ensure(t, *x.b, x.bytes))) return rc;
    a.carry = (RpElem*)t->wg_carry.p;
    a.rec = (WgWord*)t->wg_rec.p;
    a.cum = (unsigned long long*)t->wg_cum.p;
    a.first_word = (long long*)t->wg_first.p;
    a.table = (unsigned long long*)t->wg_table.p;
    a.cnt = (unsigned long long*)t->wg_cnt.p;
    a.occ = (unsigned long long*)t->wg_occ.p;
    a.flag = (uint8_t*)t->wg_flag.p;
    a.long_doc = (long long*)t->wg_long_doc.p;
    a.long_first = (long long*)t->wg_long_first.p;
    a.lhead = (unsigned long long*)t->wg_lhead.p;
    return rewrite_check_locked(t, t->wordgrams, a, {d_text, n_bytes, d_off, n_docs, nullptr, nullptr, nullptr, 0, nullptr}, s, [&]() -> int {
        // (debugging, TD_OPT_WS_FILL: a record, a slot or a flag nobody wrote reads as the chosen byte)
        if (t->opt.ws_fill >= 0)
            for (const auto& x : bufs) {
                HIP_TRY(t, hipMemsetAsync(x.b->p, t->opt.ws_fill, x.b->cap, s));
                t->ws_filled += (int64_t)x.b->cap;
            }
        HIP_TRY(t, launch_word_ngrams(a, s));
        return (int)TD_OK;
    });
}

const char* check_call(int64_t n_bytes, int groups, int flags, int64_t max_words) {
    if (!wg_groups_ok(groups)) return "groups must be TD_WG_TOP, TD_WG_DUP or both";
    if (!wg_flags_ok(flags)) return "flags must be 0 or TD_WG_NO_LDS";
    if (n_bytes >= RP_MAX_BYTES) return "the text must be shorter than 2^40 bytes";
    if (max_words < 0 || max_words > RP_MAX_BYTES) return "max_words must be 0 or a count of words";
    return nullptr;
}

}  // namespace

extern "C" {

int td_word_ngrams_host(const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int groups, int64_t* stats, int64_t* totals) {
    return wg_host(text, doc_offsets, n_docs, groups, stats, totals) ? TD_E_INVALID : TD_OK;
}

int td_word_ngrams_device(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_doc_offsets, int64_t n_docs, int groups,
                          int flags, int64_t max_words, void* d_stats, void* d_totals, void* hip_stream) {
    if (!t || n_bytes < 0 || n_docs < 0 || !d_doc_offsets || (n_bytes > 0 && !d_text) || (n_docs > 0 && !d_stats) ||
        ((((uintptr_t)d_stats) | ((uintptr_t)d_doc_offsets) | ((uintptr_t)d_totals)) & 7))
        return TD_E_INVALID;
    if (const char* why = check_call(n_bytes, groups, flags, max_words)) return fail_unlocked(t, TD_E_INVALID, std::string("td_word_ngrams_device: ") + why);
    if (!hip_stream) return fail_unlocked(t, TD_E_INVALID, "td_word_ngrams_device: hip_stream must not be the null stream");
    return locked(t, [&] {
        return word_ngrams_locked(t, d_text, n_bytes, d_doc_offsets, n_docs, groups, flags, max_words, d_stats, d_totals, (hipStream_t)hip_stream);
    });
}

int td_word_ngrams(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int groups, int64_t* stats, int64_t* totals) {
    if (!t || !doc_offsets || n_docs < 0 || (n_docs > 0 && !stats)) return TD_E_INVALID;
    if (const char* why = check_call(0, groups, 0, 0)) return fail_unlocked(t, TD_E_INVALID, std::string("td_word_ngrams: ") + why);
    return locked(t, [&] {
        int rc;
        hipStream_t s;
        if ((rc = stage_host_text(t, text, doc_offsets, n_docs, s))) return rc;
        const int64_t n = doc_offsets[n_docs];
        if (const char* why = check_call(n, groups, 0, 0)) { t->err = std::string("td_word_ngrams: ") + why; return (int)TD_E_INVALID; }
        const size_t row = WG_COLS * 8;
        if ((rc = ensure(t, t->wg_stats, (size_t)std::max<int64_t>(n_docs, 1) * row))) return rc;
        if ((rc = ensure(t, t->wg_totals, row))) return rc;
        int64_t max_words = 0, need = 0;
        for (int round = 0;; ++round) {  // once more with the need the first call reported
            if ((rc = word_ngrams_locked(t, t->h2d_text.p, n, t->h2d_offs.p, n_docs, groups, 0, max_words, t->wg_stats.p, t->wg_totals.p, s))) return rc;
            rc = device_status_locked(t, s, &need);
            if (rc != TD_E_CAPACITY || round > 0 || need <= 0) break;
            max_words = need;
        }
        if (rc) return rc;
        if (n_docs > 0 && (rc = copy_wait(t, stats, t->wg_stats.p, (size_t)n_docs * row, hipMemcpyDeviceToHost, s))) return rc;
        return totals ? copy_wait(t, totals, t->wg_totals.p, row, hipMemcpyDeviceToHost, s) : (int)TD_OK;
    });
}

}  // extern "C"
