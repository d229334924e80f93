// Word-list matches (td_wordlist.hip): the set (the checked list's lookup blob, built on the host), the contract's host statement and
// the entry points.
#include "td_handle.h"
#include "td_wordlist.h"

struct td_word_set {
    int device = 0;
    WlSet set{};          // blob: the device's copy
    void* blob = nullptr;
    bool resident = false;
    ~td_word_set() {
        DeviceGuard dg(device);
        if (blob) (void)hipFree(blob);
    }
};

namespace {

int matches_locked(td_tokenizer* t, const td_word_set* set, const void* d_text, int64_t n_bytes, const void* d_off, int64_t n_docs, int flags,
                   void* d_stats, void* d_totals, void* d_hits, hipStream_t s) {
    WlArgs a;
    memset(&a, 0, sizeof a);
    a.set = set->set;
    a.stats = (unsigned long long*)d_stats;
    a.totals = (unsigned long long*)d_totals;
    a.entry_hits = (unsigned long long*)d_hits;
    return rewrite_check_locked(t, t->wordlist, a, {d_text, n_bytes, d_off, n_docs, nullptr, nullptr, nullptr, 0, nullptr}, s, [&]() -> int {
        HIP_TRY(t, launch_wordlist(a, set->resident && !(flags & WL_NO_LDS), s));
        return (int)TD_OK;
    });
}

}  // namespace

extern "C" {

int td_word_set_create(td_tokenizer* t, const uint8_t* entry_bytes, const int64_t* entry_offsets, const int32_t* entry_groups,
                       int64_t n_entries, int flags, td_word_set** out, int64_t* err_pos) {
    if (err_pos) *err_pos = -1;
    if (!t || !out) return TD_E_INVALID;
    *out = nullptr;
    const WlList list = {entry_bytes, entry_offsets, entry_groups, n_entries, flags};
    int64_t pos = -1;
    if (wl_list_check(list, &pos)) {
        if (err_pos) *err_pos = pos;
        return fail_unlocked(t, TD_E_INVALID, pos < 0 ? std::string("td_word_set_create: 1 .. 65535 entries, flags of TD_WL_FOLD_ASCII | TD_WL_ANYWHERE, offsets from 0")
                                                      : "td_word_set_create: entry " + std::to_string(pos) +
                                                            " is empty, longer than 64 bytes, of a group outside 0 .. 63, upper case under TD_WL_FOLD_ASCII or a duplicate");
    }
    std::vector<uint32_t> words;
    std::unique_ptr<td_word_set> set(new td_word_set);
    set->device = t->device;
    set->set = wl_build(list, words);
    set->resident = wl_fits_lds(set->set);
    const int rc = locked(t, [&] {
        int rc;
        if ((rc = own_streams(t))) return rc;
        HIP_TRY(t, hipMalloc(&set->blob, words.size() * 4));
        return copy_wait(t, set->blob, words.data(), words.size() * 4, hipMemcpyHostToDevice, t->s_own);
    });
    if (rc) return rc;
    set->set.blob = (const uint32_t*)set->blob;
    *out = set.release();
    return TD_OK;
}

void td_word_set_destroy(td_word_set* set) { delete set; }

int64_t td_word_set_info(const td_word_set* set, int what) {
    if (!set) return -1;
    switch (what) {
        case TD_WORD_INFO_ENTRIES: return set->set.n_entries;
        case TD_WORD_INFO_MAX_LEN: return set->set.max_len;
        case TD_WORD_INFO_FLAGS: return set->set.flags;
        case TD_WORD_INFO_TABLE_BYTES: return (int64_t)set->set.blob_words * 4;
        case TD_WORD_INFO_RESIDENT: return set->resident;
    }
    return -1;
}

int td_word_matches_host(const uint8_t* entry_bytes, const int64_t* entry_offsets, const int32_t* entry_groups, int64_t n_entries, int flags,
                         const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int64_t* stats, int64_t* totals,
                         int64_t* entry_hits, int64_t* err_pos) {
    int64_t pos = -1;
    const int rc = wl_host({entry_bytes, entry_offsets, entry_groups, n_entries, flags}, text, doc_offsets, n_docs, stats, totals, entry_hits, &pos);
    if (err_pos) *err_pos = pos;
    return rc ? TD_E_INVALID : TD_OK;
}

int td_word_matches_device(td_tokenizer* t, const td_word_set* set, const void* d_text, int64_t n_bytes, const void* d_doc_offsets,
                           int64_t n_docs, int flags, void* d_stats, void* d_totals, void* d_entry_hits, void* hip_stream) {
    if (!t || !set || n_bytes < 0 || n_docs < 0 || !d_doc_offsets || (n_bytes > 0 && !d_text) || (n_docs > 0 && !d_stats) ||
        ((((uintptr_t)d_stats) | ((uintptr_t)d_doc_offsets) | ((uintptr_t)d_totals) | ((uintptr_t)d_entry_hits)) & 7))
        return TD_E_INVALID;
    if (!wl_call_flags_ok(flags)) return fail_unlocked(t, TD_E_INVALID, "td_word_matches_device: flags must be 0 or TD_WL_NO_LDS");
    if (set->device != t->device) return fail_unlocked(t, TD_E_INVALID, "td_word_matches_device: the set lives on another device");
    if (!hip_stream) return fail_unlocked(t, TD_E_INVALID, "td_word_matches_device: hip_stream must not be the null stream");
    return locked(t, [&] {
        return matches_locked(t, set, d_text, n_bytes, d_doc_offsets, n_docs, flags, d_stats, d_totals, d_entry_hits, (hipStream_t)hip_stream);
    });
}

int td_word_matches(td_tokenizer* t, const td_word_set* set, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int64_t* stats,
                    int64_t* totals, int64_t* entry_hits) {
    if (!t || !set || !doc_offsets || n_docs < 0 || (n_docs > 0 && !stats)) return TD_E_INVALID;
    if (set->device != t->device) return fail_unlocked(t, TD_E_INVALID, "td_word_matches: the set lives on another device");
    return locked(t, [&] {
        int rc;
        hipStream_t s;
        if ((rc = stage_host_text(t, text, doc_offsets, n_docs, s))) return rc;
        const size_t docs = (size_t)n_docs, row = WL_COLS * 8, hits = (size_t)set->set.n_entries * 8;
        if ((rc = ensure(t, t->wl_stats, std::max<size_t>(docs, 1) * row))) return rc;
        if ((rc = ensure(t, t->wl_totals, row))) return rc;
        if (entry_hits && (rc = ensure(t, t->wl_hits, hits))) return rc;
        if ((rc = matches_locked(t, set, t->h2d_text.p, doc_offsets[n_docs], t->h2d_offs.p, n_docs, 0, t->wl_stats.p, t->wl_totals.p,
                                 entry_hits ? t->wl_hits.p : nullptr, s)))
            return rc;
        if ((rc = device_status_locked(t, s, nullptr))) return rc;
        if (docs && (rc = copy_wait(t, stats, t->wl_stats.p, docs * row, hipMemcpyDeviceToHost, s))) return rc;
        if (totals && (rc = copy_wait(t, totals, t->wl_totals.p, row, hipMemcpyDeviceToHost, s))) return rc;
        return entry_hits ? copy_wait(t, entry_hits, t->wl_hits.p, hits, hipMemcpyDeviceToHost, s) : (int)TD_OK;
    });
}

}  // extern "C"
