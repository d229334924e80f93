// The text rewrites (td_nfc.hip, td_utf8.hip): the host path their entry points (td_api_nfc.cpp, td_api_utf8.cpp) share.
#include "td_handle.h"

// The host forms' start: the checks of the caller's text and offsets, and their upload into h2d_text / h2d_offs on the handle's own
// stream, which `s` becomes.
int td::stage_host_text(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, hipStream_t& s) {
    int rc;
    if ((rc = check_offsets(t, "doc_offsets", doc_offsets, n_docs, text))) return rc;
    const int64_t n = doc_offsets[n_docs];
    if ((rc = ensure(t, t->h2d_text, (size_t)n + 64))) return rc;
    if ((rc = ensure(t, t->h2d_offs, (size_t)(n_docs + 1) * 8))) return rc;
    if ((rc = own_streams(t))) return rc;
    s = t->s_own;
    if ((rc = order_before(t, s))) return rc;
    if (n > 0) HIP_TRY(t, hipMemcpyAsync(t->h2d_text.p, text, (size_t)n, hipMemcpyHostToDevice, s));
    HIP_TRY(t, hipMemcpyAsync(t->h2d_offs.p, doc_offsets, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice, s));
    return TD_OK;
}

namespace {

// The start of a launch sequence: the stream's order, w's head grown, the inputs of c and where errors are raised into a.
int rewrite_begin(td_tokenizer* t, RewriteBufs& w, RewriteArgs& a, const RewriteCall& c, hipStream_t s) {
    int rc;
    if ((rc = order_before(t, s))) return rc;
    if ((rc = ensure(t, w.head, RW_H_WORDS * 8))) return rc;
    a.text = (const uint8_t*)c.d_text;
    a.n_bytes = c.n_bytes;
    a.doc_off = (const int64_t*)c.d_off;
    a.n_docs = c.n_docs;
    a.flags = (uint8_t*)c.d_flags;
    a.counts = (unsigned long long*)c.d_counts;
    a.head = (unsigned long long*)w.head.p;
    Ctl* ctl = (Ctl*)t->ctl.p;
    a.err = &ctl->err;
    a.err_pos = &ctl->err_pos;
    return TD_OK;
}

}  // namespace

int td::rewrite_check_locked(td_tokenizer* t, RewriteBufs& w, RewriteArgs& a, const RewriteCall& c, hipStream_t s, const std::function<int()>& launch) {
    int rc;
    if ((rc = rewrite_begin(t, w, a, c, s))) return rc;
    HIP_TRY(t, hipMemsetAsync(a.head, 0, RW_H_WORDS * 8, s));
    if ((rc = launch())) return rc;
    return order_after(t, s);
}

int td::rewrite_locked(td_tokenizer* t, RewriteBufs& w, RewriteArgs& a, const RewriteCall& c, int phases, hipStream_t s,
                       const std::function<int()>& launch) {
    int rc;
    if ((rc = rewrite_begin(t, w, a, c, s))) return rc;
    if ((rc = ensure(t, w.tiles, (size_t)((c.n_bytes + 16 + RW_TILE - 1) / RW_TILE + 1) * 8))) return rc;
    if (!c.d_flags && (rc = ensure(t, w.flags, (size_t)std::max<int64_t>(c.n_docs, 1)))) return rc;
    if (!c.d_flags) a.flags = (uint8_t*)w.flags.p;
    a.out = (uint8_t*)c.d_out;
    a.out_capacity = c.out_capacity;
    a.out_doc_off = (int64_t*)c.d_out_off;
    a.tile_base = (unsigned long long*)w.tiles.p;
    if (phases & RW_RUN_MEASURE) HIP_TRY(t, hipMemsetAsync(a.head, 0, RW_H_WORDS * 8, s));
    if ((rc = launch())) return rc;
    return order_after(t, s);
}

int td::rewrite_check_staged(td_tokenizer* t, RewriteBufs& w, int64_t n_docs, int64_t* counts, hipStream_t s, const std::function<int()>& check) {
    int rc;
    if ((rc = ensure(t, w.flags, (size_t)std::max<int64_t>(n_docs, 1)))) return rc;
    if ((rc = ensure(t, w.counts, RW_C_WORDS * 8))) return rc;
    if ((rc = check())) return rc;
    if ((rc = device_status_locked(t, s, nullptr))) return rc;
    return copy_wait(t, counts, w.counts.p, RW_C_WORDS * 8, hipMemcpyDeviceToHost, s);
}

int td::rewrite_staged(td_tokenizer* t, RewriteBufs& w, int64_t n, int64_t n_docs, int64_t* counts, bool write, const char* what, hipStream_t s,
                       const std::function<int(void* d_out, int64_t out_capacity, int phases)>& run) {
    int rc;
    if ((rc = ensure(t, w.out_off, (size_t)(n_docs + 1) * 8))) return rc;
    if ((rc = rewrite_check_staged(t, w, n_docs, counts, s, [&] { return run(nullptr, INT64_MAX, RW_RUN_MEASURE); }))) return rc;
    if (!write) return TD_OK;
    const int64_t need = counts[RW_C_BYTES];
    if (need < 0 || need > 3 * n) { t->err = std::string("the ") + what + "'s byte total is outside its bound"; return TD_E_INVALID; }
    if ((rc = ensure(t, w.out, (size_t)need + 64))) return rc;
    return run(w.out.p, need, RW_RUN_WRITE);
}

int td::encode_rewritten(td_tokenizer* t, const uint8_t* text, const void* d_text, const void* d_off, int64_t n_enc, int64_t n_docs, int mode,
                         const char* text_name, uint8_t* out_text, int64_t text_capacity, int32_t* out_ids, int64_t ids_capacity,
                         int64_t* out_tok_offsets, hipStream_t s) {
    int rc;
    const size_t docs = (size_t)n_docs;
    if (out_text) {
        if (n_enc > text_capacity) {
            t->err = std::string(text_name) + " capacity too small: " + std::to_string(n_enc) + " bytes needed";
            return TD_E_CAPACITY;
        }
        if (d_text == t->h2d_text.p) { if (n_enc) memcpy(out_text, text, (size_t)n_enc); }
        else if ((rc = copy_wait(t, out_text, d_text, (size_t)n_enc, hipMemcpyDeviceToHost, s))) return rc;
    }
    // the encode, as td_encode_batch_* do it on resident text
    const int64_t dev_cap = std::max<int64_t>(n_enc, 1);
    if ((rc = ensure(t, t->d_offsets, (docs + 1) * 8))) return rc;
    if ((rc = ensure(t, t->d_tokens, (size_t)dev_cap * 4))) return rc;
    if (n_enc > 0) {
        if ((rc = encode_device_locked(t, d_text, n_enc, d_off, n_docs, mode, t->d_tokens.p, dev_cap, t->d_offsets.p, s))) return rc;
    } else {
        HIP_TRY(t, hipMemsetAsync(t->d_offsets.p, 0, (docs + 1) * 8, s));
    }
    if ((rc = device_status_locked(t, s, nullptr))) return rc;
    if ((rc = copy_wait(t, out_tok_offsets, t->d_offsets.p, (docs + 1) * 8, hipMemcpyDeviceToHost, s))) return rc;
    const int64_t total = out_tok_offsets[n_docs];
    if (total < 0 || total > dev_cap) { t->err = "the encode's token total is outside its buffer"; return TD_E_INVALID; }
    // (not deliver_ids: these two calls have no n_tokens, name out_ids, and ask for it only where ids are to come)
    if (total > ids_capacity) {
        t->err = "output capacity too small: " + std::to_string(total) + " tokens needed";
        return TD_E_CAPACITY;
    }
    if (total > 0 && !out_ids) { t->err = "null out_ids"; return TD_E_INVALID; }
    return copy_wait(t, out_ids, t->d_tokens.p, (size_t)total * 4, hipMemcpyDeviceToHost, s);
}
