// UTF-8 validation and repair (td_utf8.hip): the contract's host statement and the entry points.
#include "td_handle.h"
#include "td_utf8.h"

namespace {

bool overlap(const void* a, int64_t na, const void* b, int64_t nb) { return u8_overlap(a, na, b, nb); }

bool policy_ok(int policy) { return policy == TD_UTF8_REPLACE || policy == TD_UTF8_IGNORE; }
static_assert(TD_UTF8_REPLACE == U8_REPLACE && TD_UTF8_IGNORE == U8_IGNORE, "the header's policies are the kernels'");

int64_t tiles_of(int64_t n_bytes) { return (n_bytes + 16 + U8_TILE - 1) / U8_TILE + 1; }
int64_t windows_of(int64_t n_bytes) { return (n_bytes + 15 + 15) / 16 + 1; }

void fill_args(td_tokenizer* t, U8Args& a, const void* d_text, int64_t n_bytes, const void* d_off, int64_t n_docs) {
    memset(&a, 0, sizeof a);
    a.text = (const uint8_t*)d_text;
    a.n_bytes = n_bytes;
    a.doc_off = (const int64_t*)d_off;
    a.n_docs = n_docs;
    a.head = (unsigned long long*)t->utf8_head.p;
    Ctl* ctl = (Ctl*)t->ctl.p;
    a.err = &ctl->err;
    a.err_pos = &ctl->err_pos;
}

int check_locked(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_off, int64_t n_docs, void* d_flags, void* d_first,
                 void* d_counts, hipStream_t s) {
    int rc;
    if ((rc = order_before(t, s))) return rc;
    if ((rc = ensure(t, t->utf8_head, U8_H_WORDS * 8))) return rc;
    U8Args a;
    fill_args(t, a, d_text, n_bytes, d_off, n_docs);
    a.flags = (uint8_t*)d_flags;
    a.first_bad = (unsigned long long*)d_first;
    a.counts = (unsigned long long*)d_counts;
    HIP_TRY(t, hipMemsetAsync(a.head, 0, U8_H_WORDS * 8, s));
    HIP_TRY(t, launch_utf8_check(a, s));
    return order_after(t, s);
}

int repair_locked(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_off, int64_t n_docs, int policy, void* d_out,
                  int64_t out_capacity, void* d_out_off, void* d_flags, void* d_first, void* d_nbad, void* d_counts, hipStream_t s,
                  int phases = U8_RUN_MEASURE | U8_RUN_WRITE) {
    int rc;
    if ((rc = order_before(t, s))) return rc;
    const size_t docs1 = (size_t)std::max<int64_t>(n_docs, 1);
    if ((rc = ensure(t, t->utf8_head, U8_H_WORDS * 8))) return rc;
    if ((rc = ensure(t, t->utf8_tiles, (size_t)tiles_of(n_bytes) * 8))) return rc;
    if ((rc = ensure(t, t->utf8_dirty, (size_t)windows_of(n_bytes)))) return rc;
    if (!d_flags && (rc = ensure(t, t->utf8_flags, docs1))) return rc;
    U8Args a;
    fill_args(t, a, d_text, n_bytes, d_off, n_docs);
    a.policy = policy;
    a.flags = (uint8_t*)(d_flags ? d_flags : t->utf8_flags.p);
    a.first_bad = (unsigned long long*)d_first;
    a.n_bad = (unsigned long long*)d_nbad;
    a.out = (uint8_t*)d_out;
    a.out_capacity = out_capacity;
    a.out_doc_off = (int64_t*)d_out_off;
    a.counts = (unsigned long long*)d_counts;
    a.tile_base = (unsigned long long*)t->utf8_tiles.p;
    a.dirty = (uint8_t*)t->utf8_dirty.p;
    if (phases & U8_RUN_MEASURE) {
        HIP_TRY(t, hipMemsetAsync(a.head, 0, U8_H_WORDS * 8, s));
        HIP_TRY(t, hipMemsetAsync(a.dirty, 0, (size_t)windows_of(n_bytes), s));
    }
    HIP_TRY(t, launch_utf8(a, s, phases));
    return order_after(t, s);
}

// The host forms' start: the checks of the caller's text and offsets, and their upload into h2d_text / h2d_offs on the handle's own
// stream, which `s` becomes.
int stage_text(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, hipStream_t& s) {
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

// h2d_text / h2d_offs measured into utf8_flags, utf8_first, utf8_nbad and utf8_counts, which comes back in `counts`; where `write` is
// set, then repaired into utf8_out / utf8_out_off.  utf8_out is sized from counts[0], the bytes the text needs, not from the 3 x bound.
int repair_staged(td_tokenizer* t, int64_t n, int64_t n_docs, int policy, int64_t* counts, bool write, hipStream_t s) {
    int rc;
    const size_t docs1 = (size_t)std::max<int64_t>(n_docs, 1);
    if ((rc = ensure(t, t->utf8_out_off, (size_t)(n_docs + 1) * 8))) return rc;
    if ((rc = ensure(t, t->utf8_flags, docs1))) return rc;
    if ((rc = ensure(t, t->utf8_first, docs1 * 8))) return rc;
    if ((rc = ensure(t, t->utf8_nbad, docs1 * 8))) return rc;
    if ((rc = ensure(t, t->utf8_counts, U8_C_WORDS * 8))) return rc;
    if ((rc = repair_locked(t, t->h2d_text.p, n, t->h2d_offs.p, n_docs, policy, nullptr, INT64_MAX, t->utf8_out_off.p, t->utf8_flags.p,
                            t->utf8_first.p, t->utf8_nbad.p, t->utf8_counts.p, s, U8_RUN_MEASURE)))
        return rc;
    if ((rc = device_status_locked(t, s, nullptr))) return rc;
    if ((rc = copy_wait(t, counts, t->utf8_counts.p, U8_C_WORDS * 8, hipMemcpyDeviceToHost, s))) return rc;
    if (!write) return TD_OK;
    const int64_t need = counts[U8_C_BYTES];
    if (need < 0 || need > 3 * n) { t->err = "the repair's byte total is outside its bound"; return TD_E_INVALID; }
    if ((rc = ensure(t, t->utf8_out, (size_t)need + 64))) return rc;
    return repair_locked(t, t->h2d_text.p, n, t->h2d_offs.p, n_docs, policy, t->utf8_out.p, need, t->utf8_out_off.p, t->utf8_flags.p,
                         t->utf8_first.p, t->utf8_nbad.p, t->utf8_counts.p, s, U8_RUN_WRITE);
}

}  // namespace

extern "C" {

int td_utf8_host(const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int policy, uint8_t* out, int64_t out_capacity,
                 int64_t* out_doc_offsets, uint8_t* flags, int64_t* first_bad, int64_t* n_bad, int64_t* counts) {
    const int rc = u8_host(text, doc_offsets, n_docs, policy, out, out_capacity, out_doc_offsets, flags, first_bad, n_bad, counts);
    return rc == U8_HOST_OK ? TD_OK : rc == U8_HOST_CAPACITY ? TD_E_CAPACITY : TD_E_INVALID;
}

int td_utf8_check_device(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_doc_offsets, int64_t n_docs, void* d_flags,
                         void* d_first_bad, void* d_counts, void* hip_stream) {
    if (!t || n_bytes < 0 || n_docs < 0 || !d_doc_offsets || (n_bytes > 0 && !d_text) || (n_docs > 0 && !d_flags) || !d_counts ||
        ((((uintptr_t)d_counts) | ((uintptr_t)d_doc_offsets) | ((uintptr_t)d_first_bad)) & 7))
        return TD_E_INVALID;
    if (!hip_stream) return fail_unlocked(t, TD_E_INVALID, "td_utf8_check_device: hip_stream must not be the null stream");
    return locked(t, [&] { return check_locked(t, d_text, n_bytes, d_doc_offsets, n_docs, d_flags, d_first_bad, d_counts, (hipStream_t)hip_stream); });
}

int td_utf8_device(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_doc_offsets, int64_t n_docs, int policy, void* d_out,
                   int64_t out_capacity, void* d_out_doc_offsets, void* d_flags, void* d_first_bad, void* d_n_bad, void* d_counts,
                   void* hip_stream) {
    if (!t || n_bytes < 0 || n_docs < 0 || out_capacity < 0 || !d_doc_offsets || (n_bytes > 0 && !d_text) || (out_capacity > 0 && !d_out) ||
        !d_out_doc_offsets || !d_counts ||
        ((((uintptr_t)d_counts) | ((uintptr_t)d_doc_offsets) | ((uintptr_t)d_out_doc_offsets) | ((uintptr_t)d_first_bad) | ((uintptr_t)d_n_bad)) & 7))
        return TD_E_INVALID;
    if (!policy_ok(policy)) return fail_unlocked(t, TD_E_INVALID, "td_utf8_device: policy must be TD_UTF8_REPLACE or TD_UTF8_IGNORE");
    if (overlap(d_text, n_bytes, d_out, out_capacity)) return fail_unlocked(t, TD_E_INVALID, "td_utf8_device: d_out overlaps d_text");
    if (!hip_stream) return fail_unlocked(t, TD_E_INVALID, "td_utf8_device: hip_stream must not be the null stream");
    return locked(t, [&] {
        return repair_locked(t, d_text, n_bytes, d_doc_offsets, n_docs, policy, d_out, out_capacity, d_out_doc_offsets, d_flags, d_first_bad,
                             d_n_bad, d_counts, (hipStream_t)hip_stream);
    });
}

int td_utf8(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int policy, uint8_t* out, int64_t out_capacity,
            int64_t* out_doc_offsets, uint8_t* flags, int64_t* first_bad, int64_t* n_bad, int64_t* counts) {
    if (!t || !doc_offsets || !counts || n_docs < 0 || out_capacity < 0 || (!out && out_capacity != 0)) return TD_E_INVALID;
    if (!policy_ok(policy)) return fail_unlocked(t, TD_E_INVALID, "td_utf8: policy must be TD_UTF8_REPLACE or TD_UTF8_IGNORE");
    return locked(t, [&] {
        int rc;
        hipStream_t s;
        if ((rc = stage_text(t, text, doc_offsets, n_docs, s))) return rc;
        const int64_t n = doc_offsets[n_docs];
        if (overlap(text, n, out, out_capacity)) { t->err = "td_utf8: out overlaps text"; return (int)TD_E_INVALID; }
        const size_t docs1 = (size_t)std::max<int64_t>(n_docs, 1);
        if (!out && !out_doc_offsets && !n_bad) {  // flags and first_bad alone: the check, one pass at read speed, counts[1] alone
            if ((rc = ensure(t, t->utf8_flags, docs1))) return rc;
            if ((rc = ensure(t, t->utf8_first, docs1 * 8))) return rc;
            if ((rc = ensure(t, t->utf8_counts, U8_C_WORDS * 8))) return rc;
            if ((rc = check_locked(t, t->h2d_text.p, n, t->h2d_offs.p, n_docs, t->utf8_flags.p, t->utf8_first.p, t->utf8_counts.p, s))) return rc;
            if ((rc = device_status_locked(t, s, nullptr))) return rc;
            if ((rc = copy_wait(t, counts, t->utf8_counts.p, U8_C_WORDS * 8, hipMemcpyDeviceToHost, s))) return rc;
            if (flags && (rc = copy_wait(t, flags, t->utf8_flags.p, (size_t)n_docs, hipMemcpyDeviceToHost, s))) return rc;
            if (first_bad && (rc = copy_wait(t, first_bad, t->utf8_first.p, (size_t)n_docs * 8, hipMemcpyDeviceToHost, s))) return rc;
            return (int)TD_OK;
        }
        // (the output's offsets are made by the write phase; a call that wants neither them nor the text stops behind the measure)
        const bool write = out || out_doc_offsets;
        if ((rc = repair_staged(t, n, n_docs, policy, counts, write, s))) return rc;
        if (out && counts[U8_C_BYTES] > out_capacity) {
            t->err = "output capacity too small: " + std::to_string(counts[U8_C_BYTES]) + " bytes needed";
            return (int)TD_E_CAPACITY;
        }
        const size_t docs = (size_t)n_docs;
        if (flags && (rc = copy_wait(t, flags, t->utf8_flags.p, docs, hipMemcpyDeviceToHost, s))) return rc;
        if (first_bad && (rc = copy_wait(t, first_bad, t->utf8_first.p, docs * 8, hipMemcpyDeviceToHost, s))) return rc;
        if (n_bad && (rc = copy_wait(t, n_bad, t->utf8_nbad.p, docs * 8, hipMemcpyDeviceToHost, s))) return rc;
        if (out_doc_offsets && (rc = copy_wait(t, out_doc_offsets, t->utf8_out_off.p, (docs + 1) * 8, hipMemcpyDeviceToHost, s))) return rc;
        if (!out) return (int)TD_OK;
        return copy_wait(t, out, t->utf8_out.p, (size_t)counts[U8_C_BYTES], hipMemcpyDeviceToHost, s);
    });
}

int td_encode_batch_utf8(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode, int policy, int32_t* out_ids,
                         int64_t ids_capacity, int64_t* out_tok_offsets, uint8_t* fixed_text, int64_t fixed_capacity, int64_t* fixed_doc_offsets,
                         uint8_t* flags, int64_t* first_bad, int64_t* n_bad, int64_t* counts) {
    if (!t || !doc_offsets || !counts || !out_tok_offsets || n_docs < 0 || ids_capacity < 0 || fixed_capacity < 0 ||
        (!fixed_text && fixed_capacity != 0) || (mode != TD_MODE_ENCODE && mode != TD_MODE_ORDINARY))
        return TD_E_INVALID;
    if (!policy_ok(policy)) return fail_unlocked(t, TD_E_INVALID, "td_encode_batch_utf8: policy must be TD_UTF8_REPLACE or TD_UTF8_IGNORE");
    return locked(t, [&] {
        int rc;
        hipStream_t s;
        if ((rc = stage_text(t, text, doc_offsets, n_docs, s))) return rc;
        const int64_t n = doc_offsets[n_docs];
        const size_t docs = (size_t)n_docs;
        if (overlap(text, n, fixed_text, fixed_capacity)) { t->err = "td_encode_batch_utf8: fixed_text overlaps text"; return (int)TD_E_INVALID; }
        // the check: flags and counts[1]
        if ((rc = ensure(t, t->utf8_flags, std::max<size_t>(docs, 1)))) return rc;
        if ((rc = ensure(t, t->utf8_counts, U8_C_WORDS * 8))) return rc;
        if ((rc = check_locked(t, t->h2d_text.p, n, t->h2d_offs.p, n_docs, t->utf8_flags.p, nullptr, t->utf8_counts.p, s))) return rc;
        if ((rc = device_status_locked(t, s, nullptr))) return rc;
        if ((rc = copy_wait(t, counts, t->utf8_counts.p, U8_C_WORDS * 8, hipMemcpyDeviceToHost, s))) return rc;
        const void* d_text = t->h2d_text.p;
        const void* d_off = t->h2d_offs.p;
        int64_t n_enc = n;
        if (counts[U8_C_DOCS] == 0) {  // the text is well-formed: it is what is encoded and what is returned
            counts[U8_C_BYTES] = n;
            if (flags && docs) memset(flags, 0, docs);
            for (size_t d = 0; d < docs; ++d) {
                if (first_bad) first_bad[d] = -1;
                if (n_bad) n_bad[d] = 0;
            }
            if (fixed_doc_offsets) memcpy(fixed_doc_offsets, doc_offsets, (docs + 1) * 8);
        } else {
            if ((rc = repair_staged(t, n, n_docs, policy, counts, true, s))) return rc;
            d_text = t->utf8_out.p;
            d_off = t->utf8_out_off.p;
            n_enc = counts[U8_C_BYTES];
            if (flags && (rc = copy_wait(t, flags, t->utf8_flags.p, docs, hipMemcpyDeviceToHost, s))) return rc;
            if (first_bad && (rc = copy_wait(t, first_bad, t->utf8_first.p, docs * 8, hipMemcpyDeviceToHost, s))) return rc;
            if (n_bad && (rc = copy_wait(t, n_bad, t->utf8_nbad.p, docs * 8, hipMemcpyDeviceToHost, s))) return rc;
            if (fixed_doc_offsets && (rc = copy_wait(t, fixed_doc_offsets, t->utf8_out_off.p, (docs + 1) * 8, hipMemcpyDeviceToHost, s))) return rc;
        }
        if (fixed_text) {
            if (n_enc > fixed_capacity) {
                t->err = "fixed_text capacity too small: " + std::to_string(n_enc) + " bytes needed";
                return (int)TD_E_CAPACITY;
            }
            if (d_text == t->h2d_text.p) { if (n_enc) memcpy(fixed_text, text, (size_t)n_enc); }
            else if ((rc = copy_wait(t, fixed_text, d_text, (size_t)n_enc, hipMemcpyDeviceToHost, s))) return rc;
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
        if (total < 0 || total > dev_cap) { t->err = "the encode's token total is outside its buffer"; return (int)TD_E_INVALID; }
        if (total > ids_capacity) {
            t->err = "output capacity too small: " + std::to_string(total) + " tokens needed";
            return (int)TD_E_CAPACITY;
        }
        if (total > 0 && !out_ids) { t->err = "null out_ids"; return (int)TD_E_INVALID; }
        return copy_wait(t, out_ids, t->d_tokens.p, (size_t)total * 4, hipMemcpyDeviceToHost, s);
    });
}

}  // extern "C"
