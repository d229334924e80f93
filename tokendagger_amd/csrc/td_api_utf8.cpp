// UTF-8 validation and repair (td_utf8.hip): the contract's host statement and the entry points.
#include "td_handle.h"
#include "td_utf8.h"

namespace {

bool policy_ok(int policy) { return policy == TD_UTF8_REPLACE || policy == TD_UTF8_IGNORE; }
static_assert(TD_UTF8_REPLACE == U8_REPLACE && TD_UTF8_IGNORE == U8_IGNORE, "the header's policies are the kernels'");

int64_t windows_of(int64_t n_bytes) { return (n_bytes + 15 + 15) / 16 + 1; }

int check_locked(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_off, int64_t n_docs, void* d_flags, void* d_first,
                 void* d_counts, hipStream_t s) {
    U8Args a;
    memset(&a, 0, sizeof a);
    a.first_bad = (unsigned long long*)d_first;
    return rewrite_check_locked(t, t->utf8, a, {d_text, n_bytes, d_off, n_docs, d_flags, d_counts, nullptr, 0, nullptr}, s, [&]() -> int {
        HIP_TRY(t, launch_utf8_check(a, s));
        return (int)TD_OK;
    });
}

int repair_locked(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_off, int64_t n_docs, int policy, void* d_out,
                  int64_t out_capacity, void* d_out_off, void* d_flags, void* d_first, void* d_nbad, void* d_counts, hipStream_t s,
                  int phases = RW_RUN_MEASURE | RW_RUN_WRITE) {
    int rc;
    if ((rc = ensure(t, t->utf8_dirty, (size_t)windows_of(n_bytes)))) return rc;
    U8Args a;
    memset(&a, 0, sizeof a);
    a.policy = policy;
    a.first_bad = (unsigned long long*)d_first;
    a.n_bad = (unsigned long long*)d_nbad;
    a.dirty = (uint8_t*)t->utf8_dirty.p;
    return rewrite_locked(t, t->utf8, a, {d_text, n_bytes, d_off, n_docs, d_flags, d_counts, d_out, out_capacity, d_out_off}, phases, s, [&]() -> int {
        if (phases & RW_RUN_MEASURE) HIP_TRY(t, hipMemsetAsync(a.dirty, 0, (size_t)windows_of(n_bytes), s));
        HIP_TRY(t, launch_utf8(a, s, phases));
        return (int)TD_OK;
    });
}

// h2d_text / h2d_offs measured into utf8.flags, utf8_first, utf8_nbad and utf8.counts, which comes back in `counts`; where `write` is
// set, then repaired into utf8.out / utf8.out_off (rewrite_staged).
int repair_staged(td_tokenizer* t, int64_t n, int64_t n_docs, int policy, int64_t* counts, bool write, hipStream_t s) {
    int rc;
    const size_t docs1 = (size_t)std::max<int64_t>(n_docs, 1);
    if ((rc = ensure(t, t->utf8_first, docs1 * 8))) return rc;
    if ((rc = ensure(t, t->utf8_nbad, docs1 * 8))) return rc;
    return rewrite_staged(t, t->utf8, n, n_docs, counts, write, "repair", s, [&](void* d_out, int64_t out_capacity, int phases) {
        return repair_locked(t, t->h2d_text.p, n, t->h2d_offs.p, n_docs, policy, d_out, out_capacity, t->utf8.out_off.p, t->utf8.flags.p,
                             t->utf8_first.p, t->utf8_nbad.p, t->utf8.counts.p, s, phases);
    });
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
    if (rewrite_overlap(d_text, n_bytes, d_out, out_capacity)) return fail_unlocked(t, TD_E_INVALID, "td_utf8_device: d_out overlaps d_text");
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
        if ((rc = stage_host_text(t, text, doc_offsets, n_docs, s))) return rc;
        const int64_t n = doc_offsets[n_docs];
        if (rewrite_overlap(text, n, out, out_capacity)) { t->err = "td_utf8: out overlaps text"; return (int)TD_E_INVALID; }
        const size_t docs1 = (size_t)std::max<int64_t>(n_docs, 1);
        if (!out && !out_doc_offsets && !n_bad) {  // flags and first_bad alone: the check, one pass at read speed, counts[1] alone
            if ((rc = ensure(t, t->utf8_first, docs1 * 8))) return rc;
            if ((rc = rewrite_check_staged(t, t->utf8, n_docs, counts, s, [&] {
                     return check_locked(t, t->h2d_text.p, n, t->h2d_offs.p, n_docs, t->utf8.flags.p, t->utf8_first.p, t->utf8.counts.p, s);
                 })))
                return rc;
            if (flags && (rc = copy_wait(t, flags, t->utf8.flags.p, (size_t)n_docs, hipMemcpyDeviceToHost, s))) return rc;
            if (first_bad && (rc = copy_wait(t, first_bad, t->utf8_first.p, (size_t)n_docs * 8, hipMemcpyDeviceToHost, s))) return rc;
            return (int)TD_OK;
        }
        // (the output's offsets are made by the write phase; a call that wants neither them nor the text stops behind the measure)
        const bool write = out || out_doc_offsets;
        if ((rc = repair_staged(t, n, n_docs, policy, counts, write, s))) return rc;
        if (out && counts[RW_C_BYTES] > out_capacity) {
            t->err = "output capacity too small: " + std::to_string(counts[RW_C_BYTES]) + " bytes needed";
            return (int)TD_E_CAPACITY;
        }
        const size_t docs = (size_t)n_docs;
        if (flags && (rc = copy_wait(t, flags, t->utf8.flags.p, docs, hipMemcpyDeviceToHost, s))) return rc;
        if (first_bad && (rc = copy_wait(t, first_bad, t->utf8_first.p, docs * 8, hipMemcpyDeviceToHost, s))) return rc;
        if (n_bad && (rc = copy_wait(t, n_bad, t->utf8_nbad.p, docs * 8, hipMemcpyDeviceToHost, s))) return rc;
        if (out_doc_offsets && (rc = copy_wait(t, out_doc_offsets, t->utf8.out_off.p, (docs + 1) * 8, hipMemcpyDeviceToHost, s))) return rc;
        if (!out) return (int)TD_OK;
        return copy_wait(t, out, t->utf8.out.p, (size_t)counts[RW_C_BYTES], hipMemcpyDeviceToHost, s);
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
        if ((rc = stage_host_text(t, text, doc_offsets, n_docs, s))) return rc;
        const int64_t n = doc_offsets[n_docs];
        const size_t docs = (size_t)n_docs;
        if (rewrite_overlap(text, n, fixed_text, fixed_capacity)) { t->err = "td_encode_batch_utf8: fixed_text overlaps text"; return (int)TD_E_INVALID; }
        // the check: flags and counts[1]
        if ((rc = rewrite_check_staged(t, t->utf8, n_docs, counts, s, [&] {
                 return check_locked(t, t->h2d_text.p, n, t->h2d_offs.p, n_docs, t->utf8.flags.p, nullptr, t->utf8.counts.p, s);
             })))
            return rc;
        const void* d_text = t->h2d_text.p;
        const void* d_off = t->h2d_offs.p;
        int64_t n_enc = n;
        if (counts[U8_C_DOCS] == 0) {  // the text is well-formed: it is what is encoded and what is returned
            counts[RW_C_BYTES] = n;
            if (flags && docs) memset(flags, 0, docs);
            for (size_t d = 0; d < docs; ++d) {
                if (first_bad) first_bad[d] = -1;
                if (n_bad) n_bad[d] = 0;
            }
            if (fixed_doc_offsets) memcpy(fixed_doc_offsets, doc_offsets, (docs + 1) * 8);
        } else {
            if ((rc = repair_staged(t, n, n_docs, policy, counts, true, s))) return rc;
            d_text = t->utf8.out.p;
            d_off = t->utf8.out_off.p;
            n_enc = counts[RW_C_BYTES];
            if (flags && (rc = copy_wait(t, flags, t->utf8.flags.p, docs, hipMemcpyDeviceToHost, s))) return rc;
            if (first_bad && (rc = copy_wait(t, first_bad, t->utf8_first.p, docs * 8, hipMemcpyDeviceToHost, s))) return rc;
            if (n_bad && (rc = copy_wait(t, n_bad, t->utf8_nbad.p, docs * 8, hipMemcpyDeviceToHost, s))) return rc;
            if (fixed_doc_offsets && (rc = copy_wait(t, fixed_doc_offsets, t->utf8.out_off.p, (docs + 1) * 8, hipMemcpyDeviceToHost, s))) return rc;
        }
        return encode_rewritten(t, text, d_text, d_off, n_enc, n_docs, mode, "fixed_text", fixed_text, fixed_capacity, out_ids, ids_capacity,
                                out_tok_offsets, s);
    });
}

}  // extern "C"
