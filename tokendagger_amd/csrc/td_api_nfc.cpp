// Unicode NFC normalisation (td_nfc.hip): the tables on the host, the contract's host statement and the entry points.
#include "td_handle.h"
#include "td_nfc.h"

namespace {

#define TD_NFC_TABLE(type, name, n) const type name[n]
#include "generated/unicode_nfc.inc"
#undef TD_NFC_TABLE

const NfcTables& host_tables() {
    static const NfcTables T{td_nfc_stage1, td_nfc_stage2, td_nfc_dec_key, td_nfc_dec_off, td_nfc_dec_cps, td_nfc_pair_a, td_nfc_pair_b, td_nfc_pair_c};
    return T;
}

int check_locked(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_off, int64_t n_docs, void* d_flags, void* d_counts, hipStream_t s) {
    NfcArgs a;
    memset(&a, 0, sizeof a);
    return rewrite_check_locked(t, t->nfc, a, {d_text, n_bytes, d_off, n_docs, d_flags, d_counts, nullptr, 0, nullptr}, s, [&]() -> int {
        HIP_TRY(t, launch_nfc_check(a, s));
        return (int)TD_OK;
    });
}

int nfc_locked(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_off, int64_t n_docs, void* d_out, int64_t out_capacity,
               void* d_out_off, void* d_flags, void* d_changed, void* d_counts, hipStream_t s, int phases = RW_RUN_MEASURE | RW_RUN_WRITE) {
    int rc;
    if (!d_changed && (rc = ensure(t, t->nfc_changed, (size_t)std::max<int64_t>(n_docs, 1)))) return rc;
    NfcArgs a;
    memset(&a, 0, sizeof a);
    a.changed = (uint8_t*)(d_changed ? d_changed : t->nfc_changed.p);
    return rewrite_locked(t, t->nfc, a, {d_text, n_bytes, d_off, n_docs, d_flags, d_counts, d_out, out_capacity, d_out_off}, phases, s, [&]() -> int {
        HIP_TRY(t, launch_nfc(a, s, phases));
        return (int)TD_OK;
    });
}

// h2d_text / h2d_offs measured into nfc.flags, nfc_changed and nfc.counts, which comes back in `counts`; where `write` is set, then
// normalised into nfc.out / nfc.out_off (rewrite_staged).
int normalize_staged(td_tokenizer* t, int64_t n, int64_t n_docs, int64_t* counts, bool write, hipStream_t s) {
    int rc;
    if ((rc = ensure(t, t->nfc_changed, (size_t)std::max<int64_t>(n_docs, 1)))) return rc;
    return rewrite_staged(t, t->nfc, n, n_docs, counts, write, "normaliser", s, [&](void* d_out, int64_t out_capacity, int phases) {
        return nfc_locked(t, t->h2d_text.p, n, t->h2d_offs.p, n_docs, d_out, out_capacity, t->nfc.out_off.p, t->nfc.flags.p, t->nfc_changed.p,
                          t->nfc.counts.p, s, phases);
    });
}

}  // namespace

extern "C" {

int64_t td_nfc_info(int what) {
    switch (what) {
        case TD_NFC_INFO_UNICODE_VERSION: return TD_NFC_UNICODE_VERSION;
        case TD_NFC_INFO_TABLE_BYTES: return TD_NFC_TABLE_BYTES;
        default: return -1;
    }
}

int td_nfc_host(const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, uint8_t* out, int64_t out_capacity, int64_t* out_doc_offsets,
                uint8_t* flags, uint8_t* changed, int64_t* counts) {
    if (!doc_offsets || !counts || n_docs < 0 || out_capacity < 0 || (!out && out_capacity != 0) || !rewrite_offsets_ok(doc_offsets, n_docs)) return TD_E_INVALID;
    const int64_t total = doc_offsets[n_docs];
    if ((total > 0 && !text) || rewrite_overlap(text, total, out, out_capacity)) return TD_E_INVALID;
    const NfcTables& T = host_tables();
    int64_t c[RW_C_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int pass = 0; pass < 2; ++pass) {  // measure (flags, changed, counts, offsets), then write
        int64_t n = 0;
        for (int64_t d = 0; d < n_docs; ++d) {
            const int64_t ds = doc_offsets[d], de = doc_offsets[d + 1];
            bool unproven = false, differs = false;
            if (!pass && out_doc_offsets) out_doc_offsets[d] = n;
            for (int64_t p = ds; p < de;) {
                const NfcSeg g = nfc_seg_scan(T, text, p, de);
                if (g.proven) {
                    if (pass) memcpy(out + n, text + p, (size_t)(g.end - p));
                    n += g.end - p;
                } else {
                    bool dif;
                    n += nfc_rewrite(T, text, p, g, pass ? out + n : nullptr, dif);
                    unproven = true;
                    differs |= dif;
                    c[NFC_C_SEGMENTS] += 1;
                    c[NFC_C_CPS] += g.cps;
                }
                c[NFC_C_OPAQUE] += g.opaque;
                c[NFC_C_LONGEST] = std::max<int64_t>(c[NFC_C_LONGEST], g.cps);
                p = g.end;
            }
            if (!pass) {
                if (flags) flags[d] = unproven;
                if (changed) changed[d] = differs;
                c[NFC_C_UNPROVEN] += unproven;
                c[NFC_C_CHANGED] += differs;
            }
        }
        if (!pass) {
            if (out_doc_offsets) out_doc_offsets[n_docs] = n;
            c[RW_C_BYTES] = n;
            memcpy(counts, c, sizeof c);
            if (!out) return TD_OK;
            if (n > out_capacity) return TD_E_CAPACITY;
        }
    }
    return TD_OK;
}

int td_nfc_check_device(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_doc_offsets, int64_t n_docs, void* d_flags,
                        void* d_counts, void* hip_stream) {
    if (!t || n_bytes < 0 || n_docs < 0 || !d_doc_offsets || (n_bytes > 0 && !d_text) || (n_docs > 0 && !d_flags) || !d_counts ||
        ((((uintptr_t)d_counts) | ((uintptr_t)d_doc_offsets)) & 7))
        return TD_E_INVALID;
    if (!hip_stream) return fail_unlocked(t, TD_E_INVALID, "td_nfc_check_device: hip_stream must not be the null stream");
    return locked(t, [&] { return check_locked(t, d_text, n_bytes, d_doc_offsets, n_docs, d_flags, d_counts, (hipStream_t)hip_stream); });
}

int td_nfc_device(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_doc_offsets, int64_t n_docs, void* d_out,
                  int64_t out_capacity, void* d_out_doc_offsets, void* d_changed, void* d_counts, void* hip_stream) {
    if (!t || n_bytes < 0 || n_docs < 0 || out_capacity < 0 || !d_doc_offsets || (n_bytes > 0 && !d_text) || (out_capacity > 0 && !d_out) ||
        !d_out_doc_offsets || !d_counts || ((((uintptr_t)d_counts) | ((uintptr_t)d_doc_offsets) | ((uintptr_t)d_out_doc_offsets)) & 7))
        return TD_E_INVALID;
    if (rewrite_overlap(d_text, n_bytes, d_out, out_capacity)) return fail_unlocked(t, TD_E_INVALID, "td_nfc_device: d_out overlaps d_text");
    if (!hip_stream) return fail_unlocked(t, TD_E_INVALID, "td_nfc_device: hip_stream must not be the null stream");
    return locked(t, [&] {
        return nfc_locked(t, d_text, n_bytes, d_doc_offsets, n_docs, d_out, out_capacity, d_out_doc_offsets, nullptr, d_changed, d_counts,
                          (hipStream_t)hip_stream);
    });
}

int td_nfc(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, uint8_t* out, int64_t out_capacity,
           int64_t* out_doc_offsets, uint8_t* flags, uint8_t* changed, int64_t* counts) {
    if (!t || !doc_offsets || !counts || n_docs < 0 || out_capacity < 0 || (!out && out_capacity != 0)) return TD_E_INVALID;
    return locked(t, [&] {
        int rc;
        hipStream_t s;
        if ((rc = stage_host_text(t, text, doc_offsets, n_docs, s))) return rc;
        const int64_t n = doc_offsets[n_docs];
        if (rewrite_overlap(text, n, out, out_capacity)) { t->err = "td_nfc: out overlaps text"; return (int)TD_E_INVALID; }
        // (the output's offsets are made by the write phase; a call that wants neither them nor the text stops behind the measure)
        if ((rc = normalize_staged(t, n, n_docs, counts, out || out_doc_offsets, s))) return rc;
        const size_t docs = (size_t)n_docs;
        if (flags && (rc = copy_wait(t, flags, t->nfc.flags.p, docs, hipMemcpyDeviceToHost, s))) return rc;
        if (changed && (rc = copy_wait(t, changed, t->nfc_changed.p, docs, hipMemcpyDeviceToHost, s))) return rc;
        if (out_doc_offsets && (rc = copy_wait(t, out_doc_offsets, t->nfc.out_off.p, (docs + 1) * 8, hipMemcpyDeviceToHost, s))) return rc;
        if (!out) return (int)TD_OK;
        if (counts[RW_C_BYTES] > out_capacity) {
            t->err = "output capacity too small: " + std::to_string(counts[RW_C_BYTES]) + " bytes needed";
            return (int)TD_E_CAPACITY;
        }
        return copy_wait(t, out, t->nfc.out.p, (size_t)counts[RW_C_BYTES], hipMemcpyDeviceToHost, s);
    });
}

int td_encode_batch_nfc(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode, int32_t* out_ids,
                        int64_t ids_capacity, int64_t* out_tok_offsets, uint8_t* norm_text, int64_t norm_capacity, int64_t* norm_doc_offsets,
                        uint8_t* changed, int64_t* counts) {
    if (!t || !doc_offsets || !counts || !out_tok_offsets || n_docs < 0 || ids_capacity < 0 || norm_capacity < 0 || (!norm_text && norm_capacity != 0) ||
        (mode != TD_MODE_ENCODE && mode != TD_MODE_ORDINARY))
        return TD_E_INVALID;
    return locked(t, [&] {
        int rc;
        hipStream_t s;
        if ((rc = stage_host_text(t, text, doc_offsets, n_docs, s))) return rc;
        const int64_t n = doc_offsets[n_docs];
        const size_t docs = (size_t)n_docs;
        if (rewrite_overlap(text, n, norm_text, norm_capacity)) { t->err = "td_encode_batch_nfc: norm_text overlaps text"; return (int)TD_E_INVALID; }
        // the proof: flags and counts[1]
        if ((rc = rewrite_check_staged(t, t->nfc, n_docs, counts, s, [&] {
                 return check_locked(t, t->h2d_text.p, n, t->h2d_offs.p, n_docs, t->nfc.flags.p, t->nfc.counts.p, s);
             })))
            return rc;
        const void* d_text = t->h2d_text.p;
        const void* d_off = t->h2d_offs.p;
        int64_t n_enc = n;
        if (counts[NFC_C_UNPROVEN] == 0) {  // the text is its own NFC: it is what is encoded and what is returned
            counts[RW_C_BYTES] = n;
            if (changed && docs) memset(changed, 0, docs);
            if (norm_doc_offsets) memcpy(norm_doc_offsets, doc_offsets, (docs + 1) * 8);
        } else {
            if ((rc = normalize_staged(t, n, n_docs, counts, true, s))) return rc;
            d_text = t->nfc.out.p;
            d_off = t->nfc.out_off.p;
            n_enc = counts[RW_C_BYTES];
            if (changed && (rc = copy_wait(t, changed, t->nfc_changed.p, docs, hipMemcpyDeviceToHost, s))) return rc;
            if (norm_doc_offsets && (rc = copy_wait(t, norm_doc_offsets, t->nfc.out_off.p, (docs + 1) * 8, hipMemcpyDeviceToHost, s))) return rc;
        }
        return encode_rewritten(t, text, d_text, d_off, n_enc, n_docs, mode, "norm_text", norm_text, norm_capacity, out_ids, ids_capacity,
                                out_tok_offsets, s);
    });
}

}  // extern "C"
