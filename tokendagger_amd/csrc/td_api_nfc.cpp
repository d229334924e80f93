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

bool overlap(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && na > 0 && nb > 0 && a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

// offsets from 0, non-decreasing (what every host entry point checks before a launch)
bool offsets_ok(const int64_t* off, int64_t n_docs) {
    if (off[0] != 0) return false;
    for (int64_t d = 0; d < n_docs; ++d)
        if (off[d + 1] < off[d]) return false;
    return true;
}

int64_t tiles_of(int64_t n_bytes) { return (n_bytes + 16 + NFC_TILE - 1) / NFC_TILE + 1; }

void fill_args(td_tokenizer* t, NfcArgs& a, const void* d_text, int64_t n_bytes, const void* d_off, int64_t n_docs) {
    memset(&a, 0, sizeof a);
    a.text = (const uint8_t*)d_text;
    a.n_bytes = n_bytes;
    a.doc_off = (const int64_t*)d_off;
    a.n_docs = n_docs;
    a.head = (unsigned long long*)t->nfc_head.p;
    Ctl* ctl = (Ctl*)t->ctl.p;
    a.err = &ctl->err;
    a.err_pos = &ctl->err_pos;
}

int check_locked(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_off, int64_t n_docs, void* d_flags, void* d_counts, hipStream_t s) {
    int rc;
    if ((rc = order_before(t, s))) return rc;
    if ((rc = ensure(t, t->nfc_head, NFC_H_WORDS * 8))) return rc;
    NfcArgs a;
    fill_args(t, a, d_text, n_bytes, d_off, n_docs);
    a.flags = (uint8_t*)d_flags;
    a.counts = (unsigned long long*)d_counts;
    HIP_TRY(t, hipMemsetAsync(a.head, 0, NFC_H_WORDS * 8, s));
    HIP_TRY(t, launch_nfc_check(a, s));
    return order_after(t, s);
}

int nfc_locked(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_off, int64_t n_docs, void* d_out, int64_t out_capacity,
               void* d_out_off, void* d_flags, void* d_changed, void* d_counts, hipStream_t s, int phases = NFC_RUN_MEASURE | NFC_RUN_WRITE) {
    int rc;
    if ((rc = order_before(t, s))) return rc;
    const size_t docs1 = (size_t)std::max<int64_t>(n_docs, 1);
    if ((rc = ensure(t, t->nfc_head, NFC_H_WORDS * 8))) return rc;
    if ((rc = ensure(t, t->nfc_tiles, (size_t)tiles_of(n_bytes) * 8))) return rc;
    if (!d_flags && (rc = ensure(t, t->nfc_flags, docs1))) return rc;
    if (!d_changed && (rc = ensure(t, t->nfc_changed, docs1))) return rc;
    NfcArgs a;
    fill_args(t, a, d_text, n_bytes, d_off, n_docs);
    a.flags = (uint8_t*)(d_flags ? d_flags : t->nfc_flags.p);
    a.changed = (uint8_t*)(d_changed ? d_changed : t->nfc_changed.p);
    a.out = (uint8_t*)d_out;
    a.out_capacity = out_capacity;
    a.out_doc_off = (int64_t*)d_out_off;
    a.counts = (unsigned long long*)d_counts;
    a.tile_base = (unsigned long long*)t->nfc_tiles.p;
    if (phases & NFC_RUN_MEASURE) HIP_TRY(t, hipMemsetAsync(a.head, 0, NFC_H_WORDS * 8, s));
    HIP_TRY(t, launch_nfc(a, s, phases));
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

// h2d_text / h2d_offs measured into nfc_flags, nfc_changed and nfc_counts, which comes back in `counts`; where `write` is set, then
// normalised into nfc_out / nfc_out_off.  nfc_out is sized from counts[0], the bytes the text needs, not from the 3 x bound.
int normalize_staged(td_tokenizer* t, int64_t n, int64_t n_docs, int64_t* counts, bool write, hipStream_t s) {
    int rc;
    const size_t docs1 = (size_t)std::max<int64_t>(n_docs, 1);
    if ((rc = ensure(t, t->nfc_out_off, (size_t)(n_docs + 1) * 8))) return rc;
    if ((rc = ensure(t, t->nfc_flags, docs1))) return rc;
    if ((rc = ensure(t, t->nfc_changed, docs1))) return rc;
    if ((rc = ensure(t, t->nfc_counts, NFC_C_WORDS * 8))) return rc;
    if ((rc = nfc_locked(t, t->h2d_text.p, n, t->h2d_offs.p, n_docs, nullptr, INT64_MAX, t->nfc_out_off.p, t->nfc_flags.p, t->nfc_changed.p,
                         t->nfc_counts.p, s, NFC_RUN_MEASURE)))
        return rc;
    if ((rc = device_status_locked(t, s, nullptr))) return rc;
    if ((rc = copy_wait(t, counts, t->nfc_counts.p, NFC_C_WORDS * 8, hipMemcpyDeviceToHost, s))) return rc;
    if (!write) return TD_OK;
    const int64_t need = counts[NFC_C_BYTES];
    if (need < 0 || need > 3 * n) { t->err = "the normaliser's byte total is outside its bound"; return TD_E_INVALID; }
    if ((rc = ensure(t, t->nfc_out, (size_t)need + 64))) return rc;
    return nfc_locked(t, t->h2d_text.p, n, t->h2d_offs.p, n_docs, t->nfc_out.p, need, t->nfc_out_off.p, t->nfc_flags.p, t->nfc_changed.p,
                      t->nfc_counts.p, s, NFC_RUN_WRITE);
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
    if (!doc_offsets || !counts || n_docs < 0 || out_capacity < 0 || (!out && out_capacity != 0) || !offsets_ok(doc_offsets, n_docs)) return TD_E_INVALID;
    const int64_t total = doc_offsets[n_docs];
    if ((total > 0 && !text) || overlap(text, total, out, out_capacity)) return TD_E_INVALID;
    const NfcTables& T = host_tables();
    int64_t c[NFC_C_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
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
            c[NFC_C_BYTES] = n;
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
    if (overlap(d_text, n_bytes, d_out, out_capacity)) return fail_unlocked(t, TD_E_INVALID, "td_nfc_device: d_out overlaps d_text");
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
        if ((rc = stage_text(t, text, doc_offsets, n_docs, s))) return rc;
        const int64_t n = doc_offsets[n_docs];
        if (overlap(text, n, out, out_capacity)) { t->err = "td_nfc: out overlaps text"; return (int)TD_E_INVALID; }
        // (the output's offsets are made by the write phase; a call that wants neither them nor the text stops behind the measure)
        if ((rc = normalize_staged(t, n, n_docs, counts, out || out_doc_offsets, s))) return rc;
        const size_t docs = (size_t)n_docs;
        if (flags && (rc = copy_wait(t, flags, t->nfc_flags.p, docs, hipMemcpyDeviceToHost, s))) return rc;
        if (changed && (rc = copy_wait(t, changed, t->nfc_changed.p, docs, hipMemcpyDeviceToHost, s))) return rc;
        if (out_doc_offsets && (rc = copy_wait(t, out_doc_offsets, t->nfc_out_off.p, (docs + 1) * 8, hipMemcpyDeviceToHost, s))) return rc;
        if (!out) return (int)TD_OK;
        if (counts[NFC_C_BYTES] > out_capacity) {
            t->err = "output capacity too small: " + std::to_string(counts[NFC_C_BYTES]) + " bytes needed";
            return (int)TD_E_CAPACITY;
        }
        return copy_wait(t, out, t->nfc_out.p, (size_t)counts[NFC_C_BYTES], hipMemcpyDeviceToHost, s);
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
        if ((rc = stage_text(t, text, doc_offsets, n_docs, s))) return rc;
        const int64_t n = doc_offsets[n_docs];
        const size_t docs = (size_t)n_docs;
        if (overlap(text, n, norm_text, norm_capacity)) { t->err = "td_encode_batch_nfc: norm_text overlaps text"; return (int)TD_E_INVALID; }
        // the proof: flags and counts[1]
        if ((rc = ensure(t, t->nfc_flags, std::max<size_t>(docs, 1)))) return rc;
        if ((rc = ensure(t, t->nfc_counts, NFC_C_WORDS * 8))) return rc;
        if ((rc = check_locked(t, t->h2d_text.p, n, t->h2d_offs.p, n_docs, t->nfc_flags.p, t->nfc_counts.p, s))) return rc;
        if ((rc = copy_wait(t, counts, t->nfc_counts.p, NFC_C_WORDS * 8, hipMemcpyDeviceToHost, s))) return rc;
        const void* d_text = t->h2d_text.p;
        const void* d_off = t->h2d_offs.p;
        int64_t n_enc = n;
        if (counts[NFC_C_UNPROVEN] == 0) {  // the text is its own NFC: it is what is encoded and what is returned
            counts[NFC_C_BYTES] = n;
            if (changed && docs) memset(changed, 0, docs);
            if (norm_doc_offsets) memcpy(norm_doc_offsets, doc_offsets, (docs + 1) * 8);
        } else {
            if ((rc = normalize_staged(t, n, n_docs, counts, true, s))) return rc;
            d_text = t->nfc_out.p;
            d_off = t->nfc_out_off.p;
            n_enc = counts[NFC_C_BYTES];
            if (changed && (rc = copy_wait(t, changed, t->nfc_changed.p, docs, hipMemcpyDeviceToHost, s))) return rc;
            if (norm_doc_offsets && (rc = copy_wait(t, norm_doc_offsets, t->nfc_out_off.p, (docs + 1) * 8, hipMemcpyDeviceToHost, s))) return rc;
        }
        if (norm_text) {
            if (n_enc > norm_capacity) {
                t->err = "norm_text capacity too small: " + std::to_string(n_enc) + " bytes needed";
                return (int)TD_E_CAPACITY;
            }
            if (d_text == t->h2d_text.p) { if (n_enc) memcpy(norm_text, text, (size_t)n_enc); }
            else if ((rc = copy_wait(t, norm_text, d_text, (size_t)n_enc, hipMemcpyDeviceToHost, s))) return rc;
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
