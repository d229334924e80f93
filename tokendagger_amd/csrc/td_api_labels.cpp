// Loss labels for marked id spans (td_labels.hip): the spec's checks and the three entry points.
#include "td_handle.h"
#include "td_labels_args.h"

namespace {

// The checks of a spec (no handle, no device), and the spec as the kernels take it.
const char* labels_spec_error(const td_labels_spec* sp, LabSpec& out) {
    if (!sp) return "null td_labels_spec";
    if (sp->n_open < 1 || sp->n_open > TD_LABELS_MAX_OPEN) return "n_open must be in 1 .. 8";
    if (sp->n_close < 0 || sp->n_close > TD_LABELS_MAX_CLOSE) return "n_close must be in 0 .. 16";
    if (sp->flags & ~(int64_t)TD_LABELS_TRAIN_CLOSE) return "unknown td_labels_spec flags";
    if (sp->ignore_index < INT32_MIN || sp->ignore_index > INT32_MAX) return "ignore_index must be an int32";
    memset(&out, 0, sizeof out);
    out.n_open = (int32_t)sp->n_open;
    out.n_close = (int32_t)sp->n_close;
    out.ignore = (int32_t)sp->ignore_index;
    out.train_close = (sp->flags & TD_LABELS_TRAIN_CLOSE) ? 1 : 0;
    for (int64_t c = 0; c < sp->n_close; ++c) {
        if (sp->close_ids[c] < 0) return "a closer id is negative";
        out.close_ids[c] = sp->close_ids[c];
    }
    for (int64_t o = 0; o < sp->n_open; ++o) {
        if (sp->open_len[o] < 1 || sp->open_len[o] > TD_LABELS_MAX_OPEN_LEN) return "every open_len must be in 1 .. 8";
        out.open_len[o] = (int32_t)sp->open_len[o];
        for (int64_t k = 0; k < sp->open_len[o]; ++k) {
            const int32_t id = sp->open_ids[o][k];
            if (id < 0) return "an opener id is negative";
            for (int64_t c = 0; c < sp->n_close; ++c)
                if (sp->close_ids[c] == id) return "an opener contains a closer: no position may be both an open and a close event";
            out.open_ids[o][k] = id;
        }
    }
    return nullptr;
}

int labels_spec_fail(td_tokenizer* t, const char* fn, const char* m) {
    return m ? fail_unlocked(t, TD_E_INVALID, std::string(fn) + ": " + m) : (int)TD_OK;
}

// Enqueues the kernels on `s` into device outputs; d_mask and d_toff_out may be null.
int labels_launch_locked(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_toff, int64_t n_docs, const LabSpec& sp,
                         void* d_labels, void* d_mask, void* d_toff_out, void* d_counts, hipStream_t s) {
    int rc;
    if ((rc = order_before(t, s))) return rc;
    LabelArgs a;
    memset(&a, 0, sizeof a);
    a.ids = (const int32_t*)d_ids;
    a.n_tokens = n_tokens;
    a.tok_off = (const int64_t*)d_toff;
    a.n_docs = n_docs;
    a.spec = sp;
    a.labels = (int32_t*)d_labels;
    a.mask = (uint8_t*)d_mask;
    a.trained_off = (int64_t*)d_toff_out;
    a.counts = (long long*)d_counts;
    const size_t bits_bytes = (size_t)(n_tokens / 32 + 2) * 4, tiles = (size_t)labels_tiles_rounded(n_tokens);
    if ((rc = ensure(t, t->lab_head, LAB_HEAD_WORDS * 8))) return rc;
    if ((rc = ensure(t, t->lab_bits, bits_bytes))) return rc;
    if ((rc = ensure(t, t->lab_tiles, tiles))) return rc;
    if (d_toff_out) {
        if ((rc = ensure(t, t->lab_cnt, tiles * 8))) return rc;
        if ((rc = ensure(t, t->lab_aux, (size_t)labels_tiles(n_tokens) * LAB_THREADS * 4))) return rc;
    }
    a.head = (unsigned long long*)t->lab_head.p;
    a.bits = (uint32_t*)t->lab_bits.p;
    a.tiles = (uint8_t*)t->lab_tiles.p;
    a.tile_cnt = (unsigned long long*)t->lab_cnt.p;
    a.aux = (uint32_t*)t->lab_aux.p;
    HIP_TRY(t, hipMemsetAsync(a.head, 0, LAB_HEAD_WORDS * 8, s));
    HIP_TRY(t, hipMemsetAsync(a.bits, 0, bits_bytes, s));
    Ctl* ctl = (Ctl*)t->ctl.p;
    a.err = &ctl->err;
    a.err_pos = &ctl->err_pos;
    HIP_TRY(t, launch_labels(a, s));
    return order_after(t, s);
}

// Host entry points: `total` ids already on the device (with their offsets) on `s` -> the handle's buffers -> the caller's.
int labels_to_host(td_tokenizer* t, const void* d_ids, int64_t total, const void* d_toff, int64_t n_docs, const LabSpec& sp, int32_t* labels,
                   uint8_t* mask, int64_t* trained_offsets, int64_t* counts, hipStream_t s) {
    return labels_outputs_to_host(t, total, n_docs, labels, mask, trained_offsets, counts, s, [&](void* d_lab, void* d_mask, void* d_to, void* d_cnt) {
        return labels_launch_locked(t, d_ids, total, d_toff, n_docs, sp, d_lab, d_mask, d_to, d_cnt, s);
    });
}

}  // namespace

// The host end of a labelling call (td_span_labels*, td_range_labels*): the handle's output buffers, launch(d_labels, d_mask,
// d_trained_offsets, d_counts) on `s`, the status, then what was asked for to the caller.
int td::labels_outputs_to_host(td_tokenizer* t, int64_t total, int64_t n_docs, int32_t* labels, uint8_t* mask, int64_t* trained_offsets,
                               int64_t* counts, hipStream_t s, const std::function<int(void*, void*, void*, void*)>& launch) {
    int rc;
    const size_t n1 = (size_t)std::max<int64_t>(total, 1);
    if ((rc = ensure(t, t->lab_out, n1 * 4))) return rc;
    if (mask && (rc = ensure(t, t->lab_mask, n1))) return rc;
    if (trained_offsets && (rc = ensure(t, t->lab_toff, (size_t)(n_docs + 1) * 8))) return rc;
    if ((rc = ensure(t, t->lab_counts, 4 * sizeof(int64_t)))) return rc;
    if ((rc = launch(t->lab_out.p, mask ? t->lab_mask.p : nullptr, trained_offsets ? t->lab_toff.p : nullptr, t->lab_counts.p))) return rc;
    if ((rc = device_status_locked(t, s, nullptr))) return rc;
    if ((rc = copy_wait(t, counts, t->lab_counts.p, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, s))) return rc;
    if (trained_offsets && (rc = copy_wait(t, trained_offsets, t->lab_toff.p, (size_t)(n_docs + 1) * 8, hipMemcpyDeviceToHost, s))) return rc;
    if (total == 0) return TD_OK;
    if (mask && (rc = copy_wait(t, mask, t->lab_mask.p, (size_t)total, hipMemcpyDeviceToHost, s))) return rc;
    return copy_wait(t, labels, t->lab_out.p, (size_t)total * 4, hipMemcpyDeviceToHost, s);
}

extern "C" {

int td_span_labels_device(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_tok_offsets, int64_t n_docs,
                          const td_labels_spec* spec, void* d_labels, void* d_mask, void* d_trained_offsets, void* d_counts,
                          void* hip_stream) {
    if (!t || !spec || n_tokens < 0 || n_docs < 0 || !d_tok_offsets || (n_tokens > 0 && (!d_ids || !d_labels)) || !d_counts) return TD_E_INVALID;
    LabSpec sp;
    if (int rc = labels_spec_fail(t, "td_span_labels_device", labels_spec_error(spec, sp))) return rc;
    return locked(t, [&] {
        return labels_launch_locked(t, d_ids, n_tokens, d_tok_offsets, n_docs, sp, d_labels, d_mask, d_trained_offsets, d_counts,
                                    (hipStream_t)hip_stream);
    });
}

int td_span_labels(td_tokenizer* t, const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets, int64_t n_docs,
                   const td_labels_spec* spec, int32_t* labels, uint8_t* mask, int64_t* trained_offsets, int64_t* counts) {
    if (!t || !spec || n_tokens < 0 || n_docs < 0 || !tok_offsets || !counts) return TD_E_INVALID;
    LabSpec sp;
    if (int rc = labels_spec_fail(t, "td_span_labels", labels_spec_error(spec, sp))) return rc;
    return locked(t, [&] {
        int rc;
        if ((rc = rows_check_host_ids(t, ids, n_tokens, tok_offsets, n_docs))) return rc;
        const int64_t total = tok_offsets[n_docs];
        if (total > 0 && !labels) { t->err = "null labels output"; return (int)TD_E_INVALID; }
        hipStream_t s;
        if ((rc = rows_stage_host_ids(t, ids, tok_offsets, n_docs, s))) return rc;
        return labels_to_host(t, t->dec_tokens.p, total, t->d_offsets.p, n_docs, sp, labels, mask, trained_offsets, counts, s);
    });
}

int td_encode_batch_span_labels(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs,
                                const uint8_t* allowed_bytes, const int64_t* allowed_offsets, int64_t n_allowed,
                                const td_labels_spec* spec, int32_t* out_tokens, int64_t out_capacity, int64_t* out_offsets,
                                int32_t* out_labels, uint8_t* out_mask, int64_t* out_trained_offsets, int64_t* counts,
                                int64_t* n_tokens) {
    if (!t || !spec || !doc_offsets || n_docs < 0 || n_allowed < 0 || (n_allowed > 0 && (!allowed_bytes || !allowed_offsets)) || !out_offsets ||
        out_capacity < 0 || (out_capacity > 0 && !out_labels) || !counts)
        return TD_E_INVALID;
    LabSpec sp;
    if (int rc = labels_spec_fail(t, "td_encode_batch_span_labels", labels_spec_error(spec, sp))) return rc;
    return locked(t, [&] {
        int rc;
        if ((rc = encode_special_strs_locked(t, text, doc_offsets, n_docs, allowed_bytes, allowed_offsets, n_allowed, out_tokens, out_capacity,
                                             out_offsets, n_tokens)))
            return rc;
        const int64_t total = out_offsets[n_docs];
        hipStream_t s;
        if (t->enc_resident) {  // the encode left its ids and offsets in d_tokens / d_offsets, on its own stream
            s = t->s_own;
            return labels_to_host(t, t->d_tokens.p, total, t->d_offsets.p, n_docs, sp, out_labels, out_mask, out_trained_offsets, counts, s);
        }
        if ((rc = rows_stage_host_ids(t, out_tokens, out_offsets, n_docs, s))) return rc;
        return labels_to_host(t, t->dec_tokens.p, total, t->d_offsets.p, n_docs, sp, out_labels, out_mask, out_trained_offsets, counts, s);
    });
}

int td_encode_batch_span_label_rows(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs,
                                    const uint8_t* allowed_bytes, const int64_t* allowed_offsets, int64_t n_allowed,
                                    const td_labels_spec* lspec, const td_rows_spec* rspec, int64_t overlap, const td_rows_labels* lab,
                                    const td_label_rows_outputs* host_out, int64_t rows_capacity, int64_t* row_counts,
                                    int64_t* label_counts) {
    const char* fn = "td_encode_batch_span_label_rows";
    if (!t || !lspec || !rspec || !lab || !host_out || !doc_offsets || n_docs < 0 || n_allowed < 0 ||
        (n_allowed > 0 && (!allowed_bytes || !allowed_offsets)) || !row_counts || !label_counts)
        return TD_E_INVALID;
    LabSpec sp;
    if (int rc = labels_spec_fail(t, fn, labels_spec_error(lspec, sp))) return rc;
    if (int rc = label_rows_check(t, fn, rspec, overlap, n_docs, lab, host_out, rows_capacity)) return rc;
    return locked(t, [&] {
        int rc;
        if ((rc = check_offsets(t, "doc_offsets", doc_offsets, n_docs, text))) return rc;
        const int64_t n = doc_offsets[n_docs];
        std::vector<int64_t> toff((size_t)n_docs + 1);
        // One encode.  Where it leaves its ids in d_tokens (the device search, td_api_special.cpp) they are not copied out as well and
        // `ids` is never touched; everywhere else it writes host ids (at most one per byte), which are staged like a caller's.
        std::unique_ptr<int32_t[]> ids(new int32_t[(size_t)std::max<int64_t>(n, 1)]);
        int64_t total = 0;
        t->enc_keep_resident = true;
        rc = encode_special_strs_locked(t, text, doc_offsets, n_docs, allowed_bytes, allowed_offsets, n_allowed, ids.get(),
                                        std::max<int64_t>(n, 1), toff.data(), &total);
        t->enc_keep_resident = false;
        if (rc) return rc;
        total = toff[(size_t)n_docs];
        hipStream_t s;
        const void* d_ids;
        if (t->enc_resident) {
            s = t->s_own;
            d_ids = t->d_tokens.p;
        } else {
            if ((rc = rows_stage_host_ids(t, ids.get(), toff.data(), n_docs, s))) return rc;
            d_ids = t->dec_tokens.p;
        }
        if ((rc = ensure(t, t->lab_out, (size_t)std::max<int64_t>(total, 1) * 4))) return rc;
        if ((rc = ensure(t, t->lab_counts, 4 * sizeof(int64_t)))) return rc;
        if ((rc = labels_launch_locked(t, d_ids, total, t->d_offsets.p, n_docs, sp, t->lab_out.p, nullptr, nullptr, t->lab_counts.p, s))) return rc;
        if ((rc = device_status_locked(t, s, nullptr))) return rc;
        if ((rc = copy_wait(t, label_counts, t->lab_counts.p, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, s))) return rc;
        return label_rows_to_host(t, d_ids, t->lab_out.p, t->d_offsets.p, toff.data(), n_docs, rspec, overlap, lab, *host_out, rows_capacity,
                                  row_counts, s);
    });
}

}  // extern "C"
