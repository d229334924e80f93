// Loss labels from byte ranges (td_ranges.hip): the host plan, the spec's checks and the entry points.
#include "td_handle.h"
#include "td_ranges_args.h"

namespace {

struct RngSpec {
    int32_t rule, ignore;
};

const char* range_spec_error(const td_range_spec* sp, RngSpec& out) {
    if (!sp) return "null td_range_spec";
    if (sp->rule != TD_RANGE_OVERLAP && sp->rule != TD_RANGE_INSIDE && sp->rule != TD_RANGE_START)
        return "rule must be TD_RANGE_OVERLAP, TD_RANGE_INSIDE or TD_RANGE_START";
    if (sp->flags != 0) return "flags must be 0";
    if (sp->ignore_index < INT32_MIN || sp->ignore_index > INT32_MAX) return "ignore_index must be an int32";
    out.rule = (int32_t)sp->rule;
    out.ignore = (int32_t)sp->ignore_index;
    return nullptr;
}

int range_spec_fail(td_tokenizer* t, const char* fn, const char* m) {
    return m ? fail_unlocked(t, TD_E_INVALID, std::string(fn) + ": " + m) : (int)TD_OK;
}

// td_range_plan: *bad_doc = the first bad document of range_offsets, else *bad_range = the first bad range (-1, -1: an argument)
int range_plan(const int64_t* range_offsets, const int64_t* ranges, int64_t n_docs, const int64_t* doc_lens, int64_t* counts, int64_t* bad_doc,
               int64_t* bad_range) {
    *bad_doc = *bad_range = -1;
    if (counts) counts[0] = counts[1] = 0;
    if (!range_offsets || n_docs < 0) return TD_E_INVALID;
    if (range_offsets[0] != 0) { *bad_doc = 0; return TD_E_INVALID; }
    for (int64_t d = 0; d < n_docs; ++d)
        if (range_offsets[d] < 0 || range_offsets[d + 1] < range_offsets[d]) { *bad_doc = d; return TD_E_INVALID; }
    if (range_offsets[n_docs] > 0 && !ranges) return TD_E_INVALID;
    int64_t nonempty = 0, marked = 0;
    for (int64_t d = 0; d < n_docs; ++d) {
        int64_t prev_end = 0;
        for (int64_t r = range_offsets[d]; r < range_offsets[d + 1]; ++r) {
            const int64_t b = ranges[2 * r], e = ranges[2 * r + 1];
            if (b < prev_end || e < b || (doc_lens && e > doc_lens[d])) { *bad_range = r; return TD_E_INVALID; }  // (prev_end >= 0: b < 0 too)
            prev_end = e;
            nonempty += e > b;
            marked += e - b;
        }
    }
    if (counts) { counts[0] = nonempty; counts[1] = marked; }
    return TD_OK;
}

// ... and its verdict as a handle's error
int range_plan_locked(td_tokenizer* t, const int64_t* range_offsets, const int64_t* ranges, int64_t n_docs, const int64_t* doc_lens) {
    int64_t bad_doc, bad_range;
    if (range_plan(range_offsets, ranges, n_docs, doc_lens, nullptr, &bad_doc, &bad_range) == TD_OK) return TD_OK;
    t->err = bad_doc >= 0     ? "invalid range_offsets at document " + std::to_string(bad_doc)
             : bad_range >= 0 ? "range " + std::to_string(bad_range) +
                                    " is negative, reversed, not behind the range before it or ends beyond its document"
                              : "null range_offsets or ranges";
    return TD_E_INVALID;
}

// Enqueues the kernels on `s` into device outputs.  d_starts: null = the covered form; d_doc_off (covered form): the documents'
// text offsets, or null; d_mask and d_toff_out may be null.
int ranges_launch_locked(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_toff, int64_t n_docs, const void* d_starts,
                         const void* d_roff, const void* d_ranges, int64_t n_ranges, const RngSpec& sp, const void* d_doc_off, void* d_labels,
                         void* d_mask, void* d_toff_out, void* d_counts, hipStream_t s) {
    int rc;
    if ((rc = order_before(t, s))) return rc;
    RangeArgs a;
    memset(&a, 0, sizeof a);
    a.ids = (const int32_t*)d_ids;
    a.n_tokens = n_tokens;
    a.tok_off = (const int64_t*)d_toff;
    a.n_docs = n_docs;
    a.starts = (const int64_t*)d_starts;
    a.range_off = (const int64_t*)d_roff;
    a.ranges = (const long long*)d_ranges;
    a.n_ranges = n_ranges;
    a.rule = sp.rule;
    a.ignore = sp.ignore;
    a.len_off = t->dT.tok_off;
    a.max_id = t->H.max_id;
    a.doc_off = d_starts ? nullptr : (const int64_t*)d_doc_off;
    a.labels = (int32_t*)d_labels;
    a.mask = (uint8_t*)d_mask;
    a.trained_off = (int64_t*)d_toff_out;
    a.counts = (long long*)d_counts;
    const size_t bits_bytes = (size_t)(n_tokens / 32 + 2) * 4, rbits_bytes = (size_t)(n_ranges / 32 + 2) * 4;
    if ((rc = ensure(t, t->lab_head, LAB_HEAD_WORDS * 8))) return rc;
    if ((rc = ensure(t, t->lab_bits, bits_bytes))) return rc;
    if ((rc = ensure(t, t->rng_bits, rbits_bytes))) return rc;
    if ((rc = ensure(t, t->rng_cum, (size_t)std::max<int64_t>(n_ranges, 1) * 8))) return rc;
    if ((rc = ensure(t, t->rng_chunks, (size_t)(n_ranges / RNG_CHUNK + 2) * 8))) return rc;
    if (!d_starts && (rc = ensure(t, t->rng_sums, (size_t)(n_tokens / OFF_CHUNK + 2) * 12))) return rc;
    if (d_toff_out) {
        if ((rc = ensure(t, t->lab_cnt, (size_t)labels_tiles_rounded(n_tokens) * 8))) return rc;
        if ((rc = ensure(t, t->lab_aux, (size_t)labels_tiles(n_tokens) * LAB_THREADS * 4))) return rc;
    }
    a.head = (unsigned long long*)t->lab_head.p;
    a.bits = (uint32_t*)t->lab_bits.p;
    a.rbits = (uint32_t*)t->rng_bits.p;
    a.cum = (long long*)t->rng_cum.p;
    a.rchunks = (unsigned long long*)t->rng_chunks.p;
    a.chunk_sum = (unsigned long long*)t->rng_sums.p;
    a.tile_cnt = (unsigned long long*)t->lab_cnt.p;
    a.aux = (uint32_t*)t->lab_aux.p;
    HIP_TRY(t, hipMemsetAsync(a.head, 0, LAB_HEAD_WORDS * 8, s));
    HIP_TRY(t, hipMemsetAsync(a.bits, 0, bits_bytes, s));
    HIP_TRY(t, hipMemsetAsync(a.rbits, 0, rbits_bytes, s));
    Ctl* ctl = (Ctl*)t->ctl.p;
    a.err = &ctl->err;
    a.err_pos = &ctl->err_pos;
    HIP_TRY(t, launch_range_labels(a, s));
    return order_after(t, s);
}

// The caller's range_offsets and ranges (checked), and its starts and text offsets where given, into the handle's buffers on `s`.
int ranges_stage_host(td_tokenizer* t, const int64_t* range_offsets, const int64_t* ranges, int64_t n_docs, const int64_t* starts, int64_t total,
                      const int64_t* doc_offsets, hipStream_t s) {
    int rc;
    const int64_t n_ranges = range_offsets[n_docs];
    if ((rc = ensure(t, t->rng_off, (size_t)(n_docs + 1) * 8))) return rc;
    if ((rc = ensure(t, t->rng_ranges, (size_t)std::max<int64_t>(n_ranges, 1) * 16))) return rc;
    HIP_TRY(t, hipMemcpyAsync(t->rng_off.p, range_offsets, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice, s));
    if (n_ranges > 0) HIP_TRY(t, hipMemcpyAsync(t->rng_ranges.p, ranges, (size_t)n_ranges * 16, hipMemcpyHostToDevice, s));
    if (starts && total > 0) {
        if ((rc = ensure(t, t->rng_starts, (size_t)total * 8))) return rc;
        HIP_TRY(t, hipMemcpyAsync(t->rng_starts.p, starts, (size_t)total * 8, hipMemcpyHostToDevice, s));
    }
    if (doc_offsets) {
        if ((rc = ensure(t, t->rng_docs, (size_t)(n_docs + 1) * 8))) return rc;
        HIP_TRY(t, hipMemcpyAsync(t->rng_docs.p, doc_offsets, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice, s));
    }
    return TD_OK;
}

// The text forms' encode: doc_offsets and the ranges against them, then td_encode_batch_with_special_strs.  d_ids / s: where its ids
// are (left on the device, or staged like a caller's); the ranges (and for generic patterns the text offsets) are staged behind them.
int ranges_encode_locked(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, const uint8_t* allowed_bytes,
                         const int64_t* allowed_offsets, int64_t n_allowed, const int64_t* range_offsets, const int64_t* ranges, int32_t* out_tokens,
                         int64_t out_capacity, int64_t* out_offsets, int64_t* n_tokens, const void*& d_ids, const void*& d_doc_off, hipStream_t& s) {
    int rc;
    if ((rc = check_offsets(t, "doc_offsets", doc_offsets, n_docs, text))) return rc;
    std::vector<int64_t> lens((size_t)n_docs);
    for (int64_t d = 0; d < n_docs; ++d) lens[(size_t)d] = doc_offsets[d + 1] - doc_offsets[d];
    if ((rc = range_plan_locked(t, range_offsets, ranges, n_docs, lens.data()))) return rc;
    if ((rc = encode_special_strs_locked(t, text, doc_offsets, n_docs, allowed_bytes, allowed_offsets, n_allowed, out_tokens, out_capacity,
                                         out_offsets, n_tokens)))
        return rc;
    if (t->enc_resident) {  // the encode left its ids and offsets in d_tokens / d_offsets, on its own stream
        s = t->s_own;
        d_ids = t->d_tokens.p;
    } else {
        if ((rc = rows_stage_host_ids(t, out_tokens, out_offsets, n_docs, s))) return rc;
        d_ids = t->dec_tokens.p;
    }
    const bool generic = t->H.pattern_kind == PATTERN_GENERIC;  // (every other pattern covers every byte)
    if ((rc = ranges_stage_host(t, range_offsets, ranges, n_docs, nullptr, 0, generic ? doc_offsets : nullptr, s))) return rc;
    d_doc_off = generic ? t->rng_docs.p : nullptr;
    return TD_OK;
}

// What the device can still find in a text form: the ranges were checked against the documents' lengths on the host.
int ranges_text_error(td_tokenizer* t, int rc) {
    if (rc == TD_E_INVALID)
        t->err = "a document's ids cover fewer bytes than it has (the split pattern skipped text): use td_encode_batch_with_starts and "
                 "td_range_labels with explicit starts";
    return rc;
}

}  // namespace

extern "C" {

int td_range_plan(const int64_t* range_offsets, const int64_t* ranges, int64_t n_docs, const int64_t* doc_lens, int64_t* counts,
                  int64_t* bad) {
    int64_t bad_doc, bad_range;
    const int rc = range_plan(range_offsets, ranges, n_docs, doc_lens, counts, &bad_doc, &bad_range);
    if (bad) *bad = bad_doc >= 0 ? bad_doc : bad_range;
    return rc;
}

int td_range_labels_device(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_tok_offsets, int64_t n_docs,
                           const void* d_starts, const void* d_range_offsets, const void* d_ranges, int64_t n_ranges,
                           const td_range_spec* spec, void* d_labels, void* d_mask, void* d_trained_offsets, void* d_counts,
                           void* hip_stream) {
    if (!t || !spec || n_tokens < 0 || n_docs < 0 || n_ranges < 0 || !d_tok_offsets || !d_range_offsets || (n_ranges > 0 && !d_ranges) ||
        (n_tokens > 0 && (!d_ids || !d_labels)) || !d_counts || (((uintptr_t)d_ranges) & 7))
        return TD_E_INVALID;
    RngSpec sp;
    if (int rc = range_spec_fail(t, "td_range_labels_device", range_spec_error(spec, sp))) return rc;
    return locked(t, [&] {
        return ranges_launch_locked(t, d_ids, n_tokens, d_tok_offsets, n_docs, d_starts, d_range_offsets, d_ranges, n_ranges, sp, nullptr, d_labels,
                                    d_mask, d_trained_offsets, d_counts, (hipStream_t)hip_stream);
    });
}

int td_range_labels(td_tokenizer* t, const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets, int64_t n_docs,
                    const int64_t* starts, const int64_t* range_offsets, const int64_t* ranges, const td_range_spec* spec,
                    int32_t* labels, uint8_t* mask, int64_t* trained_offsets, int64_t* counts) {
    if (!t || !spec || n_tokens < 0 || n_docs < 0 || !tok_offsets || !range_offsets || !counts) return TD_E_INVALID;
    RngSpec sp;
    if (int rc = range_spec_fail(t, "td_range_labels", range_spec_error(spec, sp))) return rc;
    return locked(t, [&] {
        int rc;
        if ((rc = rows_check_host_ids(t, ids, n_tokens, tok_offsets, n_docs))) return rc;
        if ((rc = range_plan_locked(t, range_offsets, ranges, n_docs, nullptr))) return rc;
        const int64_t total = tok_offsets[n_docs];
        if (total > 0 && !labels) { t->err = "null labels output"; return (int)TD_E_INVALID; }
        hipStream_t s;
        if ((rc = rows_stage_host_ids(t, ids, tok_offsets, n_docs, s))) return rc;
        if ((rc = ranges_stage_host(t, range_offsets, ranges, n_docs, starts, total, nullptr, s))) return rc;
        rc = labels_outputs_to_host(t, total, n_docs, labels, mask, trained_offsets, counts, s, [&](void* d_lab, void* d_mask, void* d_to, void* d_cnt) {
            return ranges_launch_locked(t, t->dec_tokens.p, total, t->d_offsets.p, n_docs, starts && total > 0 ? t->rng_starts.p : nullptr,
                                        t->rng_off.p, t->rng_ranges.p, range_offsets[n_docs], sp, nullptr, d_lab, d_mask, d_to, d_cnt, s);
        });
        if (rc == TD_E_INVALID) t->err += " (a range index: it ends beyond the bytes its document's ids cover)";
        return rc;
    });
}

int td_encode_batch_range_labels(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs,
                                 const uint8_t* allowed_bytes, const int64_t* allowed_offsets, int64_t n_allowed,
                                 const int64_t* range_offsets, const int64_t* ranges, const td_range_spec* spec, int32_t* out_tokens,
                                 int64_t out_capacity, int64_t* out_offsets, int32_t* out_labels, uint8_t* out_mask,
                                 int64_t* out_trained_offsets, int64_t* counts, int64_t* n_tokens) {
    if (!t || !spec || !doc_offsets || n_docs < 0 || n_allowed < 0 || (n_allowed > 0 && (!allowed_bytes || !allowed_offsets)) || !out_offsets ||
        out_capacity < 0 || (out_capacity > 0 && !out_labels) || !counts || !range_offsets)
        return TD_E_INVALID;
    RngSpec sp;
    if (int rc = range_spec_fail(t, "td_encode_batch_range_labels", range_spec_error(spec, sp))) return rc;
    return locked(t, [&] {
        int rc;
        const void *d_ids, *d_doc_off;
        hipStream_t s;
        if ((rc = ranges_encode_locked(t, text, doc_offsets, n_docs, allowed_bytes, allowed_offsets, n_allowed, range_offsets, ranges, out_tokens,
                                       out_capacity, out_offsets, n_tokens, d_ids, d_doc_off, s)))
            return rc;
        const int64_t total = out_offsets[n_docs];
        return ranges_text_error(t, labels_outputs_to_host(t, total, n_docs, out_labels, out_mask, out_trained_offsets, counts, s,
                                                           [&](void* d_lab, void* d_mask, void* d_to, void* d_cnt) {
            return ranges_launch_locked(t, d_ids, total, t->d_offsets.p, n_docs, nullptr, t->rng_off.p, t->rng_ranges.p, range_offsets[n_docs], sp,
                                        d_doc_off, d_lab, d_mask, d_to, d_cnt, s);
        }));
    });
}

int td_encode_batch_range_label_rows(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs,
                                     const uint8_t* allowed_bytes, const int64_t* allowed_offsets, int64_t n_allowed,
                                     const int64_t* range_offsets, const int64_t* ranges, const td_range_spec* rgspec,
                                     const td_rows_spec* rspec, int64_t overlap, const td_rows_labels* lab,
                                     const td_label_rows_outputs* host_out, int64_t rows_capacity, int64_t* row_counts,
                                     int64_t* label_counts) {
    const char* fn = "td_encode_batch_range_label_rows";
    if (!t || !rgspec || !rspec || !lab || !host_out || !doc_offsets || n_docs < 0 || n_allowed < 0 ||
        (n_allowed > 0 && (!allowed_bytes || !allowed_offsets)) || !row_counts || !label_counts || !range_offsets)
        return TD_E_INVALID;
    RngSpec sp;
    if (int rc = range_spec_fail(t, fn, range_spec_error(rgspec, sp))) return rc;
    if (int rc = label_rows_check(t, fn, rspec, overlap, n_docs, lab, host_out, rows_capacity)) return rc;
    return locked(t, [&] {
        int rc;
        if ((rc = check_offsets(t, "doc_offsets", doc_offsets, n_docs, text))) return rc;
        const int64_t n = doc_offsets[n_docs];
        std::vector<int64_t> toff((size_t)n_docs + 1);
        // (one encode; ids that stay in d_tokens are not copied out as well: td_encode_batch_span_label_rows)
        std::unique_ptr<int32_t[]> ids(new int32_t[(size_t)std::max<int64_t>(n, 1)]);
        int64_t total = 0;
        const void *d_ids, *d_doc_off;
        hipStream_t s;
        t->enc_keep_resident = true;
        rc = ranges_encode_locked(t, text, doc_offsets, n_docs, allowed_bytes, allowed_offsets, n_allowed, range_offsets, ranges, ids.get(),
                                  std::max<int64_t>(n, 1), toff.data(), &total, d_ids, d_doc_off, s);
        t->enc_keep_resident = false;
        if (rc) return rc;
        total = toff[(size_t)n_docs];
        if ((rc = ensure(t, t->lab_out, (size_t)std::max<int64_t>(total, 1) * 4))) return rc;
        if ((rc = ensure(t, t->lab_counts, 4 * sizeof(int64_t)))) return rc;
        if ((rc = ranges_launch_locked(t, d_ids, total, t->d_offsets.p, n_docs, nullptr, t->rng_off.p, t->rng_ranges.p, range_offsets[n_docs], sp,
                                       d_doc_off, t->lab_out.p, nullptr, nullptr, t->lab_counts.p, s)))
            return rc;
        if ((rc = ranges_text_error(t, device_status_locked(t, s, nullptr)))) return rc;
        if ((rc = copy_wait(t, label_counts, t->lab_counts.p, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, s))) return rc;
        return label_rows_to_host(t, d_ids, t->lab_out.p, t->d_offsets.p, toff.data(), n_docs, rspec, overlap, lab, *host_out, rows_capacity,
                                  row_counts, s);
    });
}

}  // extern "C"
