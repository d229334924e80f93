// Bag models (td_bag.hip): the model (the checked dictionary's table, the padded matrices and the tree, built on the host), the
// contract's host statement and the entry points.
#include "td_bag.h"
#include "td_handle.h"

struct td_bag_model {
    int device = 0;
    BagModel m{};  // its pointers: the device's copies
    std::vector<void*> allocs;
    int64_t device_bytes = 0;
    int depth = 0;
    ~td_bag_model() {
        DeviceGuard dg(device);
        for (void* p : allocs) (void)hipFree(p);
    }
};

namespace {

int classify_locked(td_tokenizer* t, const td_bag_model* model, const void* d_text, int64_t n_bytes, const void* d_off, int64_t n_docs, int flags,
                    void* d_best, void* d_bprob, void* d_probs, void* d_hidden, void* d_stats, void* d_totals, hipStream_t s) {
    BagArgs a;
    memset(&a, 0, sizeof a);
    a.m = model->m;
    a.call_flags = flags;
    a.best = (int32_t*)d_best;
    a.best_prob = (float*)d_bprob;
    a.probs = (float*)d_probs;
    a.hidden = (float*)d_hidden;
    a.stats = (unsigned long long*)d_stats;
    a.totals = (unsigned long long*)d_totals;
    return rewrite_check_locked(t, t->bag, a, {d_text, n_bytes, d_off, n_docs, nullptr, nullptr, nullptr, 0, nullptr}, s, [&]() -> int {
        int rc;
        const size_t row = (size_t)a.m.dimp * 4;
        a.max_recs = bag_max_recs(n_bytes, n_docs);
        if ((rc = ensure(t, t->bag.tiles, (size_t)bag_max_tiles(n_bytes) * 8))) return rc;
        if ((rc = ensure(t, t->bag_rec, (size_t)a.max_recs * sizeof(BagRec)))) return rc;
        if ((rc = ensure(t, t->bag_first, (size_t)(n_docs + 1) * 8))) return rc;
        if ((rc = ensure(t, t->bag_hsum, std::max<size_t>((size_t)n_docs, 1) * row))) return rc;
        if ((rc = ensure(t, t->bag_part, (size_t)bag_max_chunks(n_bytes, n_docs) * 2 * row))) return rc;
        if ((rc = ensure(t, t->bag_head, BAG_H_WORDS * 8))) return rc;
        a.tile_base = (unsigned long long*)t->bag.tiles.p;
        a.rec = (BagRec*)t->bag_rec.p;
        a.first = (long long*)t->bag_first.p;
        a.hsum = (float*)t->bag_hsum.p;
        a.part = (float*)t->bag_part.p;
        a.bhead = (unsigned long long*)t->bag_head.p;
        HIP_TRY(t, launch_bag(a, s));
        return (int)TD_OK;
    });
}

// n bytes of host memory to a new device allocation the model owns
int upload(td_tokenizer* t, td_bag_model* m, const void* src, size_t bytes, const void** out) {
    void* p = nullptr;
    HIP_TRY(t, hipMalloc(&p, std::max<size_t>(bytes, 16)));
    m->allocs.push_back(p);
    m->device_bytes += (int64_t)bytes;
    *out = p;
    return bytes ? copy_wait(t, p, src, bytes, hipMemcpyHostToDevice, t->s_own) : (int)TD_OK;
}

}  // namespace

extern "C" {

int td_bag_model_create(td_tokenizer* t, const uint8_t* word_bytes, const int64_t* word_offsets, int64_t n_words, const float* input,
                        const float* output, const int64_t* label_counts, const td_bag_params* params, td_bag_model** out, int64_t* err_pos) {
    if (err_pos) *err_pos = -1;
    if (!t || !out) return TD_E_INVALID;
    *out = nullptr;
    const BagWords words = {word_bytes, word_offsets, n_words};
    int64_t pos = -1;
    std::vector<uint32_t> order;
    if (bag_check(words, params, input, output, label_counts, &pos, &order)) {
        if (err_pos) *err_pos = pos;
        return fail_unlocked(t, TD_E_INVALID, pos < 0 ? std::string("td_bag_model_create: a parameter outside its limits, a null pointer, offsets that do not start at 0 or label counts that increase")
                                                      : "td_bag_model_create: word " + std::to_string(pos) + " is empty, holds a delimiter or is a duplicate");
    }
    const td_bag_params& p = *params;
    std::unique_ptr<td_bag_model> model(new td_bag_model);
    model->device = t->device;
    BagModel& M = model->m;
    M.nwords = n_words;
    M.bucket = p.bucket;
    M.dim = p.dim;
    M.dimp = (p.dim + 3) & ~3;
    M.n_labels = p.n_labels;
    M.n_out = p.loss == BAG_HS ? p.n_labels - 1 : p.n_labels;
    M.lpad = (M.n_out + 63) & ~63;
    M.minn = p.minn;
    M.maxn = p.maxn;
    M.word_ngrams = p.word_ngrams;
    M.loss = p.loss;
    const uint8_t eos[4] = {'<', '/', 's', '>'};
    M.eos_idx = (int32_t)bag_find(words, order, eos, 4);
    std::vector<uint32_t>().swap(order);
    std::vector<uint32_t> blob, hs_off, hs_path;
    M.dict = bag_build_dict(words, blob);
    if (p.loss == BAG_HS) model->depth = bag_build_tree(label_counts, p.n_labels, hs_off, hs_path);
    const int64_t rows = n_words + p.bucket;
    std::vector<float> win, wo_t((size_t)M.dim * M.lpad, 0.0f);
    if (M.dimp != M.dim) {  // (a row padded to 16 bytes)
        win.assign((size_t)rows * M.dimp, 0.0f);
        for (int64_t r = 0; r < rows; ++r) memcpy(win.data() + r * M.dimp, input + r * M.dim, sizeof(float) * (size_t)M.dim);
    }
    for (int l = 0; l < M.n_out; ++l)
        for (int k = 0; k < M.dim; ++k) wo_t[(size_t)k * M.lpad + l] = output[(int64_t)l * M.dim + k];
    const int rc = locked(t, [&] {
        int rc;
        if ((rc = own_streams(t))) return rc;
        if ((rc = upload(t, model.get(), blob.data(), blob.size() * 4, (const void**)&M.dict.blob))) return rc;
        if ((rc = upload(t, model.get(), win.empty() ? input : win.data(), (size_t)rows * M.dimp * 4, (const void**)&M.win))) return rc;
        if ((rc = upload(t, model.get(), wo_t.data(), wo_t.size() * 4, (const void**)&M.wo_t))) return rc;
        if ((rc = upload(t, model.get(), hs_off.data(), hs_off.size() * 4, (const void**)&M.hs_off))) return rc;
        return upload(t, model.get(), hs_path.data(), hs_path.size() * 4, (const void**)&M.hs_path);
    });
    if (rc) return rc;
    *out = model.release();
    return TD_OK;
}

void td_bag_model_destroy(td_bag_model* model) { delete model; }

int64_t td_bag_model_info(const td_bag_model* model, int what) {
    if (!model) return -1;
    switch (what) {
        case TD_BAG_INFO_WORDS: return model->m.nwords;
        case TD_BAG_INFO_DIM: return model->m.dim;
        case TD_BAG_INFO_LABELS: return model->m.n_labels;
        case TD_BAG_INFO_DEVICE_BYTES: return model->device_bytes;
        case TD_BAG_INFO_EOS_INDEX: return model->m.eos_idx;
        case TD_BAG_INFO_TREE_DEPTH: return model->depth;
    }
    return -1;
}

int td_bag_classify_host(const uint8_t* word_bytes, const int64_t* word_offsets, int64_t n_words, const float* input, const float* output,
                         const int64_t* label_counts, const td_bag_params* params, const uint8_t* text, const int64_t* doc_offsets,
                         int64_t n_docs, int flags, int32_t* best, float* best_prob, float* probs, float* hidden, int64_t* stats,
                         int64_t* totals, int64_t* err_pos) {
    int64_t pos = -1;
    const int rc = bag_host({word_bytes, word_offsets, n_words}, input, output, label_counts, params, text, doc_offsets, n_docs, flags, best,
                            best_prob, probs, hidden, stats, totals, &pos);
    if (err_pos) *err_pos = pos;
    return rc ? TD_E_INVALID : TD_OK;
}

int td_bag_classify_device(td_tokenizer* t, const td_bag_model* model, const void* d_text, int64_t n_bytes, const void* d_doc_offsets,
                           int64_t n_docs, int flags, void* d_best, void* d_best_prob, void* d_probs, void* d_hidden, void* d_stats,
                           void* d_totals, void* hip_stream) {
    if (!t || !model || n_bytes < 0 || n_docs < 0 || !d_doc_offsets || (n_bytes > 0 && !d_text) ||
        (n_docs > 0 && (!d_stats || !d_best || !d_best_prob)) || ((((uintptr_t)d_stats) | ((uintptr_t)d_doc_offsets) | ((uintptr_t)d_totals)) & 7) ||
        ((((uintptr_t)d_best) | ((uintptr_t)d_best_prob) | ((uintptr_t)d_probs) | ((uintptr_t)d_hidden)) & 3))
        return TD_E_INVALID;
    if (!bag_call_flags_ok(flags)) return fail_unlocked(t, TD_E_INVALID, "td_bag_classify_device: flags must be 0 or TD_BAG_EOS");
    if (model->device != t->device) return fail_unlocked(t, TD_E_INVALID, "td_bag_classify_device: the model lives on another device");
    if (!hip_stream) return fail_unlocked(t, TD_E_INVALID, "td_bag_classify_device: hip_stream must not be the null stream");
    return locked(t, [&] {
        return classify_locked(t, model, d_text, n_bytes, d_doc_offsets, n_docs, flags, d_best, d_best_prob, d_probs, d_hidden, d_stats, d_totals,
                               (hipStream_t)hip_stream);
    });
}

int td_bag_classify(td_tokenizer* t, const td_bag_model* model, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int flags,
                    int32_t* best, float* best_prob, float* probs, float* hidden, int64_t* stats, int64_t* totals) {
    if (!t || !model || !doc_offsets || n_docs < 0 || (n_docs > 0 && (!stats || !best || !best_prob))) return TD_E_INVALID;
    if (!bag_call_flags_ok(flags)) return fail_unlocked(t, TD_E_INVALID, "td_bag_classify: flags must be 0 or TD_BAG_EOS");
    if (model->device != t->device) return fail_unlocked(t, TD_E_INVALID, "td_bag_classify: the model lives on another device");
    return locked(t, [&] {
        int rc;
        hipStream_t s;
        if ((rc = stage_host_text(t, text, doc_offsets, n_docs, s))) return rc;
        const size_t docs = std::max<size_t>((size_t)n_docs, 1), nd = (size_t)n_docs, L = (size_t)model->m.n_labels, dim = (size_t)model->m.dim;
        if ((rc = ensure(t, t->bag_best, docs * 4))) return rc;
        if ((rc = ensure(t, t->bag_bprob, docs * 4))) return rc;
        if ((rc = ensure(t, t->bag_stats, docs * BAG_COLS * 8))) return rc;
        if ((rc = ensure(t, t->bag_totals, BAG_COLS * 8))) return rc;
        if (probs && (rc = ensure(t, t->bag_probs, docs * L * 4))) return rc;
        if (hidden && (rc = ensure(t, t->bag_hidden, docs * dim * 4))) return rc;
        if ((rc = classify_locked(t, model, t->h2d_text.p, doc_offsets[n_docs], t->h2d_offs.p, n_docs, flags, t->bag_best.p, t->bag_bprob.p,
                                  probs ? t->bag_probs.p : nullptr, hidden ? t->bag_hidden.p : nullptr, t->bag_stats.p, t->bag_totals.p, s)))
            return rc;
        if ((rc = device_status_locked(t, s, nullptr))) return rc;
        if (nd && (rc = copy_wait(t, best, t->bag_best.p, nd * 4, hipMemcpyDeviceToHost, s))) return rc;
        if (nd && (rc = copy_wait(t, best_prob, t->bag_bprob.p, nd * 4, hipMemcpyDeviceToHost, s))) return rc;
        if (nd && (rc = copy_wait(t, stats, t->bag_stats.p, nd * BAG_COLS * 8, hipMemcpyDeviceToHost, s))) return rc;
        if (nd && probs && (rc = copy_wait(t, probs, t->bag_probs.p, nd * L * 4, hipMemcpyDeviceToHost, s))) return rc;
        if (nd && hidden && (rc = copy_wait(t, hidden, t->bag_hidden.p, nd * dim * 4, hipMemcpyDeviceToHost, s))) return rc;
        return totals ? copy_wait(t, totals, t->bag_totals.p, BAG_COLS * 8, hipMemcpyDeviceToHost, s) : (int)TD_OK;
    });
}

}  // extern "C"
