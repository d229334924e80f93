// MinHash signatures (td_minhash.hip): the spec's checks, the permutation table, the contract's host statement and the entry points.
#include "td_handle.h"
#include "td_minhash.h"

namespace {

struct MhSpec {
    int k, num_perm, bands, rows;
    uint64_t seed;
};

const char* minhash_spec_error(const td_minhash_spec* sp, bool have_keys, MhSpec& out) {
    if (!sp) return "null td_minhash_spec";
    if (sp->flags != 0) return "flags must be 0";
    if (sp->k < 1 || sp->k > MH_MAX_K) return "k must be in 1 .. 64";
    if (sp->num_perm < 1 || sp->num_perm > MH_MAX_PERM) return "num_perm must be in 1 .. 1024";
    if (sp->bands < 0) return "bands must be >= 0";
    if (sp->bands > 0) {
        if (sp->rows < 1 || sp->bands > sp->num_perm || sp->rows > sp->num_perm || sp->bands * sp->rows > sp->num_perm)
            return "bands * rows must be in 1 .. num_perm";
        if (!have_keys) return "null band_keys with bands >= 1";
    }
    out.k = (int)sp->k;
    out.num_perm = (int)sp->num_perm;
    out.bands = (int)sp->bands;
    out.rows = sp->bands > 0 ? (int)sp->rows : 0;
    out.seed = sp->seed;
    return nullptr;
}

// The handle's table for (seed, num_perm): rebuilt on `s`, by a kernel, only when they differ from the previous call's.  The caller has
// ordered `s` behind the handle's last call (order_before), so no earlier reader is overtaken, and no host memory is read after the
// return.
int minhash_table_locked(td_tokenizer* t, const MhSpec& sp, hipStream_t s) {
    if (t->mh_table.p && t->mh_table_perm == sp.num_perm && t->mh_table_seed == sp.seed) return TD_OK;
    int rc;
    t->mh_table_perm = 0;  // (a failure below leaves no table that claims to be built)
    if ((rc = ensure(t, t->mh_table, (size_t)sp.num_perm * sizeof(MhParam)))) return rc;
    HIP_TRY(t, launch_minhash_params((MhParam*)t->mh_table.p, sp.seed, sp.num_perm, s));
    t->mh_table_perm = sp.num_perm;
    t->mh_table_seed = sp.seed;
    return TD_OK;
}

int minhash_locked(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_toff, int64_t n_docs, const MhSpec& sp, void* d_sig,
                   void* d_keys, void* d_counts, hipStream_t s) {
    int rc;
    if ((rc = order_before(t, s))) return rc;
    if ((rc = ensure(t, t->mh_head, MH_H_WORDS * 8))) return rc;
    if ((rc = minhash_table_locked(t, sp, s))) return rc;
    MhashArgs a;
    memset(&a, 0, sizeof a);
    a.ids = (const int32_t*)d_ids;
    a.n_tokens = n_tokens;
    a.tok_off = (const int64_t*)d_toff;
    a.n_docs = n_docs;
    a.params = (const MhParam*)t->mh_table.p;
    a.k = sp.k;
    a.num_perm = sp.num_perm;
    a.bands = sp.bands;
    a.rows = sp.rows;
    a.sig = (uint32_t*)d_sig;
    a.band_keys = (unsigned long long*)d_keys;
    a.counts = (unsigned long long*)d_counts;
    a.head = (unsigned long long*)t->mh_head.p;
    Ctl* ctl = (Ctl*)t->ctl.p;
    a.err = &ctl->err;
    a.err_pos = &ctl->err_pos;
    HIP_TRY(t, hipMemsetAsync(a.head, 0, MH_H_WORDS * 8, s));
    HIP_TRY(t, launch_minhash(a, s));
    return order_after(t, s);
}

// The host forms' end: `total` ids on the device with their offsets on `s` -> the handle's buffers -> the caller's.
int minhash_to_host(td_tokenizer* t, const void* d_ids, int64_t total, const void* d_toff, int64_t n_docs, const MhSpec& sp, uint32_t* sig,
                    uint64_t* band_keys, int64_t* counts, hipStream_t s) {
    int rc;
    const size_t docs1 = (size_t)std::max<int64_t>(n_docs, 1);
    if ((rc = ensure(t, t->mh_sig, docs1 * (size_t)sp.num_perm * 4))) return rc;
    if (sp.bands && (rc = ensure(t, t->mh_keys, docs1 * (size_t)sp.bands * 8))) return rc;
    if ((rc = ensure(t, t->mh_counts, 4 * sizeof(int64_t)))) return rc;
    if ((rc = minhash_locked(t, d_ids, total, d_toff, n_docs, sp, t->mh_sig.p, sp.bands ? t->mh_keys.p : nullptr, t->mh_counts.p, s))) return rc;
    if ((rc = device_status_locked(t, s, nullptr))) return rc;
    if ((rc = copy_wait(t, counts, t->mh_counts.p, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, s))) return rc;
    if ((rc = copy_wait(t, sig, t->mh_sig.p, (size_t)n_docs * (size_t)sp.num_perm * 4, hipMemcpyDeviceToHost, s))) return rc;
    if (sp.bands && (rc = copy_wait(t, band_keys, t->mh_keys.p, (size_t)n_docs * (size_t)sp.bands * 8, hipMemcpyDeviceToHost, s))) return rc;
    return TD_OK;
}

}  // namespace

extern "C" {

int td_minhash_params(uint64_t seed, int64_t num_perm, uint64_t* a, uint64_t* b) {
    if (num_perm < 1 || num_perm > MH_MAX_PERM || !a || !b) return TD_E_INVALID;
    for (int64_t j = 0; j < num_perm; ++j) {
        const MhParam p = mh_param(seed, j);
        a[j] = p.a;
        b[j] = p.b;
    }
    return TD_OK;
}

int td_minhash_host(const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets, int64_t n_docs, const td_minhash_spec* spec,
                    uint32_t* sig, uint64_t* band_keys, int64_t* counts) {
    MhSpec sp;
    if (!counts || !tok_offsets || n_tokens < 0 || n_docs < 0 || (n_docs > 0 && !sig) || minhash_spec_error(spec, band_keys != nullptr, sp))
        return TD_E_INVALID;
    if (tok_offsets[0] != 0) return TD_E_INVALID;
    for (int64_t d = 0; d < n_docs; ++d)
        if (tok_offsets[d + 1] < tok_offsets[d]) return TD_E_INVALID;
    if (tok_offsets[n_docs] > n_tokens || (tok_offsets[n_docs] > 0 && !ids)) return TD_E_INVALID;
    std::vector<MhParam> par((size_t)sp.num_perm);
    for (int j = 0; j < sp.num_perm; ++j) par[(size_t)j] = mh_param(sp.seed, j);
    memset(counts, 0, 4 * sizeof(int64_t));
    for (int64_t d = 0; d < n_docs; ++d) {
        const int64_t a = tok_offsets[d], L = tok_offsets[d + 1] - a;
        uint32_t* row = sig + d * sp.num_perm;
        for (int j = 0; j < sp.num_perm; ++j) row[j] = 0xFFFFFFFFu;
        const int len = L < sp.k ? (int)L : sp.k;  // the one short shingle is the whole document
        for (int64_t q = a; q < a + mh_shingles(L, sp.k); ++q) {
            const uint32_t x = mh_shingle([&](int i) { return ids[q + i]; }, len);
            for (int j = 0; j < sp.num_perm; ++j) row[j] = std::min(row[j], mh_hash(par[(size_t)j], x));
        }
        for (int b = 0; b < sp.bands; ++b) band_keys[d * sp.bands + b] = mh_band_key(row, b, sp.rows);
        counts[0] += mh_shingles(L, sp.k);
        counts[1] += L == 0;
        counts[2] += L > 0 && L < sp.k;
    }
    return TD_OK;
}

int td_minhash_device(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_tok_offsets, int64_t n_docs,
                      const td_minhash_spec* spec, void* d_sig, void* d_band_keys, void* d_counts, void* hip_stream) {
    if (!t || n_tokens < 0 || n_docs < 0 || !d_tok_offsets || (n_tokens > 0 && !d_ids) || (n_docs > 0 && !d_sig) || !d_counts ||
        ((((uintptr_t)d_counts) | ((uintptr_t)d_band_keys)) & 7) || (((uintptr_t)d_sig) & 3))
        return TD_E_INVALID;
    MhSpec sp;
    if (const char* m = minhash_spec_error(spec, d_band_keys != nullptr, sp)) return fail_unlocked(t, TD_E_INVALID, std::string("td_minhash_device: ") + m);
    if (!hip_stream) return fail_unlocked(t, TD_E_INVALID, "td_minhash_device: hip_stream must not be the null stream");
    return locked(t, [&] { return minhash_locked(t, d_ids, n_tokens, d_tok_offsets, n_docs, sp, d_sig, d_band_keys, d_counts, (hipStream_t)hip_stream); });
}

int td_minhash(td_tokenizer* t, const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets, int64_t n_docs, const td_minhash_spec* spec,
               uint32_t* sig, uint64_t* band_keys, int64_t* counts) {
    if (!t || n_tokens < 0 || n_docs < 0 || !tok_offsets || (n_docs > 0 && !sig) || !counts) return TD_E_INVALID;
    MhSpec sp;
    if (const char* m = minhash_spec_error(spec, band_keys != nullptr, sp)) return fail_unlocked(t, TD_E_INVALID, std::string("td_minhash: ") + m);
    return locked(t, [&] {
        int rc;
        if ((rc = rows_check_host_ids(t, ids, n_tokens, tok_offsets, n_docs))) return rc;
        hipStream_t s;
        if ((rc = rows_stage_host_ids(t, ids, tok_offsets, n_docs, s))) return rc;
        return minhash_to_host(t, t->dec_tokens.p, tok_offsets[n_docs], t->d_offsets.p, n_docs, sp, sig, band_keys, counts, s);
    });
}

int td_encode_batch_minhash(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode,
                            const td_minhash_spec* spec, uint32_t* sig, uint64_t* band_keys, int64_t* counts, int64_t* n_tokens_out) {
    if (!t || !doc_offsets || n_docs < 0 || (n_docs > 0 && !sig) || !counts || (mode != TD_MODE_ENCODE && mode != TD_MODE_ORDINARY)) return TD_E_INVALID;
    MhSpec sp;
    if (const char* m = minhash_spec_error(spec, band_keys != nullptr, sp)) return fail_unlocked(t, TD_E_INVALID, std::string("td_encode_batch_minhash: ") + m);
    return locked(t, [&] {
        int rc;
        int64_t dev_cap;
        hipStream_t s;
        if ((rc = rows_encode_locked(t, text, doc_offsets, n_docs, mode, dev_cap, s))) return rc;
        // the ids made: eight bytes come back, they size the grid and are the caller's total
        int64_t total = 0;
        if ((rc = copy_wait(t, &total, (const int64_t*)t->d_offsets.p + n_docs, 8, hipMemcpyDeviceToHost, s))) return rc;
        if (n_tokens_out) *n_tokens_out = total;
        if (total < 0 || total > dev_cap) { t->err = "the encode's token total is outside its buffer"; return (int)TD_E_INVALID; }
        return minhash_to_host(t, t->d_tokens.p, total, t->d_offsets.p, n_docs, sp, sig, band_keys, counts, s);
    });
}

}  // extern "C"
