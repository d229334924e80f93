// Decode: ids to bytes on the device, for device buffers (td_decode_device) and host buffers (td_decode_bytes, td_decode_batch).
#include "td_handle.h"

namespace {

int decode_args(td_tokenizer* t, const void* d_tokens, int64_t n_tokens, void* d_out, int64_t out_cap, void* d_n_bytes,
                hipStream_t stream, DecodeArgs& a) {
    int rc;
    const int64_t npref = ((n_tokens / 4096 + 4) + 1) & ~1ll;  // even: the offsets behind it stay 16-byte aligned
    if ((rc = ensure(t, t->dec_off, (size_t)(n_tokens + 4) * 4 + (size_t)npref * 8))) return rc;
    memset(&a, 0, sizeof a);
    a.Tp = t->dTp;
    a.tokens = (const int32_t*)d_tokens;
    a.n = n_tokens;
    a.chunk_pref = (int64_t*)t->dec_off.p;                       // 8-byte aligned part first
    a.local_off = (uint32_t*)(a.chunk_pref + npref);
    a.out = (uint8_t*)d_out;
    a.out_cap = out_cap;
    a.n_bytes = (int64_t*)d_n_bytes;
    Ctl* ctl = (Ctl*)t->ctl.p;
    a.scan_done = &ctl->scan_done;
    a.err = &ctl->err;
    a.err_pos = &ctl->err_pos;
    if ((rc = order_before(t, stream))) return rc;
    HIP_TRY(t, hipMemsetAsync(&ctl->scan_done, 0, 4, stream));
    return TD_OK;
}

// decode_bytes on at most SMALL_DEC_MAX_TOKENS ids: ONE launch over pinned host buffers (td_small_decode).  Returns TD_OK, a
// TD_E_* code, or -1: more bytes than the kernel's window holds (the general path takes the call).
int decode_bytes_small(td_tokenizer* t, const int32_t* tokens, int64_t n_tokens, uint8_t* out, int64_t out_capacity, int64_t* n_bytes) {
    if (!t->small_dec_in.p) {  // (both or neither)
        PinnedBuf in, out;
        HIP_TRY(t, make_pinned(in, SMALL_DEC_MAX_TOKENS * 4 + 64));
        HIP_TRY(t, make_pinned(out, 64 + SMALL_DEC_MAX_BYTES));
        memset(out.p, 0, 64 + SMALL_DEC_MAX_BYTES);
        t->small_dec_in = std::move(in);
        t->small_dec_out = std::move(out);
    }
    int rc;
    if ((rc = own_streams(t))) return rc;
    hipStream_t s = t->s_own;
    if ((rc = order_before(t, s))) return rc;
    memcpy(t->small_dec_in.p, tokens, (size_t)n_tokens * 4);
    SmallDecArgs a;
    a.Tp = t->dTp;
    a.tokens = (const int32_t*)t->small_dec_in.p;
    a.status = (SmallStatus*)t->small_dec_out.p;
    a.out = (uint8_t*)t->small_dec_out.p + 64;
    a.seq = ++t->small_seq;
    a.n = (int)n_tokens;
    HIP_TRY(t, launch_small_decode(a, s));
    if ((rc = wait_for_seq(t, &a.status->seq, a.seq, s, 0xFFFu, 5, "td_small_decode did not complete"))) return rc;
    const SmallStatus st = *a.status;
    if (!st.err && st.fallback) { ++t->small_decode_handbacks; return -1; }
    ++t->small_decodes;  // (an error the kernel reported is its answer too)
    if (st.err == TD_E_BAD_TOKEN) {
        const long long ep = st.err_pos;
        t->err = "Invalid token for decoding: " + std::to_string(ep >= 0 && ep < n_tokens ? tokens[ep] : -1);  // reference: tiktoken.cpp:249
        return TD_E_BAD_TOKEN;
    }
    if (st.err) { t->err = "device error " + std::to_string(st.err); return st.err; }
    if (n_bytes) *n_bytes = st.n_tokens;
    if ((int64_t)st.n_tokens > out_capacity) { t->err = "decode capacity too small"; return TD_E_CAPACITY; }
    if (st.n_tokens > 0 && !out) { t->err = "null out"; return TD_E_INVALID; }
    if (st.n_tokens) memcpy(out, a.out, st.n_tokens);
    return TD_OK;
}

// td_decode_bytes (tok_offsets == nullptr) and td_decode_batch on the general path: the ids go up, phase 1 gives lengths and offsets
// (the byte total sizes the device buffer of the gather), phase 2 gathers, the bytes come down.  The batch form also gets the documents'
// byte offsets.  A null `out` with bytes to write: td_decode_bytes refuses it before phase 2, td_decode_batch behind it.
int decode_two_phase(td_tokenizer* t, const int32_t* tokens, int64_t n_tokens, const int64_t* tok_offsets, int64_t n_docs, uint8_t* out,
                     int64_t out_capacity, int64_t* out_offsets, int64_t* n_bytes) {
    int rc;
    if ((rc = ensure(t, t->dec_tokens, (size_t)n_tokens * 4 + 16))) return rc;
    if (tok_offsets) {
        if ((rc = ensure(t, t->h2d_offs, (size_t)(n_docs + 1) * 8))) return rc;
        if ((rc = ensure(t, t->d_offsets, (size_t)(n_docs + 1) * 8))) return rc;
    }
    if ((rc = own_streams(t))) return rc;
    hipStream_t s = t->s_own;
    if ((rc = order_before(t, s))) return rc;
    if (tok_offsets) {
        HIP_TRY(t, hipMemcpyAsync(t->dec_tokens.p, tokens, (size_t)n_tokens * 4, hipMemcpyHostToDevice, s));
        if ((rc = copy_wait(t, t->h2d_offs.p, tok_offsets, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice, s))) return rc;
    } else if ((rc = copy_wait(t, t->dec_tokens.p, tokens, (size_t)n_tokens * 4, hipMemcpyHostToDevice, s))) return rc;
    DecodeArgs a;
    if ((rc = decode_args(t, t->dec_tokens.p, n_tokens, nullptr, INT64_MAX, nullptr, s, a))) return rc;
    if (tok_offsets) {
        a.doc_tok_offsets = (const int64_t*)t->h2d_offs.p;
        a.n_docs = n_docs;
        a.doc_byte_offsets = (int64_t*)t->d_offsets.p;
    }
    HIP_TRY(t, launch_decode(a, s, 1));
    if ((rc = order_after(t, s))) return rc;
    int64_t err_pos = 0;
    rc = device_status_locked(t, s, &err_pos);
    if (rc == TD_E_BAD_TOKEN && err_pos >= 0 && err_pos < n_tokens)
        t->err = "Invalid token for decoding: " + std::to_string(tokens[err_pos]);  // reference: tiktoken.cpp:249
    if (rc) return rc;
    int64_t total;
    if (tok_offsets) {
        if ((rc = copy_wait(t, out_offsets, t->d_offsets.p, (size_t)(n_docs + 1) * 8, hipMemcpyDeviceToHost, s))) return rc;
        total = out_offsets[n_docs];
    } else {
        if ((rc = copy_wait(t, t->h_ctl.p, a.chunk_pref + (n_tokens + 4095) / 4096, 8, hipMemcpyDeviceToHost, s))) return rc;
        total = *(const int64_t*)t->h_ctl.p;
    }
    if (n_bytes) *n_bytes = total;
    if (total > out_capacity) { t->err = "decode capacity too small"; return TD_E_CAPACITY; }
    if (!tok_offsets && total > 0 && !out) { t->err = "null out"; return TD_E_INVALID; }
    if ((rc = ensure(t, t->dec_out, (size_t)total + 16))) return rc;
    a.out = (uint8_t*)t->dec_out.p;
    a.out_cap = total;
    HIP_TRY(t, launch_decode(a, s, 2));
    if ((rc = order_after(t, s))) return rc;
    if ((rc = device_status_locked(t, s, nullptr))) return rc;
    if (total > 0 && !out) { t->err = "null out"; return TD_E_INVALID; }
    return copy_wait(t, out, t->dec_out.p, (size_t)total, hipMemcpyDeviceToHost, s);
}

}  // namespace

extern "C" {

int td_decode_device(td_tokenizer* t, const void* d_tokens, int64_t n_tokens, void* d_out, int64_t out_capacity, void* d_n_bytes,
                     void* hip_stream) {
    if (!t || n_tokens < 0 || (n_tokens > 0 && (!d_tokens || !d_out)) || out_capacity < 0) return TD_E_INVALID;
    return locked(t, [&] {
        hipStream_t s = (hipStream_t)hip_stream;
        if (n_tokens == 0) {
            if (d_n_bytes) HIP_TRY(t, hipMemsetAsync(d_n_bytes, 0, 8, s));
            return (int)TD_OK;
        }
        DecodeArgs a;
        int rc = decode_args(t, d_tokens, n_tokens, d_out, out_capacity, d_n_bytes, s, a);
        if (rc) return rc;
        HIP_TRY(t, launch_decode(a, s, 3));
        return order_after(t, s);
    });
}

int td_decode_bytes(td_tokenizer* t, const int32_t* tokens, int64_t n_tokens, uint8_t* out, int64_t out_capacity,
                    int64_t* n_bytes) {
    if (!t || n_tokens < 0 || (n_tokens > 0 && !tokens)) return TD_E_INVALID;
    if (n_bytes) *n_bytes = 0;
    if (n_tokens == 0) return TD_OK;
    return locked(t, [&] {
        if (n_tokens <= SMALL_DEC_MAX_TOKENS && t->opt.small_enabled) {
            const int rc = decode_bytes_small(t, tokens, n_tokens, out, out_capacity, n_bytes);
            if (rc != -1) return rc;
        }
        return decode_two_phase(t, tokens, n_tokens, nullptr, 0, out, out_capacity, nullptr, n_bytes);
    });
}

int td_decode_batch(td_tokenizer* t, const int32_t* tokens, const int64_t* tok_offsets, int64_t n_docs, uint8_t* out,
                    int64_t out_capacity, int64_t* out_offsets, int64_t* n_bytes) {
    if (!t || !tok_offsets || n_docs < 0 || !out_offsets) return TD_E_INVALID;
    if (n_bytes) *n_bytes = 0;
    return locked(t, [&] {
        int rc;
        if ((rc = check_offsets(t, "tok_offsets", tok_offsets, n_docs, tokens))) return rc;
        const int64_t n_tokens = tok_offsets[n_docs];
        if (n_tokens == 0) {
            for (int64_t d = 0; d <= n_docs; ++d) out_offsets[d] = 0;
            return (int)TD_OK;
        }
        return decode_two_phase(t, tokens, n_tokens, tok_offsets, n_docs, out, out_capacity, out_offsets, n_bytes);
    });
}

}  // extern "C"
