// Decode rows (td_decode_rows.hip): the spec's checks, the per-id table's cache and the entry points.
#include <map>

#include "td_decode_rows_args.h"
#include "td_handle.h"

namespace {

constexpr int64_t DCR_FLAGS = TD_DECODE_KEEP_STOP | TD_DECODE_SKIP_NEGATIVE | TD_DECODE_SKIP_SPECIAL;

// The checks that need no array: nullptr, or what is wrong (bad: the index of a negative listed id, else -1).
const char* dcr_spec_error(const td_decode_spec* sp, int64_t n_tokens, int64_t n_segs, int64_t& bad) {
    bad = -1;
    if (!sp) return "null td_decode_spec";
    if (sp->flags & ~DCR_FLAGS) return "unknown flags";
    if (n_tokens < 0 || n_segs < 0) return "negative n_tokens or n_segs";
    if (sp->row_stride < 0) return "negative row_stride";
    if (sp->n_skip < 0 || sp->n_stop < 0 || (sp->n_skip > 0 && !sp->skip_ids) || (sp->n_stop > 0 && !sp->stop_ids))
        return "a list with a negative size or without its ids";
    if (sp->row_stride > 0 && n_segs > 0 && sp->row_stride > n_tokens / n_segs) return "n_segs * row_stride exceeds n_tokens";
    for (int64_t i = 0; i < sp->n_skip + sp->n_stop; ++i)
        if ((i < sp->n_skip ? sp->skip_ids[i] : sp->stop_ids[i - sp->n_skip]) < 0) {
            bad = i;
            return "a listed id is negative";
        }
    return nullptr;
}

// ... and the arrays', on the host.
const char* dcr_arrays_error(const td_decode_spec* sp, int64_t n_tokens, const int64_t* tok_offsets, const int32_t* seg_len, int64_t n_segs,
                             int64_t& bad) {
    bad = -1;
    if (sp->row_stride == 0) {
        if (!tok_offsets) return "the offsets form needs tok_offsets";
        bad = 0;
        if (tok_offsets[0] < 0) return "tok_offsets[0] is negative";
        for (int64_t d = 0; d < n_segs; ++d)
            if (tok_offsets[d + 1] < tok_offsets[d]) {
                bad = d;
                return "tok_offsets decrease";
            }
        bad = n_segs;
        if (tok_offsets[n_segs] > n_tokens) return "tok_offsets[n_segs] exceeds n_tokens";
    } else if (seg_len) {
        for (int64_t r = 0; r < n_segs; ++r)
            if (seg_len[r] < 0 || seg_len[r] > sp->row_stride) {
                bad = r;
                return "a seg_len is outside [0, row_stride]";
            }
    }
    bad = -1;
    return nullptr;
}

// The table for the spec's lists and flags, in t->dcr_table; rebuilt on `s` only when they differ from the previous call's.  The
// caller has ordered `s` behind the handle's last call (order_before), so no earlier reader is overtaken.  The listed ids travel in
// td_dcr_mark's arguments: nothing of the caller's or the handle's host memory is read after the return.  n_hi: the listed ids above max_id.
int dcr_table_locked(td_tokenizer* t, const td_decode_spec* sp, hipStream_t s, int32_t& n_hi, bool& plain) {
    const bool keep = (sp->flags & TD_DECODE_KEEP_STOP) != 0;
    std::map<int32_t, uint8_t> ids;  // 1 = skip, 2 = stop
    for (int64_t i = 0; i < sp->n_skip; ++i) ids[sp->skip_ids[i]] |= 1;
    for (int64_t i = 0; i < sp->n_stop; ++i) ids[sp->stop_ids[i]] |= keep ? 2 : 3;
    if (sp->flags & TD_DECODE_SKIP_SPECIAL)
        for (int32_t id : t->H.special_ids) ids[id] |= 1;
    plain = ids.empty() && !(sp->flags & TD_DECODE_SKIP_NEGATIVE);
    const int32_t max_id = t->H.max_id;
    std::vector<int64_t> key{sp->flags & TD_DECODE_SKIP_SPECIAL ? 1 : 0};  // (the other flags are in the bits, or no part of the table)
    n_hi = 0;
    for (const auto& e : ids) {
        key.push_back(((int64_t)e.first << 2) | e.second);
        n_hi += e.first > max_id;
    }
    if (n_hi > DCR_MAX_HI) { t->err = "more than 65535 listed ids above the vocabulary"; return TD_E_INVALID; }
    const size_t words = ((size_t)max_id + 2) & ~(size_t)1;  // the listed ids above max_id sit behind the table, 8-byte aligned
    if (key == t->dcr_key && t->dcr_table.p) return TD_OK;
    int rc;
    t->dcr_key.clear();  // (a failure below leaves no table that claims to be built)
    if ((rc = ensure(t, t->dcr_table, words * 4 + (size_t)std::max(n_hi, 1) * sizeof(DcrHi)))) return rc;
    uint32_t* table = (uint32_t*)t->dcr_table.p;
    HIP_TRY(t, launch_decode_rows_table(table, t->dT.tok_off, max_id, s));
    DcrMarkArgs m;
    memset(&m, 0, sizeof m);
    m.table = table;
    m.hi = (DcrHi*)(table + words);
    m.max_id = max_id;
    int hi_at = 0;
    for (const auto& e : ids) {
        m.ids[m.n] = e.first;
        m.bits[m.n] = e.second;
        m.hi_at[m.n] = (uint16_t)(e.first > max_id ? hi_at++ : 0);
        if (++m.n == DCR_MARK_IDS) {
            HIP_TRY(t, launch_decode_rows_mark(m, s));
            m.n = 0;
        }
    }
    if (m.n) HIP_TRY(t, launch_decode_rows_mark(m, s));
    t->dcr_key = std::move(key);
    return TD_OK;
}

// Enqueues the table's rebuild (if any), the zeroing of info and the kernels of `phases` on `s`, which the caller has ordered.
int dcr_launch_locked(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_toff, const void* d_len, int64_t n_segs,
                      const td_decode_spec* sp, void* d_out, int64_t out_cap, void* d_out_off, void* d_seg_ids, void* d_info, int phases,
                      hipStream_t s) {
    int rc;
    int32_t n_hi;
    bool plain;
    if ((rc = dcr_table_locked(t, sp, s, n_hi, plain))) return rc;
    const int64_t tiles = dcr_tiles(sp->row_stride ? n_segs * sp->row_stride : n_tokens);
    if (tiles > 0x7FFFFFF0ll) { t->err = "too many ids for one call"; return TD_E_INVALID; }
    if ((rc = ensure(t, t->dcr_tiles, (size_t)(tiles + 1) * (sizeof(DcrAgg) + 8)))) return rc;
    DecodeRowsArgs a;
    memset(&a, 0, sizeof a);
    a.ids = (const int32_t*)d_ids;
    a.n_tokens = n_tokens;
    a.tok_off = sp->row_stride ? nullptr : (const int64_t*)d_toff;
    a.seg_len = sp->row_stride ? (const int32_t*)d_len : nullptr;
    a.n_segs = n_segs;
    a.row_stride = sp->row_stride;
    a.stride_magic = sp->row_stride ? ~0ull / (unsigned long long)sp->row_stride : 0;
    a.max_id = t->H.max_id;
    a.table = (const uint32_t*)t->dcr_table.p;
    a.hi = (const DcrHi*)(a.table + (((size_t)a.max_id + 2) & ~(size_t)1));
    a.n_hi = n_hi;
    a.skip_negative = (sp->flags & TD_DECODE_SKIP_NEGATIVE) != 0;
    a.n_tiles = (int32_t)tiles;
    a.src_off = t->dT.tok_off;
    a.src_bytes = t->dT.tok_bytes;
    a.base = (unsigned long long*)t->dcr_tiles.p;  // (the 8-byte words first)
    a.agg = (DcrAgg*)(a.base + tiles + 1);
    a.out = (uint8_t*)d_out;
    a.out_cap = out_cap;
    a.out_offsets = (long long*)d_out_off;
    a.seg_ids = (long long*)d_seg_ids;
    a.info = (unsigned long long*)d_info;
    Ctl* ctl = (Ctl*)t->ctl.p;
    a.err = &ctl->err;
    a.err_pos = &ctl->err_pos;
    if (phases & 1) HIP_TRY(t, hipMemsetAsync(d_info, 0, 4 * sizeof(int64_t), s));
    HIP_TRY(t, launch_decode_rows(a, plain, phases, s));
    return order_after(t, s);
}

}  // namespace

extern "C" {

int td_decode_rows_check(const td_decode_spec* spec, int64_t n_tokens, const int64_t* tok_offsets, const int32_t* seg_len, int64_t n_segs,
                         int64_t* bad_pos) {
    int64_t bad;
    const char* m = dcr_spec_error(spec, n_tokens, n_segs, bad);
    if (!m) m = dcr_arrays_error(spec, n_tokens, tok_offsets, seg_len, n_segs, bad);
    if (bad_pos) *bad_pos = m ? bad : 0;
    return m ? TD_E_INVALID : TD_OK;
}

int td_decode_rows_device(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_tok_offsets, const void* d_seg_len,
                          int64_t n_segs, const td_decode_spec* spec, void* d_out, int64_t out_capacity, void* d_out_offsets,
                          void* d_seg_ids, void* d_info, void* hip_stream) {
    if (!t || !d_out_offsets || !d_info || out_capacity < 0 || (out_capacity > 0 && !d_out) ||
        ((((uintptr_t)d_out_offsets) | ((uintptr_t)d_seg_ids) | ((uintptr_t)d_info)) & 7))
        return TD_E_INVALID;
    int64_t bad;
    if (const char* m = dcr_spec_error(spec, n_tokens, n_segs, bad)) return fail_unlocked(t, TD_E_INVALID, std::string("td_decode_rows_device: ") + m);
    if (spec->row_stride == 0 && !d_tok_offsets) return fail_unlocked(t, TD_E_INVALID, "td_decode_rows_device: the offsets form needs d_tok_offsets");
    if (n_tokens > 0 && !d_ids) return fail_unlocked(t, TD_E_INVALID, "td_decode_rows_device: null d_ids");
    return locked(t, [&] {
        hipStream_t s = (hipStream_t)hip_stream;
        int rc;
        if ((rc = order_before(t, s))) return rc;
        return dcr_launch_locked(t, d_ids, n_tokens, d_tok_offsets, d_seg_len, n_segs, spec, d_out, out_capacity, d_out_offsets, d_seg_ids,
                                 d_info, 3, s);
    });
}

int td_decode_rows(td_tokenizer* t, const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets, const int32_t* seg_len, int64_t n_segs,
                   const td_decode_spec* spec, uint8_t* out, int64_t out_capacity, int64_t* out_offsets, int64_t* seg_ids, int64_t* info,
                   int64_t* n_bytes) {
    if (!t || !out_offsets || !info || out_capacity < 0) return TD_E_INVALID;
    if (n_bytes) *n_bytes = 0;
    int64_t bad;
    const char* m = dcr_spec_error(spec, n_tokens, n_segs, bad);
    if (!m) m = dcr_arrays_error(spec, n_tokens, tok_offsets, seg_len, n_segs, bad);
    if (m) return fail_unlocked(t, TD_E_INVALID, std::string("td_decode_rows: ") + m + (bad >= 0 ? " (index " + std::to_string(bad) + ")" : ""));
    const bool rows = spec->row_stride > 0;
    const int64_t used = rows ? n_segs * spec->row_stride : tok_offsets[n_segs];  // the ids the call can visit lie below it
    if (used > 0 && !ids) return fail_unlocked(t, TD_E_INVALID, "td_decode_rows: null ids");
    return locked(t, [&] {
        int rc;
        hipStream_t s;
        const int64_t whole[2] = {0, used};
        if ((rc = rows_stage_host_ids(t, ids, whole, 1, s))) return rc;
        const void* d_toff = nullptr;
        const void* d_len = nullptr;
        if (!rows) {
            if ((rc = ensure(t, t->dcr_off, (size_t)(n_segs + 1) * 8))) return rc;
            HIP_TRY(t, hipMemcpyAsync(t->dcr_off.p, tok_offsets, (size_t)(n_segs + 1) * 8, hipMemcpyHostToDevice, s));
            d_toff = t->dcr_off.p;
        } else if (seg_len && n_segs > 0) {
            if ((rc = ensure(t, t->dcr_len, (size_t)n_segs * 4))) return rc;
            HIP_TRY(t, hipMemcpyAsync(t->dcr_len.p, seg_len, (size_t)n_segs * 4, hipMemcpyHostToDevice, s));
            d_len = t->dcr_len.p;
        }
        if ((rc = ensure(t, t->dcr_out_off, (size_t)(n_segs + 1) * 8))) return rc;
        if ((rc = ensure(t, t->dcr_seg_ids, (size_t)std::max<int64_t>(n_segs, 1) * 8))) return rc;
        if ((rc = ensure(t, t->dcr_info, 4 * sizeof(int64_t)))) return rc;
        void* d_seg = seg_ids ? t->dcr_seg_ids.p : nullptr;
        // the sums and the scan first: the total sizes the device buffer of the bytes
        if ((rc = dcr_launch_locked(t, t->dec_tokens.p, used, d_toff, d_len, n_segs, spec, nullptr, INT64_MAX, t->dcr_out_off.p, d_seg,
                                    t->dcr_info.p, 1, s)))
            return rc;
        if ((rc = device_status_locked(t, s, nullptr))) return rc;
        int64_t total = 0;
        if ((rc = copy_wait(t, &total, (const int64_t*)t->dcr_out_off.p + n_segs, 8, hipMemcpyDeviceToHost, s))) return rc;
        if (n_bytes) *n_bytes = total;
        const bool fits = total <= out_capacity;
        if (fits && total > 0 && !out) { t->err = "null out"; return (int)TD_E_INVALID; }
        if (fits && (rc = ensure(t, t->dec_out, (size_t)total + 16))) return rc;
        if ((rc = dcr_launch_locked(t, t->dec_tokens.p, used, d_toff, d_len, n_segs, spec, fits ? t->dec_out.p : nullptr,
                                    fits ? total : 0, t->dcr_out_off.p, d_seg, t->dcr_info.p, 2, s)))
            return rc;
        int64_t err_pos = 0;
        rc = device_status_locked(t, s, &err_pos);
        if (rc == TD_E_BAD_TOKEN && err_pos >= 0 && err_pos < used) t->err = "Invalid token for decoding: " + std::to_string(ids[err_pos]) + " at index " + std::to_string(err_pos);
        if (rc) return rc;
        if ((rc = copy_wait(t, out_offsets, t->dcr_out_off.p, (size_t)(n_segs + 1) * 8, hipMemcpyDeviceToHost, s))) return rc;
        if (seg_ids && (rc = copy_wait(t, seg_ids, t->dcr_seg_ids.p, (size_t)n_segs * 8, hipMemcpyDeviceToHost, s))) return rc;
        if ((rc = copy_wait(t, info, t->dcr_info.p, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, s))) return rc;
        if (!fits) { t->err = "decode capacity too small: " + std::to_string(total) + " bytes needed"; return (int)TD_E_CAPACITY; }
        return copy_wait(t, out, t->dec_out.p, (size_t)total, hipMemcpyDeviceToHost, s);
    });
}

}  // extern "C"
