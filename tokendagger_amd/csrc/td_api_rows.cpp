// Per-token starts (td_offsets.hip), the four row layouts (td_rows.hip, td_pack.hip, td_windows.hip) and the document selection
// in front of them (td_select.hip): one host path.
#include <type_traits>

#include "td_handle.h"
#include "td_offsets.h"
#include "td_pack.h"
#include "td_rows.h"
#include "td_select.h"
#include "td_windows.h"

namespace {

// ---- per-token starts (td_offsets.hip) -------------------------------------------------------------------------------------
int starts_args(td_tokenizer* t, StartsArgs& a, const void* tokens, const void* tok_off, int64_t n_docs, int64_t n_bound, int kind,
                void* out) {
    int rc;
    const int64_t nch = n_bound / OFF_CHUNK + 2;
    if ((rc = ensure(t, t->off_heads, (size_t)(n_bound / 32 + 2) * 4))) return rc;
    if ((rc = ensure(t, t->off_chunks, (size_t)nch * 12))) return rc;
    memset(&a, 0, sizeof a);
    a.tokens = (const int32_t*)tokens;
    a.tok_off = (const int64_t*)tok_off;
    a.n_docs = n_docs;
    a.n_bound = n_bound;
    a.len_off = t->dT.tok_off;
    a.ctab = t->d_ctab;
    a.max_id = t->H.max_id;
    a.kind = kind;
    a.out = (int64_t*)out;
    a.heads = (uint32_t*)t->off_heads.p;
    a.chunk_sum = (unsigned long long*)t->off_chunks.p;
    a.chunk_head = (uint32_t*)(a.chunk_sum + nch);
    Ctl* ctl = (Ctl*)t->ctl.p;
    a.err = &ctl->err;
    a.err_pos = &ctl->err_pos;
    return TD_OK;
}

int token_starts_locked(td_tokenizer* t, const void* d_tokens, int64_t n_tokens, const void* d_tok_off, int64_t n_docs, int unit, void* d_out,
                        hipStream_t stream) {
    int rc;
    if ((rc = order_before(t, stream))) return rc;
    StartsArgs a;
    if ((rc = starts_args(t, a, d_tokens, d_tok_off, n_docs, n_tokens, unit == TD_UNIT_CHARS ? OFF_CHARS : OFF_BYTES, d_out))) return rc;
    HIP_TRY(t, launch_token_starts(a, stream));
    return order_after(t, stream);
}

// ---- training rows (td_rows.hip, td_pack.hip, td_windows.hip): what the layouts share ----------------------------------------
enum RowsFamily { FAM_ROWS, FAM_BESTFIT, FAM_WINDOWS };  // the layouts an entry point takes: CONCAT / PAD, BESTFIT, WINDOWS

// The checks of a spec that need no handle (nullptr: fine).  overlap: FAM_WINDOWS only; want_cu: cu_seqlens requested.
const char* rows_spec_error(RowsFamily fam, const td_rows_spec* sp, int64_t overlap, int64_t rows_capacity, bool want_cu) {
    if (!sp) return "null td_rows_spec";
    if (fam == FAM_ROWS && sp->layout != TD_ROWS_CONCAT && sp->layout != TD_ROWS_PAD) return "layout must be TD_ROWS_CONCAT or TD_ROWS_PAD";
    if (fam == FAM_BESTFIT && sp->layout != TD_ROWS_BESTFIT) return "layout must be TD_ROWS_BESTFIT";
    if (fam == FAM_WINDOWS && sp->layout != TD_ROWS_WINDOWS) return "layout must be TD_ROWS_WINDOWS";
    if (sp->seq_len < 1 || sp->seq_len > INT32_MAX) return "seq_len must be in 1 .. 2^31 - 1";
    if (fam == FAM_ROWS && (sp->flags & ~(int64_t)TD_ROWS_DROP_LAST)) return "unknown td_rows_spec flags";
    if (fam == FAM_ROWS && (sp->flags & TD_ROWS_DROP_LAST) && sp->layout != TD_ROWS_CONCAT) return "TD_ROWS_DROP_LAST is for TD_ROWS_CONCAT only";
    if (fam == FAM_BESTFIT && (sp->flags & ~(int64_t)TD_ROWS_TRUNCATE)) return "flags must be 0 or TD_ROWS_TRUNCATE";
    if (fam == FAM_WINDOWS && sp->flags != 0) return "flags must be 0";
    if (sp->pad_id < INT32_MIN || sp->pad_id > INT32_MAX) return "pad_id must be an int32";
    const int64_t C = sp->seq_len - (sp->bos_id >= 0) - (sp->eos_id >= 0);  // body room
    if (sp->layout == TD_ROWS_PAD && C < 0) return "TD_ROWS_PAD needs seq_len >= the BOS and EOS slots";
    if (fam == FAM_BESTFIT && (sp->flags & TD_ROWS_TRUNCATE) && C < 0) return "TD_ROWS_TRUNCATE needs seq_len >= the BOS and EOS slots";
    if (fam == FAM_WINDOWS && C < 1) return "seq_len must leave room for one id beside BOS and EOS";
    if (fam == FAM_WINDOWS && (overlap < 0 || overlap >= C)) return "overlap must be in 0 .. seq_len - BOS - EOS - 1";
    if (rows_capacity < 0) return "rows_capacity must be >= 0";
    if (rows_capacity > ((int64_t)1 << 62) / sp->seq_len) return "rows_capacity * seq_len is too large";
    if (want_cu && rows_capacity * sp->seq_len >= ((int64_t)1 << 31))
        return "cu_seqlens entries are int32: rows_capacity * seq_len must stay below 2^31";
    return nullptr;
}

// The outputs struct of a BESTFIT (td_pack_outputs) or WINDOWS (td_window_outputs) entry point, then its spec.
template <class O>
const char* rows_args_error(const td_rows_spec* sp, int64_t overlap, int64_t n_docs, int64_t rows_capacity, const O* o) {
    constexpr bool pack = std::is_same<O, td_pack_outputs>::value;
    if (!o) return pack ? "null td_pack_outputs" : "null td_window_outputs";
    if (n_docs > INT32_MAX) return pack ? "n_docs must be below 2^31" : "n_docs must stay below 2^31";
    if (rows_capacity > 0 && !o->ids) return "null ids output";
    bool want_cu = false;
    if constexpr (pack) want_cu = o->cu_seqlens != nullptr;
    return rows_spec_error(pack ? FAM_BESTFIT : FAM_WINDOWS, sp, overlap, rows_capacity, want_cu);
}

// bos_id / eos_id: -1, or an id of the vocabulary (ordinary or special)
int rows_check_ids(td_tokenizer* t, const td_rows_spec* sp) {
    for (const int64_t id : {sp->bos_id, sp->eos_id}) {
        if (id == -1) continue;
        if (id < 0 || id > INT32_MAX || td_token_bytes(t, (int32_t)id, nullptr, nullptr) != TD_OK)
            return fail_unlocked(t, TD_E_BAD_TOKEN, "td_rows_spec: bos_id / eos_id " + std::to_string(id) + " is not in the vocabulary");
    }
    return TD_OK;
}

// The entry points' step between their null tests and the lock: a spec or outputs error `m` as "<fn>: <m>", then the ids' check.
int rows_spec_fail(td_tokenizer* t, const char* fn, const char* m, const td_rows_spec* sp) {
    if (m) return fail_unlocked(t, TD_E_INVALID, std::string(fn) + ": " + m);
    return rows_check_ids(t, sp);
}

// ---- the label stream of the labeled entry points (td_rows_labels) ---------------------------------------------------------------
// The one checker of a td_rows_labels (no handle); with_ptrs: src and dst are the caller's (not the fused entry's own buffers).
const char* rows_labels_error(const td_rows_labels* lab, int64_t layout, bool with_ptrs) {
    if (!lab) return "null td_rows_labels";
    for (const int64_t v : {lab->bos_value, lab->eos_value, lab->pad_value})
        if (v < INT32_MIN || v > INT32_MAX) return "bos_value, eos_value and pad_value must be int32";
    if (lab->flags & ~(int64_t)TD_ROWLAB_MASK_OVERLAP) return "unknown td_rows_labels flags";
    if ((lab->flags & TD_ROWLAB_MASK_OVERLAP) && layout != TD_ROWS_WINDOWS) return "TD_ROWLAB_MASK_OVERLAP is for TD_ROWS_WINDOWS only";
    if (with_ptrs && !lab->src) return "null td_rows_labels src";
    if (with_ptrs && !lab->dst) return "null td_rows_labels dst";
    return nullptr;
}

// A call's label stream on its way to the kernels: spec null is a one-stream call.  d_src is device memory; dst is the caller's
// (device memory in the device forms, host memory where the rows come back through the handle's buffers).
struct LabCall {
    const td_rows_labels* spec = nullptr;
    const void* d_src = nullptr;
    void* dst = nullptr;
};

// The entry points' step behind rows_spec_fail: nothing for a one-stream call, the label spec's checks for a labeled one.
int rows_lab_fail(td_tokenizer* t, const char* fn, const td_rows_labels* lab, const td_rows_spec* sp, bool labeled) {
    if (!labeled) return TD_OK;
    const char* m = rows_labels_error(lab, sp->layout, true);
    return m ? fail_unlocked(t, TD_E_INVALID, std::string(fn) + ": " + m) : (int)TD_OK;
}

void rows_fill_lab(LabArgs& l, const LabCall& lc, void* d_dst) {  // (behind rows_fill_args: l is zero)
    if (!lc.spec) return;
    l.src = (const int32_t*)lc.d_src;
    l.dst = (int32_t*)d_dst;
    l.bos = (int32_t)lc.spec->bos_value;
    l.eos = (int32_t)lc.spec->eos_value;
    l.pad = (int32_t)lc.spec->pad_value;
    l.mask_overlap = (lc.spec->flags & TD_ROWLAB_MASK_OVERLAP) ? 1 : 0;
}

int64_t rows_needed(const td_rows_spec* sp, int64_t n_ids, int64_t n_docs) {
    if (sp->layout == TD_ROWS_PAD) return n_docs;
    const int64_t T = n_ids + n_docs * ((sp->bos_id >= 0) + (sp->eos_id >= 0));
    return (sp->flags & TD_ROWS_DROP_LAST) ? T / sp->seq_len : (T + sp->seq_len - 1) / sp->seq_len;
}

int rows_funnel_src() {  // TD_ROWS_FUNNEL=1 in the environment: misaligned ids read as aligned int4 and a funnel (A/B)
    static const int v = getenv("TD_ROWS_FUNNEL") && atoi(getenv("TD_ROWS_FUNNEL")) == 1;
    return v;
}

// Zeroes a RowsLabArgs / PackLabArgs / WindowLabArgs and fills the fields they share: the input and the spec's framing.
template <class A>
void rows_fill_args(A& a, const void* d_ids, int64_t n_tokens, const void* d_toff, int64_t n_docs, const td_rows_spec* sp) {
    memset(&a, 0, sizeof a);
    a.ids = (const int32_t*)d_ids;
    a.n_tokens = n_tokens;
    a.tok_off = (const int64_t*)d_toff;
    a.n_docs = n_docs;
    a.S = sp->seq_len;
    a.b = sp->bos_id >= 0;
    a.e = sp->eos_id >= 0;
    a.bos = a.b ? (int32_t)sp->bos_id : 0;
    a.eos = a.e ? (int32_t)sp->eos_id : 0;
    a.pad = (int32_t)sp->pad_id;
}

int rows_launch_locked(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_toff, int64_t n_docs, const td_rows_spec* sp,
                       void* d_out, int64_t cap, void* d_pos, void* d_aux, void* d_counts, const LabCall& lc, hipStream_t s) {
    int rc;
    if ((rc = order_before(t, s))) return rc;
    t->rows_last = true;
    RowsLabArgs a;
    rows_fill_args(a, d_ids, n_tokens, d_toff, n_docs, sp);
    rows_fill_lab(a.lab, lc, lc.dst);
    a.layout = (int)sp->layout;
    a.drop_last = (sp->flags & TD_ROWS_DROP_LAST) ? 1 : 0;
    a.s_magic = ~0ull / (unsigned long long)sp->seq_len;
    a.funnel_src = rows_funnel_src();
    a.out = (int32_t*)d_out;
    a.rows_cap = cap;
    a.pos = (int32_t*)d_pos;
    a.aux = (int32_t*)d_aux;
    a.aux_cap = sp->layout == TD_ROWS_CONCAT ? n_docs + cap + 1 : n_docs;
    a.counts = (long long*)d_counts;
    if (d_aux && sp->layout == TD_ROWS_CONCAT) {
        const size_t bytes = (size_t)rows_scan_words(n_docs) * 8;
        if ((rc = ensure(t, t->rows_scan, bytes))) return rc;
        a.scan = (unsigned long long*)t->rows_scan.p;
        HIP_TRY(t, hipMemsetAsync(a.scan, 0, bytes, s));
    }
    HIP_TRY(t, hipMemsetAsync(d_counts, 0, 4 * sizeof(int64_t), s));
    Ctl* ctl = (Ctl*)t->ctl.p;
    a.err = &ctl->err;
    a.err_pos = &ctl->err_pos;
    HIP_TRY(t, launch_rows(a, s));
    return order_after(t, s);
}

// One output of a host-bound form: made on the device in the handle's buffer `dev`, then copied to the caller's `host`.
struct RowsOut {
    bool want;
    void* host;
    DevBuf* dev;
    size_t elem;              // bytes an element
    int64_t n_alloc, n_copy;  // elements the kernels may write, elements the caller gets
    void* p() const { return want ? dev->p : nullptr; }
};

int rows_out_ensure(td_tokenizer* t, const RowsOut* o, int n) {
    int rc;
    for (int i = 0; i < n; ++i)
        if (o[i].want && (rc = ensure(t, *o[i].dev, (size_t)std::max<int64_t>(o[i].n_alloc, 1) * o[i].elem))) return rc;
    return TD_OK;
}

int rows_out_copy(td_tokenizer* t, const RowsOut* o, int n, hipStream_t s) {
    int rc;
    for (int i = 0; i < n; ++i)
        if (o[i].want && (rc = copy_wait(t, o[i].host, o[i].dev->p, (size_t)o[i].n_copy * o[i].elem, hipMemcpyDeviceToHost, s))) return rc;
    return TD_OK;
}

// Host entry points: rows (known on the host, checked against the capacity by the caller) from ids already on the device, into
// the handle's buffers, then to the caller's.
int rows_to_host(td_tokenizer* t, const void* d_ids, int64_t n_ids, const void* d_toff, int64_t n_docs, const td_rows_spec* sp, int64_t rows,
                 int32_t* out_ids, int32_t* out_pos, int32_t* out_aux, int64_t* counts, const LabCall& lc, hipStream_t s) {
    int rc;
    const bool concat = sp->layout == TD_ROWS_CONCAT;
    const int64_t slots = rows * sp->seq_len;
    RowsOut o[] = {{true, out_ids, &t->rows_out, 4, slots, slots},
                   {out_pos != nullptr, out_pos, &t->rows_pos, 4, slots, slots},
                   {out_aux != nullptr, out_aux, &t->rows_aux, 4, concat ? n_docs + rows + 1 : n_docs, n_docs},
                   {lc.spec != nullptr, lc.dst, &t->rows_lab, 4, slots, slots}};
    if ((rc = rows_out_ensure(t, o, 4))) return rc;
    if ((rc = ensure(t, t->rows_counts, 4 * sizeof(int64_t)))) return rc;
    if ((rc = rows_launch_locked(t, d_ids, n_ids, d_toff, n_docs, sp, o[0].p(), rows, o[1].p(), o[2].p(), t->rows_counts.p,
                                 LabCall{lc.spec, lc.d_src, o[3].p()}, s)))
        return rc;
    if ((rc = device_status_locked(t, s, nullptr))) return rc;
    if ((rc = copy_wait(t, counts, t->rows_counts.p, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, s))) return rc;
    if (concat) o[2].n_copy = counts[2] + 1;  // (cu_seqlens: the segments and the end)
    return rows_out_copy(t, o, 4, s);
}

int rows_capacity_fail(td_tokenizer* t, int64_t rows, int64_t* counts) {
    counts[0] = rows;
    counts[1] = counts[2] = counts[3] = 0;
    t->err = "output capacity too small: " + std::to_string(rows) + " rows needed";
    return TD_E_CAPACITY;
}


}  // namespace

// td_make_rows, td_pack_rows, td_window_rows, td_span_labels: the checks of the caller's ids and offsets (nothing allocated, nothing enqueued) ...
int td::rows_check_host_ids(td_tokenizer* t, const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets, int64_t n_docs) {
    int rc;
    if ((rc = check_offsets(t, "tok_offsets", tok_offsets, n_docs, ids))) return rc;
    if (tok_offsets[n_docs] > n_tokens) { t->err = "tok_offsets[n_docs] exceeds n_tokens"; return TD_E_INVALID; }
    return TD_OK;
}

// ... and their upload into dec_tokens / d_offsets on the handle's own stream `s`.
int td::rows_stage_host_ids(td_tokenizer* t, const int32_t* ids, const int64_t* tok_offsets, int64_t n_docs, hipStream_t& s) {
    int rc;
    const int64_t total = tok_offsets[n_docs];
    if ((rc = ensure(t, t->dec_tokens, (size_t)std::max<int64_t>(total, 1) * 4))) return rc;
    if ((rc = ensure(t, t->d_offsets, (size_t)(n_docs + 1) * 8))) return rc;
    if ((rc = own_streams(t))) return rc;
    s = t->s_own;
    if ((rc = order_before(t, s))) return rc;
    if (total > 0) HIP_TRY(t, hipMemcpyAsync(t->dec_tokens.p, ids, (size_t)total * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(t, hipMemcpyAsync(t->d_offsets.p, tok_offsets, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice, s));
    return TD_OK;
}

namespace {

// The labeled host entry points: the caller's label stream behind its ids, into rows_lab_src on the same stream.
int rows_stage_host_src(td_tokenizer* t, const td_rows_labels* lab, int64_t total, LabCall& lc, hipStream_t s) {
    if (!lab) return TD_OK;
    int rc;
    if ((rc = ensure(t, t->rows_lab_src, (size_t)std::max<int64_t>(total, 1) * 4))) return rc;
    if (total > 0) HIP_TRY(t, hipMemcpyAsync(t->rows_lab_src.p, lab->src, (size_t)total * 4, hipMemcpyHostToDevice, s));
    lc = LabCall{lab, t->rows_lab_src.p, lab->dst};
    return TD_OK;
}

}  // namespace

// td_encode_batch_rows, _pack_rows, _window_rows: the documents encoded on the handle's own stream `s` into d_tokens (room for
// dev_cap ids) / d_offsets, and the encode's errors returned as such, before the rows read its ids.
int td::rows_encode_locked(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode, int64_t& dev_cap,
                       hipStream_t& s) {
    int rc;
    if ((rc = stage_host_text(t, text, doc_offsets, n_docs, s))) return rc;
    const int64_t n = doc_offsets[n_docs];
    dev_cap = std::max<int64_t>(n, 1);  // (at most one id per byte)
    if ((rc = ensure(t, t->d_offsets, (size_t)(n_docs + 1) * 8))) return rc;
    if ((rc = ensure(t, t->d_tokens, (size_t)dev_cap * 4))) return rc;
    if (n > 0) {
        if ((rc = encode_device_locked(t, t->h2d_text.p, n, t->h2d_offs.p, n_docs, mode, t->d_tokens.p, dev_cap, t->d_offsets.p, s))) return rc;
    } else {  // (nothing but empty documents: no encode)
        HIP_TRY(t, hipMemsetAsync(t->d_offsets.p, 0, (size_t)(n_docs + 1) * 8, s));
    }
    return device_status_locked(t, s, nullptr);
}

namespace {

// ---- window rows (td_windows.hip) ---------------------------------------------------------------------------------------------
// w_d = max(1, ceil((L - overlap) / step))
int64_t window_count(int64_t L, int64_t C, int64_t overlap) { return L <= C ? 1 : (L - overlap + (C - overlap) - 1) / (C - overlap); }

// Enqueues the scan and the slot kernel into the outputs of o (device pointers); d_counts is device memory.
int window_launch_locked(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_toff, int64_t n_docs, const td_rows_spec* sp,
                         int64_t overlap, const td_window_outputs& o, int64_t cap, void* d_counts, const LabCall& lc, hipStream_t s) {
    int rc;
    if ((rc = order_before(t, s))) return rc;
    t->rows_last = true;
    WindowLabArgs a;
    rows_fill_args(a, d_ids, n_tokens, d_toff, n_docs, sp);
    rows_fill_lab(a.lab, lc, lc.dst);
    a.C = a.S - a.b - a.e;
    a.overlap = overlap;
    a.step = a.C - overlap;
    a.s_magic = ~0ull / (unsigned long long)a.S;
    a.step_magic = ~0ull / (unsigned long long)a.step;
    a.out = o.ids;
    a.rows_cap = cap;
    a.pos = o.positions;
    a.row_len = o.row_lengths;
    a.row_doc = o.row_docs;
    a.row_start = o.row_starts;
    a.counts = (long long*)d_counts;
    const size_t scan_bytes = (size_t)windows_scan_words(n_docs) * 8;
    if ((rc = ensure(t, t->win_scan, scan_bytes))) return rc;
    if ((rc = ensure(t, t->win_first, (size_t)(n_docs + 1) * 8))) return rc;
    a.scan = (unsigned long long*)t->win_scan.p;
    a.first_row = (int64_t*)t->win_first.p;
    HIP_TRY(t, hipMemsetAsync(a.scan, 0, WIN_SCAN_HEAD * 8, s));
    Ctl* ctl = (Ctl*)t->ctl.p;
    a.err = &ctl->err;
    a.err_pos = &ctl->err_pos;
    HIP_TRY(t, launch_windows(a, s));
    return order_after(t, s);
}

// Host entry points: `rows` rows (known on the host, checked against the capacity by the caller) from ids already on the device,
// into the handle's buffers, then into host_out.
int window_to_host(td_tokenizer* t, const void* d_ids, int64_t n_ids, const void* d_toff, int64_t n_docs, const td_rows_spec* sp,
                   int64_t overlap, const td_window_outputs& ho, int64_t rows, int64_t* counts, const LabCall& lc, hipStream_t s) {
    int rc;
    const int64_t slots = rows * sp->seq_len;
    RowsOut o[] = {{true, ho.ids, &t->rows_out, 4, slots, slots},
                   {ho.positions != nullptr, ho.positions, &t->rows_pos, 4, slots, slots},
                   {ho.row_lengths != nullptr, ho.row_lengths, &t->win_len, 4, rows, rows},
                   {ho.row_docs != nullptr, ho.row_docs, &t->win_docs, 8, rows, rows},
                   {ho.row_starts != nullptr, ho.row_starts, &t->win_starts, 8, rows, rows},
                   {lc.spec != nullptr, lc.dst, &t->rows_lab, 4, slots, slots}};
    if ((rc = rows_out_ensure(t, o, 6))) return rc;
    if ((rc = ensure(t, t->rows_counts, 4 * sizeof(int64_t)))) return rc;
    const td_window_outputs d{(int32_t*)o[0].p(), (int32_t*)o[1].p(), (int32_t*)o[2].p(), (int64_t*)o[3].p(), (int64_t*)o[4].p()};
    if ((rc = window_launch_locked(t, d_ids, n_ids, d_toff, n_docs, sp, overlap, d, rows, t->rows_counts.p,
                                   LabCall{lc.spec, lc.d_src, o[5].p()}, s)))
        return rc;
    if ((rc = device_status_locked(t, s, nullptr))) return rc;
    if ((rc = copy_wait(t, counts, t->rows_counts.p, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, s))) return rc;
    return rows_out_copy(t, o, 6, s);
}

// ---- best-fit packing (td_pack.hip) ------------------------------------------------------------------------------------------
// A document's slots after truncation, its full chunks and its remainder (the one item that is not a full row).
struct PackDoc {
    int64_t n, full, rem;
    bool cut;
};
PackDoc pack_doc(const td_rows_spec* sp, int64_t L) {
    const int64_t S = sp->seq_len, b = sp->bos_id >= 0, e = sp->eos_id >= 0;
    PackDoc p;
    if (sp->flags & TD_ROWS_TRUNCATE) {
        const int64_t body = std::min(L, S - b - e);
        p.n = b + body + e;
        p.full = p.n == S;
        p.rem = p.n == S ? 0 : p.n;
        p.cut = body < L;
    } else {
        p.n = b + L + e;
        p.full = p.n / S;
        p.rem = p.n % S;
        p.cut = p.n > S;
    }
    return p;
}


// The device pipeline up to the plan: items, scan, sort and run-length encode on `s`, one read-back and synchronisation, the
// host plan.  Fills `a` (everything but the outputs and the segment arrays) and counts.  Offsets that are negative, decreasing
// or beyond n_tokens: TD_E_INVALID, nothing launched behind the read-back.
int pack_prepare(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_toff, int64_t n_docs, const td_rows_spec* sp,
                 hipStream_t s, PackLabArgs& a, PackPlan& plan, int64_t* counts) {
    int rc;
    if ((rc = order_before(t, s))) return rc;
    rows_fill_args(a, d_ids, n_tokens, d_toff, n_docs, sp);
    a.truncate = (sp->flags & TD_ROWS_TRUNCATE) ? 1 : 0;
    const size_t nd = (size_t)std::max<int64_t>(n_docs, 1);
    for (DevBuf* b : {&t->pack_key, &t->pack_val, &t->pack_key2, &t->pack_val2})
        if ((rc = ensure(t, *b, nd * 4))) return rc;
    if ((rc = ensure(t, t->pack_full, nd * 8)) || (rc = ensure(t, t->pack_pref, nd * 8))) return rc;
    if ((rc = ensure(t, t->pack_hdr, PACK_HDR * 8 + nd * 8))) return rc;
    a.key = (uint32_t*)t->pack_key.p;
    a.val = (uint32_t*)t->pack_val.p;
    a.full = (int64_t*)t->pack_full.p;
    a.hdr = (long long*)t->pack_hdr.p;
    uint32_t* runs_key = (uint32_t*)(a.hdr + PACK_HDR);
    uint32_t* runs_cnt = runs_key + nd;
    size_t tb = 0;
    HIP_TRY(t, pack_sort_runs(nullptr, tb, a, (uint32_t*)t->pack_key2.p, (uint32_t*)t->pack_val2.p, (int64_t*)t->pack_pref.p, runs_key, runs_cnt, s));
    if ((rc = ensure(t, t->pack_tmp, tb))) return rc;
    HIP_TRY(t, hipMemsetAsync(a.hdr, 0, PACK_HDR * 8, s));
    HIP_TRY(t, launch_pack_items(a, s));
    HIP_TRY(t, pack_sort_runs(t->pack_tmp.p, tb, a, (uint32_t*)t->pack_key2.p, (uint32_t*)t->pack_val2.p, (int64_t*)t->pack_pref.p, runs_key, runs_cnt, s));
    // the header and the first runs in one round trip
    const int64_t k0 = std::min<int64_t>(n_docs, PACK_RUNS_FIRST);
    if ((rc = pinned_ensure(t, t->pack_h, PACK_HDR * 8 + (size_t)k0 * 8))) return rc;
    long long* h = (long long*)t->pack_h.p;
    uint32_t* h_key = (uint32_t*)(h + PACK_HDR);
    uint32_t* h_cnt = h_key + k0;
    HIP_TRY(t, hipMemcpyAsync(h, a.hdr, PACK_HDR * 8, hipMemcpyDeviceToHost, s));
    if (k0 > 0) {
        HIP_TRY(t, hipMemcpyAsync(h_key, runs_key, (size_t)k0 * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(t, hipMemcpyAsync(h_cnt, runs_cnt, (size_t)k0 * 4, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(t, hipStreamSynchronize(s));
    if (h[PH_ERR]) {
        t->err = "tok_offsets: document " + std::to_string(n_docs - h[PH_ERR_DOC]) +
                 " has offsets that are negative, decreasing or beyond n_tokens";
        return TD_E_INVALID;
    }
    const int64_t n_runs = (int64_t)(uint32_t)h[PH_RUNS];
    std::vector<uint32_t> more_key, more_cnt;
    if (n_runs > k0) {  // (S > PACK_RUNS_FIRST and that many distinct lengths)
        more_key.resize(n_runs - k0);
        more_cnt.resize(n_runs - k0);
        if ((rc = copy_wait(t, more_key.data(), runs_key + k0, (size_t)(n_runs - k0) * 4, hipMemcpyDeviceToHost, s))) return rc;
        if ((rc = copy_wait(t, more_cnt.data(), runs_cnt + k0, (size_t)(n_runs - k0) * 4, hipMemcpyDeviceToHost, s))) return rc;
    }
    std::vector<int64_t> lens, cnts;
    for (int64_t r = 0; r < n_runs; ++r) {
        const uint32_t key = r < k0 ? h_key[r] : more_key[r - k0];
        if ((int64_t)key == a.S) continue;  // documents without a remainder item
        lens.push_back(a.S - (int64_t)key);
        cnts.push_back(r < k0 ? h_cnt[r] : more_cnt[r - k0]);
    }
    pack_plan_runs(a.S, h[PH_FULL], h[PH_REAL], lens.data(), cnts.data(), (int64_t)lens.size(), plan);
    a.full_rows = plan.full;
    a.n_mixed = (int64_t)plan.fill.size();
    a.n_items = h[PH_ITEMS];
    a.rows = plan.rows;
    a.segs = plan.segs;
    a.pref = (const int64_t*)t->pack_pref.p;
    a.sorted_doc = (const uint32_t*)t->pack_val2.p;
    counts[0] = plan.rows;
    counts[1] = plan.real;
    counts[2] = plan.segs;
    counts[3] = h[PH_CUT];
    return TD_OK;
}

// Uploads the plan and enqueues td_pack_segments + td_pack_slots into the outputs of o (device pointers).
int pack_emit(td_tokenizer* t, PackLabArgs& a, const PackPlan& plan, const td_pack_outputs& o, const LabCall& lc, hipStream_t s) {
    int rc;
    rows_fill_lab(a.lab, lc, lc.dst);
    const size_t n_pl = plan.pl.size(), n_m = plan.fill.size();
    const size_t up = n_pl * sizeof(PackPlacement) + (n_m + n_m + 1) * 8;
    if ((rc = pinned_ensure(t, t->pack_up, up))) return rc;
    if ((rc = ensure(t, t->pack_plan, up))) return rc;
    char* hp = (char*)t->pack_up.p;
    if (n_pl) memcpy(hp, plan.pl.data(), n_pl * sizeof(PackPlacement));
    if (n_m) memcpy(hp + n_pl * sizeof(PackPlacement), plan.fill.data(), n_m * 8);
    memcpy(hp + n_pl * sizeof(PackPlacement) + n_m * 8, plan.seg0.data(), (n_m + 1) * 8);
    HIP_TRY(t, hipMemcpyAsync(t->pack_plan.p, hp, up, hipMemcpyHostToDevice, s));
    const char* dp = (const char*)t->pack_plan.p;
    a.pl = (const PackPlacement*)dp;
    a.n_pl = (int64_t)n_pl;
    a.fill = (const int64_t*)(dp + n_pl * sizeof(PackPlacement));
    a.seg0 = a.fill + n_m;
    const size_t ns = (size_t)plan.segs + 1;
    if ((rc = ensure(t, t->pack_seg, ns * 8 * 3))) return rc;
    a.seg_start = (int64_t*)t->pack_seg.p;
    a.seg_doc = a.seg_start + ns;
    a.seg_q0 = a.seg_doc + ns;
    a.out = o.ids;
    a.pos = o.positions;
    a.cu = o.cu_seqlens;
    a.lengths = o.row_lengths;
    a.docs = o.seg_docs;
    HIP_TRY(t, launch_pack_outputs(a, s));
    return order_after(t, s);
}

// Host entry points: packs ids already on the device into the handle's buffers, then copies them into host_out.
int pack_to_host(td_tokenizer* t, const void* d_ids, int64_t n_ids, const void* d_toff, int64_t n_docs, const td_rows_spec* sp,
                 const td_pack_outputs& ho, int64_t cap, int64_t* counts, const LabCall& lc, hipStream_t s) {
    int rc;
    PackLabArgs a;
    PackPlan plan;
    if ((rc = pack_prepare(t, d_ids, n_ids, d_toff, n_docs, sp, s, a, plan, counts))) return rc;
    if (plan.rows > cap) return rows_capacity_fail(t, plan.rows, counts);
    const int64_t slots = plan.rows * sp->seq_len;
    const RowsOut o[] = {{true, ho.ids, &t->rows_out, 4, slots, slots},
                         {ho.positions != nullptr, ho.positions, &t->rows_pos, 4, slots, slots},
                         {ho.cu_seqlens != nullptr, ho.cu_seqlens, &t->rows_aux, 4, plan.segs + 1, plan.segs + 1},
                         {ho.row_lengths != nullptr, ho.row_lengths, &t->pack_len, 4, plan.rows, plan.rows},
                         {ho.seg_docs != nullptr, ho.seg_docs, &t->pack_docs, 8, plan.segs + 1, plan.segs},
                         {lc.spec != nullptr, lc.dst, &t->rows_lab, 4, slots, slots}};
    if ((rc = rows_out_ensure(t, o, 6))) return rc;
    const td_pack_outputs d{(int32_t*)o[0].p(), (int32_t*)o[1].p(), (int32_t*)o[2].p(), (int32_t*)o[3].p(), (int64_t*)o[4].p()};
    if ((rc = pack_emit(t, a, plan, d, LabCall{lc.spec, lc.d_src, o[5].p()}, s))) return rc;
    if ((rc = rows_out_copy(t, o, 6, s))) return rc;
    HIP_TRY(t, hipStreamSynchronize(s));  // (nothing copied at all: the kernels are still done when the call returns)
    return TD_OK;
}

}  // namespace

// Behind encode_device_locked, on the same stream: the generic engine's bitmaps in the workspace are still those of this call.
// Starts by the covered rule (chars: bytes and characters packed, every document checked against its length), then the documents
// with skipped text through the covered-byte bitmap.
int td::encode_starts_locked(td_tokenizer* t, const void* d_text, int64_t n, const void* d_offs, int64_t n_docs, const void* d_tokens,
                             int64_t cap, const void* d_out_offs, int unit, void* d_starts, hipStream_t stream) {
    const int64_t bound = std::min(cap, n);
    if (bound <= 0 || n_docs <= 0) return TD_OK;  // (no ids; a capacity too small for the ids is the encode's error)
    const bool chars = unit == TD_UNIT_CHARS, generic = t->H.pattern_kind == PATTERN_GENERIC;
    int rc;
    StartsArgs a;
    if ((rc = starts_args(t, a, d_tokens, d_out_offs, n_docs, bound, chars ? OFF_PAIR : OFF_BYTES, d_starts))) return rc;
    if ((rc = ensure(t, t->off_docs, (size_t)n_docs + 16))) return rc;
    a.text = (const uint8_t*)d_text;
    a.n = n;
    a.doc_off = (const int64_t*)d_offs;
    a.doc_gap = (uint8_t*)t->off_docs.p;
    a.generic = generic ? 1 : 0;
    a.chars = chars ? 1 : 0;
    if (generic) {
        if ((rc = ensure(t, t->off_rank, off_rank_bytes(n)))) return rc;
        off_rank_layout(a, t->off_rank.p, n);
        a.startbits = (const uint32_t*)t->startbits.p;
        a.gapbits = (const uint32_t*)t->gapbits.p;
    }
    HIP_TRY(t, launch_token_starts(a, stream));
    HIP_TRY(t, launch_encode_starts(a, stream));
    return order_after(t, stream);
}

// td_encode_batch_span_label_rows (td_api_labels.cpp): the checks of its row arguments, nothing allocated or enqueued ...
int td::label_rows_check(td_tokenizer* t, const char* fn, const td_rows_spec* sp, int64_t overlap, int64_t n_docs, const td_rows_labels* lab,
                         const td_label_rows_outputs* o, int64_t rows_capacity) {
    const char* m = nullptr;
    if (!sp) m = "null td_rows_spec";
    else if (!o) m = "null td_label_rows_outputs";
    else if (sp->layout < TD_ROWS_CONCAT || sp->layout > TD_ROWS_WINDOWS) m = "unknown layout";
    else if (rows_capacity > 0 && !o->labels) m = "null labels output";
    else if (sp->layout <= TD_ROWS_PAD) {
        if (o->row_lengths || o->seg_docs || o->row_docs || o->row_starts) m = "TD_ROWS_CONCAT / TD_ROWS_PAD have ids, labels, positions and aux only";
        else if (rows_capacity > 0 && !o->ids) m = "null ids output";
        else m = rows_spec_error(FAM_ROWS, sp, 0, rows_capacity, sp->layout == TD_ROWS_CONCAT && o->aux);
    } else if (sp->layout == TD_ROWS_BESTFIT) {
        const td_pack_outputs po{o->ids, o->positions, o->aux, o->row_lengths, o->seg_docs};
        m = o->row_docs || o->row_starts ? "TD_ROWS_BESTFIT has no row_docs and no row_starts" : rows_args_error(sp, 0, n_docs, rows_capacity, &po);
    } else {
        const td_window_outputs wo{o->ids, o->positions, o->row_lengths, o->row_docs, o->row_starts};
        m = o->aux || o->seg_docs ? "TD_ROWS_WINDOWS has no aux and no seg_docs" : rows_args_error(sp, overlap, n_docs, rows_capacity, &wo);
    }
    if (int rc = rows_spec_fail(t, fn, m, sp)) return rc;
    m = rows_labels_error(lab, sp->layout, false);
    return m ? fail_unlocked(t, TD_E_INVALID, std::string(fn) + ": " + m) : (int)TD_OK;
}

// ... and the labeled row call of sp->layout (checked by label_rows_check) on `total` ids and labels already on the device, on `s`:
// the host path of td_make_rows_labeled / td_pack_rows_labeled / td_window_rows_labeled behind their staging.
int td::label_rows_to_host(td_tokenizer* t, const void* d_ids, const void* d_src, const void* d_toff, const int64_t* h_toff, int64_t n_docs,
                           const td_rows_spec* sp, int64_t overlap, const td_rows_labels* lab, const td_label_rows_outputs& o,
                           int64_t rows_capacity, int64_t* counts, hipStream_t s) {
    const int64_t total = h_toff[n_docs];
    const LabCall lc{lab, d_src, o.labels};
    if (sp->layout == TD_ROWS_BESTFIT)
        return pack_to_host(t, d_ids, total, d_toff, n_docs, sp, td_pack_outputs{o.ids, o.positions, o.aux, o.row_lengths, o.seg_docs},
                            rows_capacity, counts, lc, s);
    if (sp->layout == TD_ROWS_WINDOWS) {
        int64_t plan[4];
        if (td_window_plan(h_toff, n_docs, sp, overlap, plan, nullptr) != TD_OK) { t->err = "invalid token offsets"; return TD_E_INVALID; }
        if (plan[0] > rows_capacity) return rows_capacity_fail(t, plan[0], counts);
        return window_to_host(t, d_ids, total, d_toff, n_docs, sp, overlap,
                              td_window_outputs{o.ids, o.positions, o.row_lengths, o.row_docs, o.row_starts}, plan[0], counts, lc, s);
    }
    const int64_t rows = rows_needed(sp, total, n_docs);
    if (rows > rows_capacity) return rows_capacity_fail(t, rows, counts);
    return rows_to_host(t, d_ids, total, d_toff, n_docs, sp, rows, o.ids, o.positions, o.aux, counts, lc, s);
}

extern "C" {

int td_token_starts(td_tokenizer* t, const int32_t* tokens, int64_t n_tokens, const int64_t* tok_offsets, int64_t n_docs, int unit,
                    int64_t* out_starts) {
    if (!t || n_tokens < 0 || (n_tokens > 0 && (!tokens || !out_starts)) || !tok_offsets || n_docs < 0 ||
        (unit != TD_UNIT_BYTES && unit != TD_UNIT_CHARS))
        return TD_E_INVALID;
    return locked(t, [&] {
        int rc;
        if ((rc = check_offsets(t, "tok_offsets", tok_offsets, n_docs, tokens))) return rc;
        const int64_t total = tok_offsets[n_docs];
        if (total > n_tokens) { t->err = "output capacity too small: " + std::to_string(total) + " starts needed"; return (int)TD_E_CAPACITY; }
        if (total == 0) return (int)TD_OK;
        if ((rc = ensure(t, t->dec_tokens, (size_t)total * 4))) return rc;
        if ((rc = ensure(t, t->d_offsets, (size_t)(n_docs + 1) * 8))) return rc;
        if ((rc = ensure(t, t->off_starts, (size_t)total * 8))) return rc;
        if ((rc = own_streams(t))) return rc;
        hipStream_t s = t->s_own;
        if ((rc = order_before(t, s))) return rc;
        HIP_TRY(t, hipMemcpyAsync(t->dec_tokens.p, tokens, (size_t)total * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(t, hipMemcpyAsync(t->d_offsets.p, tok_offsets, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice, s));
        if ((rc = token_starts_locked(t, t->dec_tokens.p, total, t->d_offsets.p, n_docs, unit, t->off_starts.p, s))) return rc;
        if ((rc = device_status_locked(t, s, nullptr))) return rc;
        return copy_wait(t, out_starts, t->off_starts.p, (size_t)total * 8, hipMemcpyDeviceToHost, s);
    });
}

int td_token_starts_device(td_tokenizer* t, const void* d_tokens, int64_t n_tokens, const void* d_tok_offsets, int64_t n_docs, int unit,
                           void* d_out_starts, void* hip_stream) {
    if (!t || n_tokens < 0 || (n_tokens > 0 && (!d_tokens || !d_out_starts)) || !d_tok_offsets || n_docs < 0 ||
        (unit != TD_UNIT_BYTES && unit != TD_UNIT_CHARS))
        return TD_E_INVALID;
    return locked(t, [&] {
        return token_starts_locked(t, d_tokens, n_tokens, d_tok_offsets, n_docs, unit, d_out_starts, (hipStream_t)hip_stream);
    });
}

int td_encode_device_with_starts(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_doc_offsets, int64_t n_docs, int mode,
                                 int unit, void* d_out_tokens, int64_t out_capacity, void* d_out_offsets, void* d_out_starts,
                                 void* hip_stream) {
    if (!t || (unit != TD_UNIT_BYTES && unit != TD_UNIT_CHARS) || (n_bytes > 0 && out_capacity > 0 && !d_out_starts)) return TD_E_INVALID;
    if (unit == TD_UNIT_CHARS && n_bytes >= (1ll << 32))
        return fail_unlocked(t, TD_E_INVALID, "td_encode_device_with_starts: character starts need less than 4 GiB of text a call");
    return locked(t, [&] {
        const hipStream_t s = (hipStream_t)hip_stream;
        int rc = encode_device_locked(t, d_text, n_bytes, d_doc_offsets, n_docs, mode, d_out_tokens, out_capacity, d_out_offsets, s);
        if (rc) return rc;
        return encode_starts_locked(t, d_text, n_bytes, d_doc_offsets, n_docs, d_out_tokens, out_capacity, d_out_offsets, unit, d_out_starts, s);
    });
}

// Every entry point with a labeled form is one function: `fn` names the form called, lab is its td_rows_labels (labeled) or
// nothing.  The label spec is checked behind the counterpart's own checks, before the lock and any launch.
static int make_rows_device_any(const char* fn, bool labeled, td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_tok_offsets,
                                int64_t n_docs, const td_rows_spec* spec, void* d_out_ids, int64_t rows_capacity, void* d_positions,
                                void* d_aux, void* d_counts, void* hip_stream, const td_rows_labels* lab) {
    if (!t || !spec || n_tokens < 0 || n_docs < 0 || !d_tok_offsets || (n_tokens > 0 && !d_ids) || !d_counts ||
        (rows_capacity > 0 && !d_out_ids))
        return TD_E_INVALID;
    if (int rc = rows_spec_fail(t, fn, rows_spec_error(FAM_ROWS, spec, 0, rows_capacity, spec->layout == TD_ROWS_CONCAT && d_aux), spec)) return rc;
    if (int rc = rows_lab_fail(t, fn, lab, spec, labeled)) return rc;
    return locked(t, [&] {
        return rows_launch_locked(t, d_ids, n_tokens, d_tok_offsets, n_docs, spec, d_out_ids, rows_capacity, d_positions, d_aux, d_counts,
                                  labeled ? LabCall{lab, lab->src, lab->dst} : LabCall{}, (hipStream_t)hip_stream);
    });
}

int td_make_rows_device(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_tok_offsets, int64_t n_docs,
                        const td_rows_spec* spec, void* d_out_ids, int64_t rows_capacity, void* d_positions, void* d_aux,
                        void* d_counts, void* hip_stream) {
    return make_rows_device_any("td_make_rows_device", false, t, d_ids, n_tokens, d_tok_offsets, n_docs, spec, d_out_ids, rows_capacity,
                                d_positions, d_aux, d_counts, hip_stream, nullptr);
}

int td_make_rows_labeled_device(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_tok_offsets, int64_t n_docs,
                                const td_rows_spec* spec, void* d_out_ids, int64_t rows_capacity, void* d_positions, void* d_aux,
                                void* d_counts, void* hip_stream, const td_rows_labels* lab) {
    return make_rows_device_any("td_make_rows_labeled_device", true, t, d_ids, n_tokens, d_tok_offsets, n_docs, spec, d_out_ids,
                                rows_capacity, d_positions, d_aux, d_counts, hip_stream, lab);
}

static int make_rows_any(const char* fn, bool labeled, td_tokenizer* t, const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets,
                         int64_t n_docs, const td_rows_spec* spec, int32_t* out_ids, int64_t rows_capacity, int32_t* out_positions,
                         int32_t* out_aux, int64_t* counts, const td_rows_labels* lab) {
    if (!t || !spec || n_tokens < 0 || n_docs < 0 || !tok_offsets || !counts || (rows_capacity > 0 && !out_ids)) return TD_E_INVALID;
    if (int rc = rows_spec_fail(t, fn, rows_spec_error(FAM_ROWS, spec, 0, rows_capacity, spec->layout == TD_ROWS_CONCAT && out_aux), spec)) return rc;
    if (int rc = rows_lab_fail(t, fn, lab, spec, labeled)) return rc;
    return locked(t, [&] {
        int rc2;
        if ((rc2 = rows_check_host_ids(t, ids, n_tokens, tok_offsets, n_docs))) return rc2;
        const int64_t total = tok_offsets[n_docs];
        const int64_t rows = rows_needed(spec, total, n_docs);
        if (rows > rows_capacity) return rows_capacity_fail(t, rows, counts);
        hipStream_t s;
        LabCall lc;
        if ((rc2 = rows_stage_host_ids(t, ids, tok_offsets, n_docs, s))) return rc2;
        if ((rc2 = rows_stage_host_src(t, lab, total, lc, s))) return rc2;
        return rows_to_host(t, t->dec_tokens.p, total, t->d_offsets.p, n_docs, spec, rows, out_ids, out_positions, out_aux, counts, lc, s);
    });
}

int td_make_rows(td_tokenizer* t, const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets, int64_t n_docs,
                 const td_rows_spec* spec, int32_t* out_ids, int64_t rows_capacity, int32_t* out_positions, int32_t* out_aux,
                 int64_t* counts) {
    return make_rows_any("td_make_rows", false, t, ids, n_tokens, tok_offsets, n_docs, spec, out_ids, rows_capacity, out_positions, out_aux,
                         counts, nullptr);
}

int td_make_rows_labeled(td_tokenizer* t, const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets, int64_t n_docs,
                         const td_rows_spec* spec, int32_t* out_ids, int64_t rows_capacity, int32_t* out_positions, int32_t* out_aux,
                         int64_t* counts, const td_rows_labels* lab) {
    return make_rows_any("td_make_rows_labeled", true, t, ids, n_tokens, tok_offsets, n_docs, spec, out_ids, rows_capacity, out_positions,
                         out_aux, counts, lab);
}

int td_encode_batch_rows(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode,
                         const td_rows_spec* spec, int32_t* out_ids, int64_t rows_capacity, int32_t* out_positions, int32_t* out_aux,
                         int64_t* counts) {
    if (!t || !spec || !doc_offsets || n_docs < 0 || !counts || (rows_capacity > 0 && !out_ids) ||
        (mode != TD_MODE_ENCODE && mode != TD_MODE_ORDINARY))
        return TD_E_INVALID;
    if (int rc = rows_spec_fail(t, "td_encode_batch_rows",
                                rows_spec_error(FAM_ROWS, spec, 0, rows_capacity, spec->layout == TD_ROWS_CONCAT && out_aux), spec)) return rc;
    return locked(t, [&] {
        int rc2;
        int64_t dev_cap;
        hipStream_t s;
        if ((rc2 = rows_encode_locked(t, text, doc_offsets, n_docs, mode, dev_cap, s))) return rc2;
        int64_t total = 0;
        if ((rc2 = copy_wait(t, &total, (const int64_t*)t->d_offsets.p + n_docs, 8, hipMemcpyDeviceToHost, s))) return rc2;
        const int64_t rows = rows_needed(spec, total, n_docs);
        if (rows > rows_capacity) return rows_capacity_fail(t, rows, counts);
        return rows_to_host(t, t->d_tokens.p, dev_cap, t->d_offsets.p, n_docs, spec, rows, out_ids, out_positions, out_aux, counts, LabCall{}, s);
    });
}

int td_pack_plan(const int64_t* tok_offsets, int64_t n_docs, const td_rows_spec* spec, int64_t* counts, int64_t* doc_row,
                 int64_t* doc_slot) {
    if (!tok_offsets || n_docs < 0 || n_docs > INT32_MAX || !counts || rows_spec_error(FAM_BESTFIT, spec, 0, 0, false)) return TD_E_INVALID;
    if (tok_offsets[0] != 0) return TD_E_INVALID;
    for (int64_t d = 0; d < n_docs; ++d)
        if (tok_offsets[d + 1] < tok_offsets[d]) return TD_E_INVALID;
    const int64_t S = spec->seq_len;
    std::vector<int64_t> rem((size_t)n_docs), order;
    int64_t F = 0, R = 0, cut = 0;
    for (int64_t d = 0; d < n_docs; ++d) {
        const PackDoc p = pack_doc(spec, tok_offsets[d + 1] - tok_offsets[d]);
        if (doc_row) doc_row[d] = p.full == 1 && p.rem == 0 ? F : -1;  // (a document that is exactly one full row)
        if (doc_slot) doc_slot[d] = p.full == 1 && p.rem == 0 ? 0 : -1;
        rem[d] = p.rem;
        F += p.full;
        R += p.n;
        cut += p.cut;
        if (p.rem) order.push_back(d);
    }
    std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return rem[x] > rem[y]; });
    std::vector<int64_t> lens, cnts;
    for (const int64_t d : order) {
        if (lens.empty() || lens.back() != rem[d]) { lens.push_back(rem[d]); cnts.push_back(0); }
        ++cnts.back();
    }
    PackPlan plan;
    pack_plan_runs(S, F, R, lens.data(), cnts.data(), (int64_t)lens.size(), plan);
    if (doc_row || doc_slot)
        for (const PackPlacement& p : plan.pl)
            for (int64_t j = 0; j < p.count; ++j) {
                const int64_t d = order[p.first_item + j];
                if (doc_row) doc_row[d] = p.row;
                if (doc_slot) doc_slot[d] = p.slot + j * p.len;
            }
    counts[0] = plan.rows;
    counts[1] = R;
    counts[2] = plan.segs;
    counts[3] = cut;
    return TD_OK;
}

static int pack_rows_any(const char* fn, bool labeled, td_tokenizer* t, const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets,
                         int64_t n_docs, const td_rows_spec* spec, const td_pack_outputs* host_out, int64_t rows_capacity, int64_t* counts,
                         const td_rows_labels* lab) {
    if (!t || !spec || !host_out || n_tokens < 0 || n_docs < 0 || !tok_offsets || !counts) return TD_E_INVALID;
    if (int rc = rows_spec_fail(t, fn, rows_args_error(spec, 0, n_docs, rows_capacity, host_out), spec)) return rc;
    if (int rc = rows_lab_fail(t, fn, lab, spec, labeled)) return rc;
    return locked(t, [&] {
        int rc2;
        if ((rc2 = rows_check_host_ids(t, ids, n_tokens, tok_offsets, n_docs))) return rc2;
        const int64_t total = tok_offsets[n_docs];
        hipStream_t s;
        LabCall lc;
        if ((rc2 = rows_stage_host_ids(t, ids, tok_offsets, n_docs, s))) return rc2;
        if ((rc2 = rows_stage_host_src(t, lab, total, lc, s))) return rc2;
        return pack_to_host(t, t->dec_tokens.p, total, t->d_offsets.p, n_docs, spec, *host_out, rows_capacity, counts, lc, s);
    });
}

int td_pack_rows(td_tokenizer* t, const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets, int64_t n_docs,
                 const td_rows_spec* spec, const td_pack_outputs* host_out, int64_t rows_capacity, int64_t* counts) {
    return pack_rows_any("td_pack_rows", false, t, ids, n_tokens, tok_offsets, n_docs, spec, host_out, rows_capacity, counts, nullptr);
}

int td_pack_rows_labeled(td_tokenizer* t, const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets, int64_t n_docs,
                         const td_rows_spec* spec, const td_pack_outputs* host_out, int64_t rows_capacity, int64_t* counts,
                         const td_rows_labels* lab) {
    return pack_rows_any("td_pack_rows_labeled", true, t, ids, n_tokens, tok_offsets, n_docs, spec, host_out, rows_capacity, counts, lab);
}

static int pack_rows_device_any(const char* fn, bool labeled, td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_tok_offsets,
                                int64_t n_docs, const td_rows_spec* spec, const td_pack_outputs* dev_out, int64_t rows_capacity,
                                int64_t* counts, void* hip_stream, const td_rows_labels* lab) {
    if (!t || !spec || !dev_out || n_tokens < 0 || n_docs < 0 || !d_tok_offsets || (n_tokens > 0 && !d_ids) || !counts)
        return TD_E_INVALID;
    if (int rc = rows_spec_fail(t, fn, rows_args_error(spec, 0, n_docs, rows_capacity, dev_out), spec)) return rc;
    if (int rc = rows_lab_fail(t, fn, lab, spec, labeled)) return rc;
    return locked(t, [&] {
        hipStream_t s = (hipStream_t)hip_stream;
        PackLabArgs a;
        PackPlan plan;
        int rc2;
        if ((rc2 = pack_prepare(t, d_ids, n_tokens, d_tok_offsets, n_docs, spec, s, a, plan, counts))) return rc2;
        if (plan.rows > rows_capacity) return rows_capacity_fail(t, plan.rows, counts);
        return pack_emit(t, a, plan, *dev_out, labeled ? LabCall{lab, lab->src, lab->dst} : LabCall{}, s);
    });
}

int td_pack_rows_device(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_tok_offsets, int64_t n_docs,
                        const td_rows_spec* spec, const td_pack_outputs* dev_out, int64_t rows_capacity, int64_t* counts,
                        void* hip_stream) {
    return pack_rows_device_any("td_pack_rows_device", false, t, d_ids, n_tokens, d_tok_offsets, n_docs, spec, dev_out, rows_capacity, counts,
                                hip_stream, nullptr);
}

int td_pack_rows_labeled_device(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_tok_offsets, int64_t n_docs,
                                const td_rows_spec* spec, const td_pack_outputs* dev_out, int64_t rows_capacity, int64_t* counts,
                                void* hip_stream, const td_rows_labels* lab) {
    return pack_rows_device_any("td_pack_rows_labeled_device", true, t, d_ids, n_tokens, d_tok_offsets, n_docs, spec, dev_out, rows_capacity,
                                counts, hip_stream, lab);
}

int td_encode_batch_pack_rows(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode,
                              const td_rows_spec* spec, const td_pack_outputs* host_out, int64_t rows_capacity, int64_t* counts) {
    if (!t || !spec || !host_out || !doc_offsets || n_docs < 0 || !counts || (mode != TD_MODE_ENCODE && mode != TD_MODE_ORDINARY))
        return TD_E_INVALID;
    if (int rc = rows_spec_fail(t, "td_encode_batch_pack_rows", rows_args_error(spec, 0, n_docs, rows_capacity, host_out), spec)) return rc;
    return locked(t, [&] {
        int rc2;
        int64_t dev_cap;
        hipStream_t s;
        if ((rc2 = rows_encode_locked(t, text, doc_offsets, n_docs, mode, dev_cap, s))) return rc2;
        return pack_to_host(t, t->d_tokens.p, dev_cap, t->d_offsets.p, n_docs, spec, *host_out, rows_capacity, counts, LabCall{}, s);
    });
}

int td_window_plan(const int64_t* tok_offsets, int64_t n_docs, const td_rows_spec* spec, int64_t overlap, int64_t* counts,
                   int64_t* first_row) {
    if (!tok_offsets || n_docs < 0 || n_docs > INT32_MAX || !counts || rows_spec_error(FAM_WINDOWS, spec, overlap, 0, false)) return TD_E_INVALID;
    if (tok_offsets[0] != 0) return TD_E_INVALID;
    const int64_t k = (spec->bos_id >= 0) + (spec->eos_id >= 0), C = spec->seq_len - k;
    int64_t rows = 0, R = 0, multi = 0, mx = 0;
    for (int64_t d = 0; d < n_docs; ++d) {
        const int64_t L = tok_offsets[d + 1] - tok_offsets[d];
        if (L < 0) return TD_E_INVALID;
        const int64_t w = window_count(L, C, overlap);
        if (first_row) first_row[d] = rows;
        rows += w;
        R += w * k + L + (w - 1) * overlap;
        multi += w > 1;
        mx = std::max(mx, w);
    }
    if (first_row) first_row[n_docs] = rows;
    counts[0] = rows;
    counts[1] = R;
    counts[2] = multi;
    counts[3] = mx;
    return TD_OK;
}

static int window_rows_device_any(const char* fn, bool labeled, td_tokenizer* t, const void* d_ids, int64_t n_tokens,
                                  const void* d_tok_offsets, int64_t n_docs, const td_rows_spec* spec, int64_t overlap,
                                  const td_window_outputs* dev_out, int64_t rows_capacity, void* d_counts, void* hip_stream,
                                  const td_rows_labels* lab) {
    if (!t || !spec || !dev_out || n_tokens < 0 || n_docs < 0 || !d_tok_offsets || (n_tokens > 0 && !d_ids) || !d_counts)
        return TD_E_INVALID;
    if (int rc = rows_spec_fail(t, fn, rows_args_error(spec, overlap, n_docs, rows_capacity, dev_out), spec)) return rc;
    if (int rc = rows_lab_fail(t, fn, lab, spec, labeled)) return rc;
    return locked(t, [&] {
        return window_launch_locked(t, d_ids, n_tokens, d_tok_offsets, n_docs, spec, overlap, *dev_out, rows_capacity, d_counts,
                                    labeled ? LabCall{lab, lab->src, lab->dst} : LabCall{}, (hipStream_t)hip_stream);
    });
}

int td_window_rows_device(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_tok_offsets, int64_t n_docs,
                          const td_rows_spec* spec, int64_t overlap, const td_window_outputs* dev_out, int64_t rows_capacity,
                          void* d_counts, void* hip_stream) {
    return window_rows_device_any("td_window_rows_device", false, t, d_ids, n_tokens, d_tok_offsets, n_docs, spec, overlap, dev_out,
                                  rows_capacity, d_counts, hip_stream, nullptr);
}

int td_window_rows_labeled_device(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_tok_offsets, int64_t n_docs,
                                  const td_rows_spec* spec, int64_t overlap, const td_window_outputs* dev_out, int64_t rows_capacity,
                                  void* d_counts, void* hip_stream, const td_rows_labels* lab) {
    return window_rows_device_any("td_window_rows_labeled_device", true, t, d_ids, n_tokens, d_tok_offsets, n_docs, spec, overlap, dev_out,
                                  rows_capacity, d_counts, hip_stream, lab);
}

static int window_rows_any(const char* fn, bool labeled, td_tokenizer* t, const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets,
                           int64_t n_docs, const td_rows_spec* spec, int64_t overlap, const td_window_outputs* host_out,
                           int64_t rows_capacity, int64_t* counts, const td_rows_labels* lab) {
    if (!t || !spec || !host_out || n_tokens < 0 || n_docs < 0 || !tok_offsets || !counts) return TD_E_INVALID;
    if (int rc = rows_spec_fail(t, fn, rows_args_error(spec, overlap, n_docs, rows_capacity, host_out), spec)) return rc;
    if (int rc = rows_lab_fail(t, fn, lab, spec, labeled)) return rc;
    return locked(t, [&] {
        int rc2;
        if ((rc2 = rows_check_host_ids(t, ids, n_tokens, tok_offsets, n_docs))) return rc2;
        const int64_t total = tok_offsets[n_docs];
        int64_t plan[4];
        if (td_window_plan(tok_offsets, n_docs, spec, overlap, plan, nullptr) != TD_OK) { t->err = "invalid tok_offsets"; return (int)TD_E_INVALID; }
        if (plan[0] > rows_capacity) return rows_capacity_fail(t, plan[0], counts);
        hipStream_t s;
        LabCall lc;
        if ((rc2 = rows_stage_host_ids(t, ids, tok_offsets, n_docs, s))) return rc2;
        if ((rc2 = rows_stage_host_src(t, lab, total, lc, s))) return rc2;
        return window_to_host(t, t->dec_tokens.p, total, t->d_offsets.p, n_docs, spec, overlap, *host_out, plan[0], counts, lc, s);
    });
}

int td_window_rows(td_tokenizer* t, const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets, int64_t n_docs,
                   const td_rows_spec* spec, int64_t overlap, const td_window_outputs* host_out, int64_t rows_capacity, int64_t* counts) {
    return window_rows_any("td_window_rows", false, t, ids, n_tokens, tok_offsets, n_docs, spec, overlap, host_out, rows_capacity, counts,
                           nullptr);
}

int td_window_rows_labeled(td_tokenizer* t, const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets, int64_t n_docs,
                           const td_rows_spec* spec, int64_t overlap, const td_window_outputs* host_out, int64_t rows_capacity,
                           int64_t* counts, const td_rows_labels* lab) {
    return window_rows_any("td_window_rows_labeled", true, t, ids, n_tokens, tok_offsets, n_docs, spec, overlap, host_out, rows_capacity,
                           counts, lab);
}

int td_encode_batch_window_rows(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode,
                                const td_rows_spec* spec, int64_t overlap, const td_window_outputs* host_out, int64_t rows_capacity,
                                int64_t* counts) {
    if (!t || !spec || !host_out || !doc_offsets || n_docs < 0 || !counts || (mode != TD_MODE_ENCODE && mode != TD_MODE_ORDINARY))
        return TD_E_INVALID;
    if (int rc = rows_spec_fail(t, "td_encode_batch_window_rows", rows_args_error(spec, overlap, n_docs, rows_capacity, host_out), spec)) return rc;
    return locked(t, [&] {
        int rc2;
        int64_t dev_cap;
        hipStream_t s;
        if ((rc2 = rows_encode_locked(t, text, doc_offsets, n_docs, mode, dev_cap, s))) return rc2;
        // the rows are known from the token offsets: they come back (8 bytes a document) and are planned on the host
        std::vector<int64_t> toff((size_t)n_docs + 1);
        if ((rc2 = copy_wait(t, toff.data(), t->d_offsets.p, (size_t)(n_docs + 1) * 8, hipMemcpyDeviceToHost, s))) return rc2;
        int64_t plan[4];
        if (td_window_plan(toff.data(), n_docs, spec, overlap, plan, nullptr) != TD_OK) { t->err = "invalid token offsets"; return (int)TD_E_INVALID; }
        if (plan[0] > rows_capacity) return rows_capacity_fail(t, plan[0], counts);
        return window_to_host(t, t->d_tokens.p, dev_cap, t->d_offsets.p, n_docs, spec, overlap, *host_out, plan[0], counts, LabCall{}, s);
    });
}

}  // extern "C"

// ---- document selection (td_select.hip) ---------------------------------------------------------------------------------------
namespace {

const char* select_spec_error(const td_select_spec* sp, const void* sel, int64_t n_sel, int64_t n_docs) {
    if (!sp) return "null td_select_spec";
    if (sp->min_len < 0) return "min_len must be >= 0";
    if (sp->max_len < -1) return "max_len must be -1 (no limit) or >= min_len";
    if (sp->max_len >= 0 && sp->max_len < sp->min_len) return "max_len must be -1 (no limit) or >= min_len";
    if (sp->flags != 0) return "flags must be 0";
    if (!sel && n_sel != n_docs) return "a null sel is the identity: n_sel must be n_docs";
    return nullptr;
}

// Enqueues the scan and the slot kernel; every pointer is device memory.  d_labels / d_out_labels: both null, or the second stream.
int select_launch_locked(td_tokenizer* t, const void* d_ids, const void* d_labels, int64_t n_tokens, const void* d_toff, int64_t n_docs,
                         const void* d_sel, int64_t n_sel, const td_select_spec* sp, void* d_out, void* d_out_labels, int64_t cap,
                         void* d_out_off, void* d_out_docs, void* d_counts, hipStream_t s) {
    int rc;
    if ((rc = order_before(t, s))) return rc;  // (rows_last stays false: a capacity here counts ids)
    SelectLabArgs a;
    memset(&a, 0, sizeof a);
    a.ids = (const int32_t*)d_ids;
    a.n_tokens = n_tokens;
    a.tok_off = (const int64_t*)d_toff;
    a.n_docs = n_docs;
    a.sel = (const int64_t*)d_sel;
    a.n_sel = n_sel;
    a.min_len = sp->min_len;
    a.max_len = sp->max_len;
    a.out = (int32_t*)d_out;
    a.ids_cap = cap;
    a.out_off = (int64_t*)d_out_off;
    a.out_docs = (int64_t*)d_out_docs;
    a.counts = (long long*)d_counts;
    a.lab.src = (const int32_t*)d_labels;
    a.lab.dst = (int32_t*)d_out_labels;
    if ((rc = ensure(t, t->sel_scan, (size_t)select_scan_words(n_sel) * 8))) return rc;
    if ((rc = ensure(t, t->sel_base, (size_t)std::max<int64_t>(n_sel, 1) * 8))) return rc;
    a.scan = (unsigned long long*)t->sel_scan.p;
    a.src_base = (int64_t*)t->sel_base.p;
    HIP_TRY(t, hipMemsetAsync(a.scan, 0, SEL_SCAN_HEAD * 8, s));
    Ctl* ctl = (Ctl*)t->ctl.p;
    a.err = &ctl->err;
    a.err_pos = &ctl->err_pos;
    HIP_TRY(t, launch_select(a, s));
    return order_after(t, s);
}

// Host entry points: the plan on the host offsets h_toff, counts and the errors before any launch.
int select_plan_host(td_tokenizer* t, const int64_t* h_toff, int64_t n_docs, const int64_t* sel, int64_t n_sel, const td_select_spec* sp,
                     const int32_t* out_ids, int64_t cap, int64_t* counts) {
    if (td_select_plan(h_toff, n_docs, sel, n_sel, sp, counts, nullptr, nullptr) != TD_OK) {
        t->err = "sel[" + std::to_string(counts[0]) + "] is not a document in 0 .. n_docs - 1 with valid offsets";
        return TD_E_INVALID;
    }
    if (counts[1] > cap) {
        t->err = "output capacity too small: " + std::to_string(counts[1]) + " tokens needed";
        return TD_E_CAPACITY;
    }
    if (counts[1] > 0 && !out_ids) { t->err = "null out_ids"; return TD_E_INVALID; }
    return TD_OK;
}

// ... and behind it and the staging: the list up, the selection (counts: the plan's K and T) from ids (and lc's label stream)
// already on the device into the handle's buffers, then to the caller's.
int select_to_host(td_tokenizer* t, const void* d_ids, int64_t n_ids, const void* d_toff, int64_t n_docs, const int64_t* sel, int64_t n_sel,
                   const td_select_spec* sp, int32_t* out_ids, int64_t* out_offsets, int64_t* out_docs, int64_t* counts, const LabCall& lc,
                   hipStream_t s) {
    int rc;
    const int64_t K = counts[0], T = counts[1];
    if (sel) {
        if ((rc = ensure(t, t->sel_in, (size_t)std::max<int64_t>(n_sel, 1) * 8))) return rc;
        if (n_sel > 0) HIP_TRY(t, hipMemcpyAsync(t->sel_in.p, sel, (size_t)n_sel * 8, hipMemcpyHostToDevice, s));
    }
    const RowsOut o[] = {{true, out_ids, &t->rows_out, 4, T, T},
                         {lc.spec != nullptr, lc.dst, &t->rows_lab, 4, T, T},
                         {true, out_offsets, &t->sel_off, 8, n_sel + 1, K + 1},
                         {out_docs != nullptr, out_docs, &t->sel_docs, 8, n_sel, K}};
    if ((rc = rows_out_ensure(t, o, 4))) return rc;
    if ((rc = ensure(t, t->rows_counts, 4 * sizeof(int64_t)))) return rc;
    if ((rc = select_launch_locked(t, d_ids, lc.d_src, n_ids, d_toff, n_docs, sel ? t->sel_in.p : nullptr, n_sel, sp, o[0].p(), o[1].p(), T,
                                   o[2].p(), o[3].p(), t->rows_counts.p, s)))
        return rc;
    if ((rc = device_status_locked(t, s, nullptr))) return rc;
    if ((rc = copy_wait(t, counts, t->rows_counts.p, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, s))) return rc;
    return rows_out_copy(t, o, 4, s);
}

}  // namespace

extern "C" {

int td_select_plan(const int64_t* tok_offsets, int64_t n_docs, const int64_t* sel, int64_t n_sel, const td_select_spec* spec,
                   int64_t* counts, int64_t* out_offsets, int64_t* out_docs) {
    if (!counts) return TD_E_INVALID;
    counts[0] = -1;
    counts[1] = counts[2] = counts[3] = 0;
    if (!tok_offsets || n_docs < 0 || n_sel < 0 || select_spec_error(spec, sel, n_sel, n_docs)) return TD_E_INVALID;
    // the walk, twice: what is kept and every check first, so that an error leaves the outputs alone
    for (int pass = 0; pass < 2; ++pass) {
        int64_t K = 0, T = 0, n_short = 0, n_long = 0;
        for (int64_t i = 0; i < n_sel; ++i) {
            const int64_t d = sel ? sel[i] : i;
            if (d < 0 || d >= n_docs || tok_offsets[d] < 0 || tok_offsets[d + 1] < tok_offsets[d]) {
                counts[0] = i;
                return TD_E_INVALID;
            }
            const int64_t L = tok_offsets[d + 1] - tok_offsets[d];
            if (L < spec->min_len) { ++n_short; continue; }
            if (spec->max_len >= 0 && L > spec->max_len) { ++n_long; continue; }
            if (pass == 1) {
                if (out_offsets) out_offsets[K] = T;
                if (out_docs) out_docs[K] = d;
            }
            ++K;
            T += L;
        }
        if (pass == 1 || (!out_offsets && !out_docs)) {
            if (out_offsets) out_offsets[K] = T;
            counts[0] = K;
            counts[1] = T;
            counts[2] = n_short;
            counts[3] = n_long;
            break;
        }
    }
    return TD_OK;
}

int td_select_docs_device(td_tokenizer* t, const void* d_ids, const void* d_labels, int64_t n_tokens, const void* d_tok_offsets,
                          int64_t n_docs, const void* d_sel, int64_t n_sel, const td_select_spec* spec, void* d_out_ids,
                          void* d_out_labels, int64_t ids_capacity, void* d_out_offsets, void* d_out_docs, void* d_counts,
                          void* hip_stream) {
    if (!t || n_tokens < 0 || n_docs < 0 || n_sel < 0 || !d_tok_offsets || (n_tokens > 0 && !d_ids) || !d_counts || !d_out_offsets ||
        ids_capacity < 0 || (ids_capacity > 0 && !d_out_ids) || (d_labels != nullptr) != (d_out_labels != nullptr))
        return TD_E_INVALID;
    if (const char* m = select_spec_error(spec, d_sel, n_sel, n_docs)) return fail_unlocked(t, TD_E_INVALID, std::string("td_select_docs_device: ") + m);
    return locked(t, [&] {
        return select_launch_locked(t, d_ids, d_labels, n_tokens, d_tok_offsets, n_docs, d_sel, n_sel, spec, d_out_ids, d_out_labels,
                                    ids_capacity, d_out_offsets, d_out_docs, d_counts, (hipStream_t)hip_stream);
    });
}

int td_select_docs(td_tokenizer* t, const int32_t* ids, const int32_t* labels, int64_t n_tokens, const int64_t* tok_offsets,
                   int64_t n_docs, const int64_t* sel, int64_t n_sel, const td_select_spec* spec, int32_t* out_ids,
                   int32_t* out_labels, int64_t ids_capacity, int64_t* out_offsets, int64_t* out_docs, int64_t* counts) {
    if (!t || n_tokens < 0 || n_docs < 0 || n_sel < 0 || !tok_offsets || !counts || !out_offsets || ids_capacity < 0 ||
        (labels != nullptr) != (out_labels != nullptr))
        return TD_E_INVALID;
    if (const char* m = select_spec_error(spec, sel, n_sel, n_docs)) return fail_unlocked(t, TD_E_INVALID, std::string("td_select_docs: ") + m);
    return locked(t, [&] {
        int rc;
        if ((rc = rows_check_host_ids(t, ids, n_tokens, tok_offsets, n_docs))) return rc;
        if ((rc = select_plan_host(t, tok_offsets, n_docs, sel, n_sel, spec, out_ids, ids_capacity, counts))) return rc;
        hipStream_t s;
        LabCall lc;
        const td_rows_labels lab{labels, out_labels, 0, 0, 0, 0};
        if ((rc = rows_stage_host_ids(t, ids, tok_offsets, n_docs, s))) return rc;
        if ((rc = rows_stage_host_src(t, labels ? &lab : nullptr, tok_offsets[n_docs], lc, s))) return rc;
        return select_to_host(t, t->dec_tokens.p, tok_offsets[n_docs], t->d_offsets.p, n_docs, sel, n_sel, spec, out_ids, out_offsets, out_docs,
                              counts, lc, s);
    });
}

int td_encode_batch_select(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode,
                           const int64_t* sel, int64_t n_sel, const td_select_spec* spec, int32_t* out_ids, int64_t ids_capacity,
                           int64_t* out_offsets, int64_t* out_docs, int64_t* counts) {
    if (!t || !doc_offsets || n_docs < 0 || n_sel < 0 || !counts || !out_offsets || ids_capacity < 0 ||
        (mode != TD_MODE_ENCODE && mode != TD_MODE_ORDINARY))
        return TD_E_INVALID;
    if (const char* m = select_spec_error(spec, sel, n_sel, n_docs)) return fail_unlocked(t, TD_E_INVALID, std::string("td_encode_batch_select: ") + m);
    return locked(t, [&] {
        int rc;
        int64_t dev_cap;
        hipStream_t s;
        if ((rc = rows_encode_locked(t, text, doc_offsets, n_docs, mode, dev_cap, s))) return rc;
        // what is kept is known from the token offsets: they come back (8 bytes a document) and are planned on the host
        std::vector<int64_t> toff((size_t)n_docs + 1);
        if ((rc = copy_wait(t, toff.data(), t->d_offsets.p, (size_t)(n_docs + 1) * 8, hipMemcpyDeviceToHost, s))) return rc;
        if ((rc = select_plan_host(t, toff.data(), n_docs, sel, n_sel, spec, out_ids, ids_capacity, counts))) return rc;
        return select_to_host(t, t->d_tokens.p, dev_cap, t->d_offsets.p, n_docs, sel, n_sel, spec, out_ids, out_offsets, out_docs, counts,
                              LabCall{}, s);
    });
}

}  // extern "C"
