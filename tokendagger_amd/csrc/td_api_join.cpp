// Field joins (td_join.hip): the spec's checks, td_join_plan (host only), and the device, host and fused entry points.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "td_handle.h"
#include "td_join.h"

namespace {

bool fits_i32(int64_t v) { return v >= INT32_MIN && v <= INT32_MAX; }

const char* join_spec_error(const td_join_spec* sp, int64_t n_docs) {
    if (!sp) return "null td_join_spec";
    if (sp->n_fields < 1 || sp->n_fields > TD_JOIN_MAX_FIELDS) return "n_fields must be 1 .. TD_JOIN_MAX_FIELDS";
    if (sp->n_tail < 0 || sp->n_tail > TD_JOIN_MAX_LITERAL) return "n_tail must be 0 .. TD_JOIN_MAX_LITERAL";
    if (sp->max_total < -1) return "max_total must be -1 (no limit) or >= 0";
    if (sp->shrink != TD_JOIN_SHRINK_ORDER && sp->shrink != TD_JOIN_SHRINK_LONGEST) return "unknown shrink";
    if (sp->flags & ~(int64_t)(TD_JOIN_FIELD_MAJOR | TD_JOIN_TRAIN_TAIL)) return "unknown flags";
    if (!fits_i32(sp->ignore_index)) return "ignore_index must fit int32";
    if (!fits_i32(sp->tail_type)) return "tail_type must fit int32";
    for (int64_t f = 0; f < sp->n_fields; ++f) {
        const td_join_field& fd = sp->fields[f];
        if (fd.n_before < 0 || fd.n_before > TD_JOIN_MAX_LITERAL) return "n_before must be 0 .. TD_JOIN_MAX_LITERAL";
        if (fd.max_len < -1) return "max_len must be -1 (no cap) or >= 0";
        if (fd.shrink_rank < 0) return "shrink_rank must be >= 0";
        if (fd.flags & ~(int64_t)(TD_JOIN_KEEP_TAIL | TD_JOIN_TRAIN | TD_JOIN_TRAIN_BEFORE)) return "unknown field flags";
        if (!fits_i32(fd.type_value)) return "type_value must fit int32";
    }
    if (n_docs % sp->n_fields != 0) return "n_docs must be a multiple of n_fields";
    return nullptr;
}

// The rule's form of a checked spec.
JoinRule join_rule_of(const td_join_spec* sp) {
    JoinRule r;
    memset(&r, 0, sizeof r);
    r.K = (int32_t)sp->n_fields;
    r.longest = sp->shrink == TD_JOIN_SHRINK_LONGEST;
    r.field_major = (sp->flags & TD_JOIN_FIELD_MAJOR) != 0;
    r.n_tail = (int32_t)sp->n_tail;
    r.max_total = sp->max_total;
    r.fixed = sp->n_tail;
    int order[TD_JOIN_MAX_FIELDS], n = 0;
    for (int f = 0; f < r.K; ++f) {
        const td_join_field& fd = sp->fields[f];
        r.max_len[f] = fd.max_len;
        r.n_before[f] = (int32_t)fd.n_before;
        r.fixed += fd.n_before;
        r.order_pos[f] = -1;
        if (fd.flags & TD_JOIN_KEEP_TAIL) r.keep_tail |= 1u << f;
        if (fd.shrink_rank > 0) order[n++] = f;
    }
    std::stable_sort(order, order + n, [sp](int x, int y) { return sp->fields[x].shrink_rank < sp->fields[y].shrink_rank; });
    for (int i = 0; i < n; ++i) r.order_pos[order[i]] = i;
    return r;
}

// Every literal: an id of the vocabulary, ordinary or special (the rule of bos_id / eos_id).
int join_check_literals(td_tokenizer* t, const char* fn, const td_join_spec* sp) {
    auto one = [&](int64_t id) {
        if (id >= 0 && id <= INT32_MAX && td_token_bytes(t, (int32_t)id, nullptr, nullptr) == TD_OK) return (int)TD_OK;
        return fail_unlocked(t, TD_E_BAD_TOKEN, std::string(fn) + ": literal id " + std::to_string(id) + " is not in the vocabulary");
    };
    int rc;
    for (int64_t f = 0; f < sp->n_fields; ++f)
        for (int64_t i = 0; i < sp->fields[f].n_before; ++i)
            if ((rc = one(sp->fields[f].before[i]))) return rc;
    for (int64_t i = 0; i < sp->n_tail; ++i)
        if ((rc = one(sp->tail[i]))) return rc;
    return TD_OK;
}

bool ranges_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
    if (!a || !b || na <= 0 || nb <= 0) return false;
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)nb * 4 && b0 < a0 + (uintptr_t)na * 4;
}

// The checks of every handle entry point between its null tests and the lock.
int join_args_check(td_tokenizer* t, const char* fn, const td_join_spec* sp, int64_t n_docs, const void* ids, int64_t n_tokens,
                    const td_join_outputs* o) {
    if (const char* m = join_spec_error(sp, n_docs)) return fail_unlocked(t, TD_E_INVALID, std::string(fn) + ": " + m);
    if (ranges_overlap(ids, n_tokens, o->ids, o->ids_capacity))
        return fail_unlocked(t, TD_E_INVALID, std::string(fn) + ": the output ids overlap the input ids (joining in place is not supported)");
    return join_check_literals(t, fn, sp);
}

// Enqueues the scan and the slot kernel; every pointer is device memory.
int join_launch_locked(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_toff, int64_t n_docs, const td_join_spec* sp,
                       const td_join_outputs& o, void* d_counts, hipStream_t s) {
    int rc;
    if ((rc = order_before(t, s))) return rc;  // (rows_last stays false: a capacity here counts ids)
    JoinArgs a;
    memset(&a, 0, sizeof a);
    a.rule = join_rule_of(sp);
    const int K = a.rule.K;
    a.ids = (const int32_t*)d_ids;
    a.n_tokens = n_tokens;
    a.tok_off = (const int64_t*)d_toff;
    a.n_ex = n_docs / K;
    for (int f = 0; f < K; ++f) {
        const td_join_field& fd = sp->fields[f];
        for (int i = 0; i < fd.n_before; ++i) a.lit[f][i] = (int32_t)fd.before[i];
        a.type_of[f] = (int32_t)fd.type_value;
        if (fd.flags & TD_JOIN_TRAIN_BEFORE) a.train |= 1u << (2 * f);
        if (fd.flags & TD_JOIN_TRAIN) a.train |= 1u << (2 * f + 1);
    }
    for (int i = 0; i < sp->n_tail; ++i) a.lit[K][i] = (int32_t)sp->tail[i];
    a.type_of[K] = (int32_t)sp->tail_type;
    if (sp->flags & TD_JOIN_TRAIN_TAIL) a.train |= 1u << (2 * K);
    a.ignore_index = (int32_t)sp->ignore_index;
    a.out = (int32_t*)o.ids;
    a.out_labels = (int32_t*)o.labels;
    a.out_types = (int32_t*)o.types;
    a.ids_cap = o.ids_capacity;
    a.out_off = (int64_t*)o.offsets;
    a.out_examples = (int64_t*)o.examples;
    a.out_field_len = (int32_t*)o.field_len;
    a.counts = (long long*)d_counts;
    if ((rc = ensure(t, t->join_scan, (size_t)join_scan_words(a.n_ex) * 8))) return rc;
    if ((rc = ensure(t, t->join_plan, (size_t)std::max<int64_t>(a.n_ex, 1) * join_plan_words(K) * 8))) return rc;
    a.scan = (unsigned long long*)t->join_scan.p;
    a.plan = (int64_t*)t->join_plan.p;
    HIP_TRY(t, hipMemsetAsync(a.scan, 0, JOIN_SCAN_HEAD * 8, s));
    Ctl* ctl = (Ctl*)t->ctl.p;
    a.err = &ctl->err;
    a.err_pos = &ctl->err_pos;
    HIP_TRY(t, launch_join(a, s));
    return order_after(t, s);
}

// Host entry points: the plan on the host offsets h_toff, counts and the errors before any launch.
int join_plan_host(td_tokenizer* t, const int64_t* h_toff, int64_t n_docs, const td_join_spec* sp, const td_join_outputs* o, int64_t* counts) {
    if (td_join_plan(h_toff, n_docs, sp, counts, nullptr, nullptr, nullptr) != TD_OK) {
        t->err = "example " + std::to_string(counts[0]) + " has a document without valid offsets";
        return TD_E_INVALID;
    }
    if (counts[1] > o->ids_capacity) {
        t->err = "output capacity too small: " + std::to_string(counts[1]) + " tokens needed";
        return TD_E_CAPACITY;
    }
    if (counts[1] > 0 && !o->ids) { t->err = "null output ids"; return TD_E_INVALID; }
    return TD_OK;
}

struct JoinOut {  // an output of a host entry point: the caller's buffer, the handle's on the device, what comes back
    void* host;
    DevBuf* dev;
    size_t elem;
    int64_t n_alloc, n_copy;
    void* p() const { return host ? dev->p : nullptr; }
};

// ... and behind it and the staging: the join (counts: the plan's E and T) from ids already on the device into the handle's
// buffers, then to the caller's.
int join_to_host(td_tokenizer* t, const void* d_ids, int64_t n_ids, const void* d_toff, int64_t n_docs, const td_join_spec* sp,
                 const td_join_outputs* o, int64_t* counts, hipStream_t s) {
    int rc;
    const int64_t E = counts[0], T = counts[1], K = sp->n_fields, n_ex = n_docs / K;
    JoinOut out[] = {{o->ids, &t->rows_out, 4, T, T},  // (NULL only with T = 0: join_plan_host)
                     {o->labels, &t->rows_lab, 4, T, T},
                     {o->types, &t->join_types, 4, T, T},
                     {o->offsets, &t->join_off, 8, n_ex + 1, E + 1},
                     {o->examples, &t->join_ex, 8, n_ex, E},
                     {o->field_len, &t->join_flen, 4, n_ex * K, E * K}};
    for (const JoinOut& b : out)
        if (b.host && (rc = ensure(t, *b.dev, (size_t)std::max<int64_t>(b.n_alloc, 1) * b.elem))) return rc;
    if ((rc = ensure(t, t->rows_counts, 4 * sizeof(int64_t)))) return rc;
    const td_join_outputs d{out[0].p(), out[1].p(), out[2].p(), T, out[3].p(), out[4].p(), out[5].p()};
    if ((rc = join_launch_locked(t, d_ids, n_ids, d_toff, n_docs, sp, d, t->rows_counts.p, s))) return rc;
    if ((rc = device_status_locked(t, s, nullptr))) return rc;
    if ((rc = copy_wait(t, counts, t->rows_counts.p, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, s))) return rc;
    for (const JoinOut& b : out)
        if (b.host && b.n_copy > 0 && (rc = copy_wait(t, b.host, b.dev->p, (size_t)b.n_copy * b.elem, hipMemcpyDeviceToHost, s))) return rc;
    return TD_OK;
}

}  // namespace

extern "C" {

int td_join_plan(const int64_t* tok_offsets, int64_t n_docs, const td_join_spec* spec, int64_t* counts, int64_t* out_offsets,
                 int64_t* out_examples, int32_t* out_field_len) {
    if (!counts) return TD_E_INVALID;
    counts[0] = -1;
    counts[1] = counts[2] = counts[3] = 0;
    if (!tok_offsets || n_docs < 0 || join_spec_error(spec, n_docs)) return TD_E_INVALID;
    const JoinRule r = join_rule_of(spec);
    const int64_t n_ex = n_docs / r.K;
    const bool outputs = out_offsets || out_examples || out_field_len;
    // the walk, twice: what is kept and every check first, so that an error leaves the outputs alone
    for (int pass = 0; pass < 2; ++pass) {
        int64_t E = 0, T = 0, n_drop = 0, n_trunc = 0;
        for (int64_t x = 0; x < n_ex; ++x) {
            int64_t L[JOIN_MAX_FIELDS] = {}, c[JOIN_MAX_FIELDS] = {};
            for (int f = 0; f < r.K; ++f) {
                const int64_t d = join_doc(r, n_ex, x, f);
                const int64_t lo = tok_offsets[d], hi = tok_offsets[d + 1];
                if (lo < 0 || hi < lo || hi > (int64_t(1) << 59)) {
                    counts[0] = x;
                    return TD_E_INVALID;
                }
                L[f] = hi - lo;
            }
            const int st = join_keep(r, L, c);
            if (st == JOIN_DROPPED) { ++n_drop; continue; }
            n_trunc += st == JOIN_TRUNCATED;
            if (pass == 1) {
                if (out_offsets) out_offsets[E] = T;
                if (out_examples) out_examples[E] = x;
                if (out_field_len)
                    for (int f = 0; f < r.K; ++f) out_field_len[E * r.K + f] = c[f] > INT32_MAX ? INT32_MAX : (int32_t)c[f];
            }
            ++E;
            T += r.fixed;
            for (int f = 0; f < r.K; ++f) T += c[f];
        }
        if (pass == 1 || !outputs) {
            if (out_offsets) out_offsets[E] = T;
            counts[0] = E;
            counts[1] = T;
            counts[2] = n_drop;
            counts[3] = n_trunc;
            break;
        }
    }
    return TD_OK;
}

int td_join_fields_device(td_tokenizer* t, const void* d_ids, int64_t n_tokens, const void* d_tok_offsets, int64_t n_docs,
                          const td_join_spec* spec, const td_join_outputs* d_out, void* d_counts, void* hip_stream) {
    if (!t || n_tokens < 0 || n_docs < 0 || !d_tok_offsets || (n_tokens > 0 && !d_ids) || !d_counts || !d_out || !d_out->offsets ||
        d_out->ids_capacity < 0 || (d_out->ids_capacity > 0 && !d_out->ids))
        return TD_E_INVALID;
    int rc;
    if ((rc = join_args_check(t, "td_join_fields_device", spec, n_docs, d_ids, n_tokens, d_out))) return rc;
    return locked(t, [&] { return join_launch_locked(t, d_ids, n_tokens, d_tok_offsets, n_docs, spec, *d_out, d_counts, (hipStream_t)hip_stream); });
}

int td_join_fields(td_tokenizer* t, const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets, int64_t n_docs,
                   const td_join_spec* spec, const td_join_outputs* out, int64_t* counts) {
    if (!t || n_tokens < 0 || n_docs < 0 || !tok_offsets || !counts || !out || !out->offsets || out->ids_capacity < 0) return TD_E_INVALID;
    int rc;
    if ((rc = join_args_check(t, "td_join_fields", spec, n_docs, ids, n_tokens, out))) return rc;
    return locked(t, [&] {
        int rc;
        if ((rc = rows_check_host_ids(t, ids, n_tokens, tok_offsets, n_docs))) return rc;
        if ((rc = join_plan_host(t, tok_offsets, n_docs, spec, out, counts))) return rc;
        hipStream_t s;
        if ((rc = rows_stage_host_ids(t, ids, tok_offsets, n_docs, s))) return rc;
        return join_to_host(t, t->dec_tokens.p, tok_offsets[n_docs], t->d_offsets.p, n_docs, spec, out, counts, s);
    });
}

int td_encode_batch_join(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode,
                         const td_join_spec* spec, const td_join_outputs* out, int64_t* counts) {
    if (!t || !doc_offsets || n_docs < 0 || !counts || !out || !out->offsets || out->ids_capacity < 0 ||
        (mode != TD_MODE_ENCODE && mode != TD_MODE_ORDINARY))
        return TD_E_INVALID;
    int rc;
    if ((rc = join_args_check(t, "td_encode_batch_join", spec, n_docs, nullptr, 0, out))) return rc;
    return locked(t, [&] {
        int rc;
        int64_t dev_cap;
        hipStream_t s;
        if ((rc = rows_encode_locked(t, text, doc_offsets, n_docs, mode, dev_cap, s))) return rc;
        // what is kept is known from the token offsets: they come back (8 bytes a document) and are planned on the host
        std::vector<int64_t> toff((size_t)n_docs + 1);
        if ((rc = copy_wait(t, toff.data(), t->d_offsets.p, (size_t)(n_docs + 1) * 8, hipMemcpyDeviceToHost, s))) return rc;
        if ((rc = join_plan_host(t, toff.data(), n_docs, spec, out, counts))) return rc;
        return join_to_host(t, t->d_tokens.p, dev_cap, t->d_offsets.p, n_docs, spec, out, counts, s);
    });
}

}  // extern "C"
