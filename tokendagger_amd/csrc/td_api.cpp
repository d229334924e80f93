// C-ABI host library (include/tokendagger_hip.h) over the gfx950 kernels.
// Host code is C++; it owns the device tables, the per-call workspace and stream-ordered launches.
// There is deliberately NO CPU tokenization path in this file: if HIP is unusable, td_create fails.
#include "td_counts_args.h"
#include "td_handle.h"
#include "td_regex.h"

static thread_local std::string g_create_err;  // td_last_error(nullptr): why this thread's last td_create / td_clone failed
// td_last_error(t) must not hand out a pointer into t->err, which another thread's call may be rewriting: every failing
// call copies its message (under the handle's lock) into this thread's slot (fail_unlocked), and td_last_error reads the slot.
static thread_local std::string g_thread_err;
static thread_local const td_tokenizer* g_thread_err_owner = nullptr;

namespace td {  // ---- the helpers td_handle.h declares ----------------------------------------------------------------------------

hipError_t make_stream(Stream& s) {
    hipStream_t h = nullptr;
    const hipError_t e = hipStreamCreateWithFlags(&h, hipStreamNonBlocking);
    if (e == hipSuccess) s = Stream(h);
    return e;
}
hipError_t make_event(Event& ev) {
    hipEvent_t h = nullptr;
    const hipError_t e = hipEventCreateWithFlags(&h, hipEventDisableTiming);
    if (e == hipSuccess) ev = Event(h);
    return e;
}
hipError_t make_pinned(PinnedBuf& b, size_t bytes) {
    void* p = nullptr;
    const hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
    if (e == hipSuccess) { PinnedBuf n; n.p = p; n.cap = bytes; b = std::move(n); }
    return e;
}

Options Options::from_env() {
    Options o;
    if (const char* e = getenv("TD_FUSED")) o.fused = atoi(e) != 0;
    if (const char* e = getenv("TD_GRAPH")) o.graphs = atoi(e) != 0;
    if (const char* e = getenv("TD_DIRECT")) o.direct = atoi(e) != 0;
    if (const char* e = getenv("TD_PACK_SPLIT")) o.pack_split = atoi(e) != 0;
    if (const char* e = getenv("TD_DEDUPE")) o.dedupe = atoi(e) != 0;
    if (const char* e = getenv("TD_OVERLAP")) o.overlap = atoi(e) != 0;
    if (const char* e = getenv("TD_MID_PATH")) o.mid_enabled = atoi(e) != 0;
    if (const char* e = getenv("TD_SMALL_RESIDENT")) o.small_resident = atoi(e) != 0;
    if (const char* e = getenv("TD_SMALL_IDLE_US")) { const long v = atol(e); if (v >= 1 && v <= 1000000) o.small_idle_ticks = (unsigned long long)v * 100ull; }
    if (const char* e = getenv("TD_SPARSE")) { const int v = atoi(e); if (v >= -1 && v <= 1) o.sparse_opt = v; }
    if (const char* e = getenv("TD_GP_COOP_MIN")) { if (atol(e) >= 1024) o.gp_coop_min = (uint32_t)std::min<long>(atol(e), 0x7FFFFFFF); }
    if (const char* e = getenv("TD_DD_REPLICAS")) { const int v = atoi(e); if (v >= 1 && v <= 16 && !(v & (v - 1))) o.dd_replicas = (uint32_t)v; }
    if (const char* e = getenv("TD_DD_MINLEN")) o.dd_minlen = (uint32_t)std::max(2, atoi(e));
    if (const char* e = getenv("TD_DD_ENTRIES")) { const long v = atol(e); if (v >= 2 && v <= (1l << 24) && !(v & (v - 1))) o.dd_entries_opt = (uint32_t)v; }
    if (const char* e = getenv("TD_COLL_SHRINK")) o.coll_shrink = std::max(1, atoi(e));
    if (const char* e = getenv("TD_WS_FILL")) { const int v = atoi(e); if (v >= 0 && v <= 255) o.ws_fill = v; }
    return o;
}

int ensure(td_tokenizer* t, DevBuf& b, size_t bytes) {
    if (b.cap >= bytes && b.p) return TD_OK;
    if (b.p) {  // kernels of an earlier call may still read it: park it until the next synchronisation point
        t->ws_bytes -= b.cap;
        t->graveyard.push_back(std::move(b));
    }
    size_t want = bytes + bytes / 8 + 256;
    HIP_TRY(t, hipMalloc(&b.p, want));
    b.cap = want;
    t->ws_bytes += want;
    if (t->opt.ws_fill >= 0) {  // (debugging, TD_OPT_WS_FILL: what nobody has written yet reads as this byte, not as what the allocator left)
        int rc = own_streams(t);
        if (rc) return rc;
        HIP_TRY(t, hipMemsetAsync(b.p, t->opt.ws_fill, want, t->s_own));
        HIP_TRY(t, hipStreamSynchronize(t->s_own));
        t->ws_filled += (int64_t)want;
    }
    return TD_OK;
}

// TD_OPT_WS_FILL in front of a step: every buffer of the step workspace over its whole capacity, on the call's stream, but for the
// control block's own bytes (the sticky error, the counters the host reads after a call); td_giant_pieces' scratch behind them is filled.
static int fill_step_ws(td_tokenizer* t, hipStream_t stream) {
    DevBuf* const ws[] = {&t->dd_table, &t->rest_mask, &t->coll_ctr, &t->tile_state, &t->slab, &t->docbits, &t->startbits, &t->slow_list,
                          &t->tile_flag, &t->tile_carry, &t->stage, &t->stage2, &t->tile_count, &t->tile_extra, &t->miss_list,
                          &t->flagged_list, &t->deferred_list, &t->gap_list, &t->gapbits, &t->gx_exit, &t->gx_state, &t->tile_base,
                          &t->doc_slot, &t->long_list, &t->pool, &t->ctl, &t->tile_first_doc, &t->chunk_pref};
    static_assert(sizeof ws / sizeof ws[0] == 28, "the step workspace (td_handle.h)");
    for (DevBuf* b : ws) {
        if (!b->p) continue;
        const size_t skip = b == &t->ctl ? std::min(CTL_BYTES, b->cap) : 0;
        if (b->cap == skip) continue;
        HIP_TRY(t, hipMemsetAsync((char*)b->p + skip, t->opt.ws_fill, b->cap - skip, stream));
        t->ws_filled += (int64_t)(b->cap - skip);
    }
    return TD_OK;
}

int own_streams(td_tokenizer* t) {
    if (!t->s_own) HIP_TRY(t, make_stream(t->s_own));
    if (!t->h_ctl.p) HIP_TRY(t, make_pinned(t->h_ctl, 256));
    return TD_OK;
}
// A copy (or fill) the host waits for: on the call's stream, then that stream is synchronised.  Never the legacy stream.
int copy_wait(td_tokenizer* t, void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
    if (bytes == 0) return TD_OK;
    HIP_TRY(t, hipMemcpyAsync(dst, src, bytes, kind, s));
    HIP_TRY(t, hipStreamSynchronize(s));
    return TD_OK;
}
int zero_wait(td_tokenizer* t, void* dst, size_t bytes, hipStream_t s) {
    HIP_TRY(t, hipMemsetAsync(dst, 0, bytes, s));
    HIP_TRY(t, hipStreamSynchronize(s));
    return TD_OK;
}
// Everything this handle has in flight is done when this returns (its own streams + the last call's event: the caller's
// stream itself may be gone by now, the event is ours).
void drain(td_tokenizer* t) {
    if (t->has_last && t->last_done) (void)hipEventSynchronize(t->last_done);
    for (hipStream_t st : {t->s_own.h, t->s_h2d.h, t->s_k.h, t->s_d2h.h, t->s_aux.h}) if (st) (void)hipStreamSynchronize(st);
}

int fail_unlocked(td_tokenizer* t, int rc, const std::string& msg) {
    g_thread_err = msg;
    g_thread_err_owner = t;
    return rc;
}

// Stream order across calls: the per-handle workspace and control block are reused by every call, so a call on a
// stream other than the previous call's waits for that call's last kernel (device-side wait, no host stall).
int order_before(td_tokenizer* t, hipStream_t stream) {
    t->rows_last = false;
    if (t->has_last && stream != t->last_stream) HIP_TRY(t, hipStreamWaitEvent(stream, t->last_done, 0));
    return TD_OK;
}
int order_after(td_tokenizer* t, hipStream_t stream) {
    if (!t->last_done) HIP_TRY(t, make_event(t->last_done));
    HIP_TRY(t, hipEventRecord(t->last_done, stream));
    t->last_stream = stream;
    t->has_last = true;
    return TD_OK;
}

int check_offsets(td_tokenizer* t, const char* what, const int64_t* offs, int64_t n_docs, const void* payload) {
    if (offs[0] != 0) { t->err = std::string(what) + " must start at 0"; return TD_E_INVALID; }
    for (int64_t d = 0; d < n_docs; ++d)
        if (offs[d + 1] < offs[d]) { t->err = std::string(what) + " must be non-decreasing"; return TD_E_INVALID; }
    if (offs[n_docs] > 0 && !payload) { t->err = "null buffer with non-empty documents"; return TD_E_INVALID; }
    return TD_OK;
}

int pinned_ensure(td_tokenizer* t, PinnedBuf& b, size_t bytes) {
    if (b.cap >= bytes && b.p) return TD_OK;
    b = PinnedBuf();  // (the old one first)
    HIP_TRY(t, make_pinned(b, bytes + bytes / 8 + 4096));
    return TD_OK;
}

int wait_for_seq(td_tokenizer* t, const volatile unsigned long long* seqp, unsigned long long seq, hipStream_t s, uint32_t spin_mask,
                 int limit_s, const char* what) {
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spins = 0;; ++spins) {
        if (__atomic_load_n(seqp, __ATOMIC_ACQUIRE) == seq) return TD_OK;
        if ((spins & spin_mask) == spin_mask && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(limit_s)) {
            HIP_TRY(t, hipStreamSynchronize(s));  // (a launch failure surfaces here)
            if (__atomic_load_n(seqp, __ATOMIC_ACQUIRE) == seq) return TD_OK;
            t->err = what;
            return TD_E_HIP;
        }
    }
}

}  // namespace td

namespace {  // ---- the workspace of a step ----------------------------------------------------------------------------------------

void drop_graph(td_tokenizer* t) { t->graph_exec = GraphExec(); }

template <class V>
int upload(td_tokenizer* t, const V* src, size_t count, const V** dst) {
    void* p = nullptr;
    const size_t bytes = std::max<size_t>(count * sizeof(V), 16);
    HIP_TRY(t, hipMalloc(&p, bytes + 16));
    t->table_allocs.push_back(p);
    int rc = copy_wait(t, p, src, count * sizeof(V), hipMemcpyHostToDevice, t->s_own);
    if (rc) return rc;
    *dst = (const V*)p;
    return TD_OK;
}

// The miss lists in one buffer: the tile loops' five (room for K_MISS_LISTED_MAX per tile each), then td_collect_misses'
// K_MISS_CLASSES x COLL_SUBS.  A class gets room for the most records n bytes can hold up to 64 Ki, beyond that for a fixed share
// of n: a miss of <= 8 bytes every 24 bytes of text, 9..16 every 48, 17..32 every 96, 33..48 every 128, longer ones every 160 (0.7 bytes
// of list per byte of text — round 4 had 2.1; mixed-script text has a miss every 51 bytes over all classes, the reference's code
// file set one of <= 8 bytes every 33, and since round 5 only the DISTINCT pieces of a call are listed).  What finds no room is merged by the slow scan
// at the end of td_merge_pieces.  dense (encode_ordinary with a vocabulary whose tokens the merge loop does not all reproduce: no
// whole-piece lookup, EVERY piece of two bytes or more is merged): the worst case, 5.8 bytes per byte of text.  TD_COLL_SHRINK=<k>
// (tests): 1/k of that.
struct CollLayout {
    unsigned long long base[K_MISS_CLASSES];
    uint32_t cap[K_MISS_CLASSES];
    unsigned long long dup_base;  // the lists of repeats behind them: COLL_SUBS x dup_cap entries
    uint32_t dup_cap;
    unsigned long long total;
};
static CollLayout coll_layout(const td_tokenizer* t, int64_t n, int64_t n_tiles, bool dense) {
    static const int minlen[K_MISS_CLASSES] = {2, 9, 17, 33, 49}, share[K_MISS_CLASSES] = {24, 48, 96, 128, 160};
    CollLayout L;
    unsigned long long at = (unsigned long long)(n_tiles + 1) * K_MISS_LISTED_MAX * K_MISS_CLASSES;
    for (int c = 0; c < K_MISS_CLASSES; ++c) {
        const int64_t worst = n / minlen[c] + 1;
        int64_t cls = dense ? worst : std::min<int64_t>(worst, std::max<int64_t>(n / share[c] + 1, 65536));
        if (t->opt.coll_shrink > 1) cls = cls / t->opt.coll_shrink + 1;
        const int64_t per_list = std::min<int64_t>((cls + COLL_SUBS - 1) / COLL_SUBS + 64, 0x7FFFFFF0ll);
        L.base[c] = at;
        L.cap[c] = (uint32_t)per_list;
        at += (unsigned long long)per_list * COLL_SUBS;
    }
    // the repeats (round 5; 8 bytes each): room for as many as the lists of the classes hold records — a missed piece is on one or the other
    L.dup_base = at;
    const unsigned long long coll_records = at - (unsigned long long)(n_tiles + 1) * K_MISS_LISTED_MAX * K_MISS_CLASSES;
    L.dup_cap = (uint32_t)std::min<unsigned long long>(coll_records / COLL_SUBS + 64, 0x7FFFFFF0ull);
    at += (unsigned long long)L.dup_cap * COLL_SUBS;
    L.total = at;
    return L;
}

// seats of the table of distinct missed pieces (EncodeArgs::dd_table): a power of two, about one per 128 bytes of text
// ... as many as an entry of the list of repeats can name next to its tile (39 bits for both: 2 Mi seats up to 1 GiB of text)
static uint32_t dd_tile_bits(int64_t n) {
    const int64_t n_tiles = (n + K_TILE - 1) / K_TILE;
    uint32_t b = 1;
    while (b < 39 && (1ll << b) < n_tiles) ++b;
    return b;
}
static uint32_t dd_entries(const td_tokenizer* t, int64_t n) {
    const uint32_t most = 1u << std::min<uint32_t>(39 - dd_tile_bits(n), 21);  // (21 bits: what a TOK_DUPREF slot has for the seat)
    if (t->opt.dd_entries_opt) return std::min(t->opt.dd_entries_opt, most);
    uint32_t e = 4096;
    while (e < (2u << 20) && e < most && (int64_t)e * 128 < n) e <<= 1;
    return std::min(e, most);
}

int reserve_ws(td_tokenizer* t, int64_t n, int64_t n_docs, bool dense = false) {
    const int64_t n_tiles = (n + K_TILE - 1) / K_TILE;
    int rc;
    if ((rc = ensure(t, t->docbits, (size_t)((n + 31) / 32 + 2) * 4))) return rc;
    if ((rc = ensure(t, t->startbits, (size_t)((n + 31) / 32 + 8) * 4))) return rc;
    if ((rc = ensure(t, t->slow_list, (size_t)(n_tiles * 8 + 64) * 8))) return rc;
    if ((rc = ensure(t, t->tile_flag, (size_t)(n_tiles + 2) * 4))) return rc;   // (per pre-tokenizer tile: fewer than n_tiles)
    if ((rc = ensure(t, t->tile_carry, (size_t)(n_tiles + 2) * 8))) return rc;
    if ((rc = ensure(t, t->tile_state, (size_t)(n_tiles + 2) * 8))) return rc;   // (per pre-tokenizer tile too)
    if (t->opt.direct && t->H.pattern_kind != PATTERN_GENERIC && (rc = ensure(t, t->slab, (size_t)direct_grid_blocks() * SLAB_RING * SLAB_WORDS * 4))) return rc;
    if ((rc = ensure(t, t->stage, (size_t)std::max<int64_t>(n_tiles, 1) * K_STAGE * 4))) return rc;
    if ((rc = ensure(t, t->stage2, (size_t)std::max<int64_t>(n_tiles, 1) * K_STAGE * 4))) return rc;  // ids of merged pieces
    if ((rc = ensure(t, t->tile_count, (size_t)(n_tiles + 1) * 4))) return rc;
    if ((rc = ensure(t, t->tile_extra, (size_t)(n_tiles + 1) * 4))) return rc;
    if ((rc = ensure(t, t->rest_mask, (size_t)((n_tiles + 15) / 16 + 4) * 2))) return rc;
    if ((rc = ensure(t, t->flagged_list, (size_t)(n_tiles + 64) * 4))) return rc;
    if ((rc = ensure(t, t->deferred_list, (size_t)(n_tiles + 64) * 4))) return rc;
    if (t->H.pattern_kind == PATTERN_GENERIC) {
        if ((rc = ensure(t, t->gap_list, (size_t)(n / gx_chunk_for(n) + 64) * 4))) return rc;   // chunks that failed the check
        if ((rc = ensure(t, t->gapbits, (size_t)((n + 31) / 32 + 8) * 4))) return rc;
        if ((rc = ensure(t, t->gx_exit, (size_t)(n / gx_chunk_for(n) + 2) * 8))) return rc;
        if ((rc = ensure(t, t->gx_state, (size_t)(n / gx_chunk_for(n) + 2) * 4))) return rc;
    }
    {
        CollLayout L = coll_layout(t, n, n_tiles, dense);
        if ((rc = ensure(t, t->miss_list, (size_t)L.total * 8))) return rc;
        if ((rc = ensure(t, t->coll_ctr, (size_t)(K_MISS_CLASSES + 1) * COLL_SUBS * COLL_STRIDE * 4))) return rc;
    }
    if ((rc = ensure(t, t->dd_table, (size_t)dd_entries(t, n) * 8))) return rc;
    if ((rc = ensure(t, t->tile_base, (size_t)(n_tiles + 2) * 8))) return rc;
    if ((rc = ensure(t, t->doc_slot, (size_t)(n_docs + 1) * 4))) return rc;
    if ((rc = ensure(t, t->tile_first_doc, (size_t)(n_tiles + 1) * 4))) return rc;
    if ((rc = ensure(t, t->chunk_pref, (size_t)(n_tiles / 4096 + 2) * 8))) return rc;
    if ((rc = ensure(t, t->long_list, (size_t)(n / (K_MAXSHORT + 1) + n_tiles + 16) * sizeof(LongEntry)))) return rc;
    const int64_t pool_bytes = t->opt.pool_bytes_opt > 0 ? t->opt.pool_bytes_opt : std::max<int64_t>(64ll << 20, 2 * n);
    if ((rc = ensure(t, t->pool, (size_t)pool_bytes))) return rc;
    if ((rc = ensure(t, t->ctl, CTL_BYTES + TD_GP_SCRATCH_BYTES))) return rc;
    return TD_OK;
}

}  // namespace

int td::encode_device_locked(td_tokenizer* t, const void* d_text, int64_t n, const void* d_offs, int64_t n_docs, int mode, void* d_out,
                             int64_t out_cap, void* d_out_offs, hipStream_t stream) {
    if (n < 0 || n_docs < 0 || (n > 0 && (!d_text || !d_offs)) || !d_out_offs || (mode != TD_MODE_ENCODE && mode != TD_MODE_ORDINARY)) {
        t->err = "td_encode_device: bad argument";
        return TD_E_INVALID;
    }
    int rc;
    if ((rc = order_before(t, stream))) return rc;
    if (n == 0) {  // nothing but empty documents
        HIP_TRY(t, hipMemsetAsync(d_out_offs, 0, (size_t)(n_docs + 1) * 8, stream));
        return order_after(t, stream);
    }
    const bool dense = mode != TD_MODE_ENCODE && !t->H.merge_closed;
    if ((rc = reserve_ws(t, n, n_docs, dense))) return rc;
    if (t->opt.ws_fill >= 0 && (rc = fill_step_ws(t, stream))) return rc;  // (in front of the plain launches and of a graph's replay alike)
    const int64_t n_tiles = (n + K_TILE - 1) / K_TILE;
    if (n_tiles > 0x7FFFFFF0ll) { t->err = "input too large"; return TD_E_INVALID; }
    EncodeArgs a;
    memset(&a, 0, sizeof a);
    a.Tp = t->dTp;
    a.text = (const uint8_t*)d_text;
    a.n = n;
    a.doc_offsets = (const int64_t*)d_offs;
    a.n_docs = n_docs;
    a.docbits = (uint32_t*)t->docbits.p;
    a.startbits = (uint32_t*)t->startbits.p;
    a.slow_list = (int64_t*)t->slow_list.p;
    a.tile_flag = (uint32_t*)t->tile_flag.p;
    a.tile_carry = (int64_t*)t->tile_carry.p;
    a.slow_cap = (uint32_t)std::min<size_t>(t->slow_list.cap / 8, 0x7FFFFFF0u);
    a.stage = (uint32_t*)t->stage.p;
    a.merge_out = (uint32_t*)t->stage2.p;
    a.tile_count = (uint32_t*)t->tile_count.p;
    a.tile_extra = (uint32_t*)t->tile_extra.p;
    a.rest_mask = (uint16_t*)t->rest_mask.p;
    a.tile_base = (int64_t*)t->tile_base.p;
    a.doc_slot = (uint32_t*)t->doc_slot.p;
    a.tile_first_doc = (uint32_t*)t->tile_first_doc.p;
    a.long_list = (LongEntry*)t->long_list.p;
    a.long_cap = (uint32_t)std::min<size_t>(t->long_list.cap / sizeof(LongEntry), 0x7FFFFFF0u);
    Ctl* ctl = (Ctl*)t->ctl.p;
    a.long_count = &ctl->long_count;
    a.giant_count = &ctl->giant_count;
    a.gp_ctl = ctl->gp_ctl;
    a.gp_scratch = (uint32_t*)((char*)t->ctl.p + CTL_BYTES);  // (behind the control block; needs no reset: what is read was written in front of the grid barrier the read is behind)
    a.gp_coop_min = t->opt.gp_coop_min;
    a.tile_draw = &ctl->tile_draw;
    a.far_count = &ctl->far_tiles;
    a.ph_bar = &ctl->ph_bar;
    a.gs_done = &ctl->gs_done;
    a.lp_next = &ctl->lp_next;
    int pack_dense_opt = 1;
    {
        static const int far_light = getenv("TD_FAR_LIGHT") ? atoi(getenv("TD_FAR_LIGHT")) : 1;
        a.far_light = far_light;
        static const int pack_dense = getenv("TD_PACK_DENSE") ? atoi(getenv("TD_PACK_DENSE")) : 1;
        pack_dense_opt = pack_dense;
    }
    a.slow_count = &ctl->slow_count;
    a.pool = (uint32_t*)t->pool.p;
    a.pool_cap = t->pool.cap / 4;
    a.pool_used = &ctl->pool_used;
    a.scan_done = &ctl->scan_done;
    a.merge_next = &ctl->merge_next;
    a.miss_list = (unsigned long long*)t->miss_list.p;
    a.miss_count = ctl->miss_count;
    {
        const CollLayout L = coll_layout(t, n, n_tiles, dense);
        for (int c = 0; c < K_MISS_CLASSES; ++c) { a.coll_base[c] = L.base[c]; a.coll_cap[c] = L.cap[c]; }
        a.dup_list = a.miss_list + L.dup_base;
        a.dup_cap = L.dup_cap;
        a.coll_count = (uint32_t*)t->coll_ctr.p;
        a.ovf_count = &ctl->ovf_count;
    }
    a.dedupe = (t->opt.dedupe && n_tiles < (1ll << 24)) ? 1 : 0;  // (a table entry keeps the tile in 24 bits)
    a.dd_seat_bits = std::min<uint32_t>(39 - dd_tile_bits(n), 21);
    a.dd_minlen = t->opt.dd_minlen;
    a.dd_replicas = t->opt.dd_replicas;
    a.dd_stats = ctl->dd_stats;
    a.dd_table = a.dedupe ? (unsigned long long*)t->dd_table.p : nullptr;
    a.dd_mask = a.dedupe ? dd_entries(t, n) - 1u : 0u;
    a.flagged_count = &ctl->flagged_count;
    a.rx = t->d_rx;
    a.rx_stage1 = t->d_rx_s1;
    a.rx_stage2 = t->d_rx_s2;
    a.gap_list = (int64_t*)t->gap_list.p;
    a.gap_cap = (uint32_t)std::min<size_t>(t->gap_list.cap / 4, 0x7FFFFFF0u);
    a.gapbits = (uint32_t*)t->gapbits.p;
    a.gx_chunk = gx_chunk_for(n);
    a.gx_exit = (int64_t*)t->gx_exit.p;
    a.gx_state = (uint32_t*)t->gx_state.p;
    a.gap_count = &ctl->gap_count;
    a.gx_prefix = t->gx_prefix_dev;
    a.flagged_list = (uint32_t*)t->flagged_list.p;
    a.deferred_list = (uint32_t*)t->deferred_list.p;
    a.deferred_count = &ctl->deferred_count;
    a.fused = t->opt.fused ? 1 : 0;
    a.pack_split = t->opt.pack_split ? 1 : 0;
    a.direct = (t->opt.direct && t->opt.fused && !t->sp_active && t->H.pattern_kind != PATTERN_GENERIC && d_out && !t->stop_after) ? 1 : 0;
    a.tile_state = (unsigned long long*)t->tile_state.p;
    a.slab = (uint32_t*)t->slab.p;
    a.direct_tiles = &ctl->direct_tiles;
    a.probe_deferred = 0;
    a.miss_cap = (uint32_t)((n_tiles + 1) * K_MISS_LISTED_MAX);
    a.chunk_pref = (int64_t*)t->chunk_pref.p;
    a.ctl_reset = &ctl->long_count;  // keep a sticky error (err / err_pos) but reset the per-call counters
    a.ctl_reset_words = (uint32_t)((sizeof(Ctl) - offsetof(Ctl, long_count)) / 4);
    a.out_tokens = (int32_t*)d_out;
    a.out_cap = d_out ? out_cap : 0;
    a.out_offsets = (int64_t*)d_out_offs;
    a.err = &ctl->err;
    a.err_pos = &ctl->err_pos;
    a.n_tiles = (int)n_tiles;
    a.n_stiles = (int)((n + KS_TILE - 1) / KS_TILE);
    a.pat_flags = pattern_flags(t->H.pattern_kind);
    // encode_ordinary has no whole-piece fast path (tiktoken.cpp:156-167); when every token is
    // reproduced by the merge loop the fast path cannot change the result and stays on.
    a.use_fastpath = (mode == TD_MODE_ENCODE) || t->H.merge_closed;
    a.text_aligned = (((uintptr_t)d_text) & 15) == 0;
    a.stop_after = t->stop_after;
    if (t->sp_active) {
        a.sp.bytes = (const uint8_t*)t->sp_bytes.p;
        a.sp.off = (const uint32_t*)t->sp_off.p;
        a.sp.len = (const uint32_t*)t->sp_len.p;
        a.sp.id = (const int32_t*)t->sp_id.p;
        a.sp.parent = (const int32_t*)t->sp_parent.p;
        a.sp.first2 = (const uint32_t*)t->sp_first2.p;
        a.sp.hitbits = (uint32_t*)t->sp_hit.p;
        a.sp.cand_pos = (int64_t*)t->sp_cpos.p;
        a.sp.cand_lit = (int32_t*)t->sp_clit.p;
        a.sp.cand_count = (uint32_t*)t->sp_ccount.p;
        // (entries BOTH lists hold: ensure() grows a buffer by an eighth and 256 BYTES, which is 64 entries of cand_lit and 32 of cand_pos)
        a.sp.cand_cap = (uint32_t)std::min<size_t>(std::min(t->sp_clit.cap / 4, t->sp_cpos.cap / 8), 0x7FFFFFF0u);
        a.sp.accbits = (uint32_t*)t->sp_acc.p;
        a.sp.n = t->sp_n;
        a.sp.maxlen = t->sp_maxlen;
    }
    hipEvent_t* prof = nullptr;
    if (t->profile) {
        td_tokenizer::Ev3 ev;  // (a failure frees the events it has made so far)
        if (!t->ev_free.empty()) { ev = std::move(t->ev_free.back()); t->ev_free.pop_back(); }
        else for (auto& e : ev.e) HIP_TRY(t, hipEventCreate(&e));
        t->ev_pending.push_back(std::move(ev));
        prof = t->ev_pending.back().e;
    }
    // A call that repeats the previous one exactly (same buffers, sizes, stream: a loop over a resident batch, one rank's step
    // of a multi-GPU job) can replay the step as ONE hipGraph launch instead of its dozen kernel launches (opt-in: TD_OPT_GRAPH):
    // the second such call captures the launches, the following ones replay them.  The capture runs on a PRIVATE non-blocking
    // stream in thread-local mode — nothing executes during a capture, so it needs no ordering with the caller's stream — and
    // the caller's stream only ever sees hipGraphLaunch: no stream of the application is in capture because of this library,
    // other threads' legacy-stream work (torch's default stream) stays legal, and a failed capture costs nothing but itself:
    // it is ended, the error is cleared and the step is launched kernel by kernel.
    // The launch sequence (launch_encode): SPARSE — six launches, everything between the tile loop and the packing in td_tail +
    // td_giant_scan — when the last call whose counters were read had next to nothing for the kernels that plain text leaves idle (no
    // deferred or far tiles, few flagged tiles, few long pieces); DENSE — those kernels on their own, at their own occupancies —
    // otherwise and for a handle whose counters nobody has read yet.  Either sequence is correct for any text: a wrong guess costs time.
    {
        bool sparse = t->seen_counters && t->last_far == 0 && t->last_deferred == 0 && t->last_giant == 0 &&
                      t->last_flagged * 64 <= n_tiles && t->last_long * 16 <= n_tiles;
        if (t->opt.sparse_opt >= 0) sparse = t->opt.sparse_opt != 0;
        a.sparse = (sparse && a.fused && !a.direct && !t->sp_active && t->H.pattern_kind != PATTERN_GENERIC && !t->stop_after) ? 1 : 0;
        t->last_sparse = a.sparse != 0;
        a.pack_dense = (!a.sparse && a.pack_split && pack_dense_opt) ? 1 : 0;  // (the sparse sequence keeps its six launches: td_pack_rest takes the odd tile with many markers)
    }
    LaunchAux aux_v{nullptr, nullptr, nullptr};
    const LaunchAux* aux = nullptr;
    // ... when the handle has SEEN long pieces: the fork and the join cost a step without any ~13 us (English: -2 % at 256 MiB), a step
    // with a hundred thousand of them gains 4-7 %.  What the last call whose counters were read had (td_device_status, every host-buffer
    // entry point) decides; a handle that never reads them stays in line.
    if (t->opt.overlap && t->last_long >= 2048 && !a.sparse) {
        hipError_t ae = hipSuccess;
        if (!t->s_aux) ae = make_stream(t->s_aux);  // (a stream priority, either way, changes nothing: r6 call 17)
        if (ae == hipSuccess && !t->e_fork) ae = make_event(t->e_fork);
        if (ae == hipSuccess && !t->e_join) ae = make_event(t->e_join);
        if (ae == hipSuccess) { aux_v = LaunchAux{t->s_aux, t->e_fork, t->e_join}; aux = &aux_v; }
        else (void)hipGetLastError();  // (no second stream: everything in line)
    }
    a.overlap = aux ? 1 : 0;
    hipStreamCaptureStatus cap_status = hipStreamCaptureStatusNone;
    if (stream && hipStreamIsCapturing(stream, &cap_status) != hipSuccess) { cap_status = hipStreamCaptureStatusNone; (void)hipGetLastError(); }
    // (a caller that is capturing this stream into a graph of its own gets the plain launches captured there)
    if (t->opt.graphs && !t->profile && !t->stop_after && cap_status == hipStreamCaptureStatusNone) {
        const bool same_as_graph = t->graph_exec && t->graph_stream == stream && memcmp(&a, &t->graph_key, sizeof a) == 0;
        if (same_as_graph) {
            HIP_TRY(t, hipGraphLaunch(t->graph_exec, stream));
            return order_after(t, stream);
        }
        const bool repeats = t->has_last_key && t->last_key_stream == stream && memcmp(&a, &t->last_key, sizeof a) == 0;
        if (repeats) {
            drop_graph(t);
            hipGraph_t g = nullptr;
            hipError_t ce = t->s_cap ? hipSuccess : make_stream(t->s_cap);
            if (ce == hipSuccess) ce = hipStreamBeginCapture(t->s_cap, hipStreamCaptureModeThreadLocal);
            if (ce == hipSuccess) {
                const hipError_t le = launch_encode(a, t->s_cap, nullptr, aux);
                ce = hipStreamEndCapture(t->s_cap, &g);  // (always: also ends a capture that was invalidated)
                if (le != hipSuccess) ce = le;
            }
            hipGraphExec_t ge = nullptr;
            if (ce == hipSuccess && g && hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) == hipSuccess) {
                (void)hipGraphDestroy(g);
                t->graph_exec = GraphExec(ge);
                t->graph_key = a;
                t->graph_stream = stream;
                t->graph_failures = 0;
                HIP_TRY(t, hipGraphLaunch(t->graph_exec, stream));
                return order_after(t, stream);
            }
            if (g) (void)hipGraphDestroy(g);
            (void)hipGetLastError();
            // not this time: plain launches below; two more identical calls try again, three failures in a row give up
            if (++t->graph_failures >= 3) t->opt.graphs = false;
            t->has_last_key = false;
        } else {
            t->last_key = a;
            t->last_key_stream = stream;
            t->has_last_key = true;
        }
    }
    HIP_TRY(t, launch_encode(a, stream, prof, aux));
    return order_after(t, stream);
}

// The text of an error a kernel left in the control block (err, err_pos).  rows_last: the last launch made rows (the unit of a capacity).
static std::string device_error_text(int code, long long pos, bool rows_last) {
    switch (code) {
        case TD_E_UNKNOWN_BYTE:
            return "No value found for piece at byte offset " + std::to_string(pos) + ": byte sequence is not in the vocabulary";
        case TD_E_CAPACITY:
            return "output capacity too small: " + std::to_string(pos) + (rows_last ? " rows needed" : " tokens needed");
        case TD_E_BAD_TOKEN:
            return "Invalid token for decoding at index " + std::to_string(pos);
        case TD_E_SCRATCH:
            return "device scratch exhausted near byte offset " + std::to_string(pos) +
                   " (pieces above 64 bytes: raise TD_OPT_LONG_POOL_BYTES; allowed special tokens: more candidates than one per 32 bytes of the batch)";
    }
    return "device error " + std::to_string(code) + " at byte offset " + std::to_string(pos);
}

// the control block of a finished call, on the host: counters the launch sequence / second stream are chosen by, the device's error (if any)
int td::absorb_ctl(td_tokenizer* t, Ctl c, hipStream_t stream, int64_t* err_pos) {
    int rc0;
    if (c.err == TD_E_BAD_TOKEN) c.err_pos = 0x7FFFFFFFFFFFFFFFll - c.err_pos;  // (td_decode_len keeps the LOWEST invalid index as a maximum)
    t->last_long = c.long_count;
    t->last_far = (int64_t)c.slow_count + c.far_tiles;
    t->last_giant = c.giant_count;
    t->seen_counters = true;
    t->last_deferred = c.deferred_count;
    t->last_flagged = c.flagged_count;
    t->last_direct = c.direct_tiles;
    t->last_timeouts = c.lb_timeouts;
    t->last_repeats = c.dd_stats[0];
    t->last_listed = c.dd_stats[1];
    if (err_pos) *err_pos = c.err_pos;
    if (c.err != 0) {
        if ((rc0 = zero_wait(t, t->ctl.p, sizeof(Ctl), stream))) return rc0;
        t->err = device_error_text(c.err, c.err_pos, t->rows_last);
        return c.err;
    }
    return TD_OK;
}

int td::device_status_locked(td_tokenizer* t, hipStream_t stream, int64_t* err_pos) {
    if (!t->ctl.p) { HIP_TRY(t, hipStreamSynchronize(stream)); return TD_OK; }
    int rc0 = own_streams(t);
    if (rc0) return rc0;
    static_assert(sizeof(Ctl) <= 256, "h_ctl");
    HIP_TRY(t, hipMemcpyAsync(t->h_ctl.p, t->ctl.p, sizeof(Ctl), hipMemcpyDeviceToHost, stream));  // (behind the call's kernels)
    HIP_TRY(t, hipStreamSynchronize(stream));
    if (!t->has_last || t->last_stream == stream) t->graveyard.clear();  // nothing of this handle is in flight any more
    return absorb_ctl(t, *(const Ctl*)t->h_ctl.p, stream, err_pos);
}

namespace {  // ---- the host-buffer paths of td_encode_batch --------------------------------------------------------------------------

// ---- large inputs: chunks of documents through pinned bounce buffers, H2D || kernels || D2H ----------------------------
// A plain hipMemcpy from pageable memory runs at 9-10 GB/s (the runtime stages it through one pinned buffer on one thread)
// and round 1's td_encode_batch did copy in, kernels, copy out one after the other: 29 ms for 256 MiB of which 1.7 ms were
// kernels.  Here several host threads copy a chunk into a pinned buffer while the previous chunk is on the wire, the kernels
// of chunk i run while chunk i + 1 goes down and the ids of chunk i - 1 come up, and the ids are copied out of their pinned
// buffer by the same threads.

// The streams, events and control-block copies of the pipeline: made aside and moved in only when all of them exist, so that
// a failure leaves the handle without a pipeline, never with half of one (and null streams).
int pipe_init(td_tokenizer* t) {
    if (t->s_h2d) return TD_OK;
    Stream h2d, k, d2h;
    td_tokenizer::PipeSlot slots[td_tokenizer::PIPE_SLOTS];
    for (Stream* st : {&h2d, &k, &d2h}) HIP_TRY(t, make_stream(*st));
    for (auto& sl : slots) {
        for (Event* e : {&sl.ev_h2d, &sl.ev_k, &sl.ev_off, &sl.ev_tok}) HIP_TRY(t, make_event(*e));
        HIP_TRY(t, make_pinned(sl.h_ctl, sizeof(Ctl)));
    }
    for (int i = 0; i < td_tokenizer::PIPE_SLOTS; ++i) t->pipe[i] = std::move(slots[i]);  // (the slots have no buffers yet)
    t->s_k = std::move(k);
    t->s_d2h = std::move(d2h);
    t->s_h2d = std::move(h2d);
    return TD_OK;
}

int encode_batch_pipelined(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode,
                           int32_t* out_tokens, int64_t out_capacity, int64_t* out_offsets, int64_t* n_tokens) {
    int rc;
    if ((rc = pipe_init(t))) return rc;
    if (!t->pool_threads || t->pool_threads->size() != std::max(t->opt.pipe_threads - 1, 1)) t->pool_threads.reset(new CopyPool(std::max(t->opt.pipe_threads - 1, 1)));
    if ((rc = order_before(t, t->s_k))) return rc;
    // chunks: whole documents, about pipe_chunk_bytes each (inputs of less than six such chunks: a sixth of the input, down to an
    // eighth of pipe_chunk_bytes — the pipeline needs a few chunks in flight to hide anything)
    const int64_t n_all = doc_offsets[n_docs] - doc_offsets[0];
    const int64_t chunk_bytes = std::min(t->opt.pipe_chunk_bytes, std::max<int64_t>(t->opt.pipe_chunk_bytes / 8, n_all / 6));
    std::vector<int64_t> cd{0};
    for (int64_t d = 0; d < n_docs;) {
        const int64_t lo = doc_offsets[d];
        int64_t e = d + 1;
        // (binary search for the last document that still fits)
        int64_t a = d + 1, b = n_docs;
        while (a < b) { const int64_t mid = (a + b + 1) >> 1; if (doc_offsets[mid] - lo <= chunk_bytes) a = mid; else b = mid - 1; }
        e = std::max(e, a);
        cd.push_back(e);
        d = e;
    }
    const int nchunks = (int)cd.size() - 1;
    t->last_direct = t->last_timeouts = 0;
    struct Pending { int64_t d0, d1, b0, nbytes, ntok; };
    std::vector<Pending> pend((size_t)nchunks);
    int64_t tok_base = 0;
    bool capacity_miss = false;
    int first_err = TD_OK;
    constexpr int NS = td_tokenizer::PIPE_SLOTS;
    const bool timing = getenv("TD_PIPE_TIMING") != nullptr;
    static const bool publish = !(getenv("TD_PIPE_PUBLISH") && atoi(getenv("TD_PIPE_PUBLISH")) == 0);
    // A chunk's ids leave the device by a KERNEL that stores them into the pinned buffer (32 workgroups; TD_PIPE_D2H_KERNEL=0: by
    // hipMemcpyAsync).  As SDMA copies on their own stream they did not run beside the H2D copies of the next chunks on this box — a
    // GiB of English took the SUM of the two directions, 37 ms, whatever the chunk size, the copy threads, a second pair of streams,
    // HSA_ENABLE_SDMA_GANG=0 or the small dependent copies (profiles/r5_bench/e2e_sweep.txt) — although two streams of queued copies
    // alone do overlap (tools/gpu_pcie_duplex.py: 20 ms).  Stores over PCIe from a kernel do: 27 ms.
    static const int d2h_blocks = getenv("TD_PIPE_D2H_KERNEL") ? atoi(getenv("TD_PIPE_D2H_KERNEL")) : 32;
    double tm[6] = {0, 0, 0, 0, 0, 0};  // wait for the text copy | enqueue | wait for a chunk's kernels | wait for an out-copy | wait for its ids | start copies
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto lap = [&](int k, std::chrono::steady_clock::time_point t0) { if (timing) tm[k] += std::chrono::duration<double, std::milli>(now() - t0).count(); };
    std::shared_ptr<CopyPool::Job> in_job[NS], out_job[NS];
    // chunk i's text starts its way into the slot's pinned buffer (the pool copies; nobody waits here).  The slot was chunk
    // i - NS's, whose H2D copy was over before its kernels were, and those were waited for in fetch(i - NS)
    auto start_in = [&](int i) -> int {
        td_tokenizer::PipeSlot& sl = t->pipe[i % NS];
        const int64_t d0 = cd[(size_t)i], d1 = cd[(size_t)i + 1], b0 = doc_offsets[d0], nb = doc_offsets[d1] - b0;
        const auto t0 = now();
        int r;
        if ((r = pinned_ensure(t, sl.h_text, (size_t)nb + 64))) return r;
        in_job[i % NS] = t->pool_threads->copy(sl.h_text.p, text + b0, (size_t)nb);
        lap(5, t0);
        return TD_OK;
    };
    auto submit = [&](int i) -> int {
        td_tokenizer::PipeSlot& sl = t->pipe[i % NS];
        const int64_t d0 = cd[(size_t)i], d1 = cd[(size_t)i + 1], b0 = doc_offsets[d0], nb = doc_offsets[d1] - b0, nd = d1 - d0;
        pend[(size_t)i] = {d0, d1, b0, nb, 0};
        int r;
        auto t0 = now();
        if ((r = pinned_ensure(t, sl.h_offs, (size_t)(nd + 1) * 8))) return r;
        if ((r = ensure(t, sl.d_text, (size_t)nb + 64))) return r;
        if ((r = ensure(t, sl.d_offs, (size_t)(nd + 1) * 8))) return r;
        if ((r = ensure(t, sl.d_toff, (size_t)(nd + 1) * 8))) return r;
        if ((r = ensure(t, sl.d_tok, (size_t)std::max<int64_t>(nb, 1) * 4))) return r;  // worst case one id per byte
        int64_t* ho = (int64_t*)sl.h_offs.p;
        for (int64_t k = 0; k <= nd; ++k) ho[k] = doc_offsets[d0 + k] - b0;
        lap(1, t0);
        t0 = now();
        if (in_job[i % NS]) { t->pool_threads->wait(in_job[i % NS]); in_job[i % NS].reset(); }
        lap(0, t0);
        t0 = now();
        if (nb > 0) HIP_TRY(t, hipMemcpyAsync(sl.d_text.p, sl.h_text.p, (size_t)nb, hipMemcpyHostToDevice, t->s_h2d));
        HIP_TRY(t, hipMemcpyAsync(sl.d_offs.p, sl.h_offs.p, (size_t)(nd + 1) * 8, hipMemcpyHostToDevice, t->s_h2d));
        HIP_TRY(t, hipEventRecord(sl.ev_h2d, t->s_h2d));
        HIP_TRY(t, hipStreamWaitEvent(t->s_k, sl.ev_h2d, 0));
        if ((r = encode_device_locked(t, sl.d_text.p, nb, sl.d_offs.p, nd, mode, sl.d_tok.p, std::max<int64_t>(nb, 1), sl.d_toff.p, t->s_k))) return r;
        // the chunk's error word and the workspace counters travel with its offsets (the next chunk resets the counters)
        if (publish) {
            HIP_TRY(t, launch_pipe_publish(t->ctl.p, (uint32_t)sizeof(Ctl), sl.h_ctl.p, (const int64_t*)sl.d_toff.p, nd + 1, (int64_t*)sl.h_offs.p, t->s_k));
        } else {
            HIP_TRY(t, hipMemcpyAsync(sl.h_ctl.p, t->ctl.p, sizeof(Ctl), hipMemcpyDeviceToHost, t->s_k));
            HIP_TRY(t, hipMemcpyAsync(sl.h_offs.p, sl.d_toff.p, (size_t)(nd + 1) * 8, hipMemcpyDeviceToHost, t->s_k));
        }
        HIP_TRY(t, hipEventRecord(sl.ev_off, t->s_k));
        lap(1, t0);
        return TD_OK;
    };
    auto fetch = [&](int i) -> int {  // chunk i's kernels are done: its total is known, its ids start their way up
        td_tokenizer::PipeSlot& sl = t->pipe[i % NS];
        Pending& P = pend[(size_t)i];
        auto t0 = now();
        HIP_TRY(t, hipEventSynchronize(sl.ev_off));
        lap(2, t0);
        const int64_t nd = P.d1 - P.d0;
        const int64_t* to = (const int64_t*)sl.h_offs.p;
        const Ctl& c = *(const Ctl*)sl.h_ctl.p;
        P.ntok = to[nd];
        t->last_direct += c.direct_tiles;  // (td_info: sums over the call's chunks)
        t->last_timeouts += c.lb_timeouts;
        if (c.err != 0 && first_err == TD_OK) {
            first_err = c.err;
            const long long pos = c.err_pos + (first_err == TD_E_UNKNOWN_BYTE || first_err == TD_E_SCRATCH ? P.b0 : 0);
            t->err = first_err == TD_E_UNKNOWN_BYTE ? device_error_text(first_err, pos, false)
                                                    : "device error " + std::to_string(first_err) + " near byte offset " + std::to_string(pos);
        }
        for (int64_t k = 0; k < nd; ++k) out_offsets[P.d0 + k] = tok_base + to[k];
        if (tok_base + P.ntok > out_capacity) capacity_miss = true;
        int r;
        // the slot's pinned id buffer was chunk i - NS's: its ids have to have left it (the pool's copy, started three rounds ago)
        t0 = now();
        if (out_job[i % NS]) { t->pool_threads->wait(out_job[i % NS]); out_job[i % NS].reset(); }
        lap(3, t0);
        if ((r = pinned_ensure(t, sl.h_tok, (size_t)std::max<int64_t>(P.ntok, 1) * 4))) return r;
        if (P.ntok > 0 && !capacity_miss && first_err == TD_OK)
        {
            if (d2h_blocks > 0) HIP_TRY(t, launch_pipe_copy_out(sl.d_tok.p, sl.h_tok.p, P.ntok, d2h_blocks, t->s_d2h));
            else HIP_TRY(t, hipMemcpyAsync(sl.h_tok.p, sl.d_tok.p, (size_t)P.ntok * 4, hipMemcpyDeviceToHost, t->s_d2h));
        }
        HIP_TRY(t, hipEventRecord(sl.ev_tok, t->s_d2h));
        const int64_t base = tok_base;
        tok_base += P.ntok;
        P.nbytes = base;  // (reused: where the chunk's ids go in the caller's buffer)
        return TD_OK;
    };
    auto deliver = [&](int i) -> int {  // chunk i's ids are in its pinned buffer: the pool copies them out while the next chunks go in
        td_tokenizer::PipeSlot& sl = t->pipe[i % NS];
        const Pending& P = pend[(size_t)i];
        auto t0 = now();
        HIP_TRY(t, hipEventSynchronize(sl.ev_tok));
        lap(4, t0);
        t0 = now();
        if (P.ntok > 0 && !capacity_miss && first_err == TD_OK) out_job[i % NS] = t->pool_threads->copy(out_tokens + P.nbytes, sl.h_tok.p, (size_t)P.ntok * 4);
        lap(5, t0);
        return TD_OK;
    };
    // Round 5: the host thread no longer WAITS for a copy it has just started.  The text of chunk i + 1 goes into its pinned buffer
    // while chunk i is enqueued and chunks i - 1, i - 2 are collected, and a slot's ids have three rounds to leave it (four slots):
    // with three slots and the text copied inside submit() a round was out-copy + in-copy back to back on this thread (1.1 ms per
    // 32 MiB chunk: 37 ms per GiB of English = 0.50 of what the two PCIe directions allow side by side).
    if (nchunks > 0) rc = start_in(0);
    for (int i = 0; rc == TD_OK && i < nchunks + 2; ++i) {
        if (i < nchunks && (rc = submit(i))) break;
        if (i + 1 < nchunks && (rc = start_in(i + 1))) break;
        if (i - 1 >= 0 && i - 1 < nchunks && (rc = fetch(i - 1))) break;
        if (i - 2 >= 0 && i - 2 < nchunks && (rc = deliver(i - 2))) break;
    }
    for (auto& j : in_job) if (j) t->pool_threads->wait(j);
    for (auto& j : out_job) if (j) t->pool_threads->wait(j);
    if (timing)
        fprintf(stderr, "[tokendagger] pipeline: %d chunks; host thread ms: wait text copy %.2f | enqueue %.2f | wait kernels %.2f | wait out-copy %.2f | wait ids %.2f | start copies %.2f\n",
                nchunks, tm[0], tm[1], tm[2], tm[3], tm[4], tm[5]);
    if (rc != TD_OK) {
        // a chunk failed on the host side (allocation, a HIP call): nothing of this call may still be reading the caller's
        // text or writing its output buffers when the error is returned — the copy jobs are done (above), the three streams
        // are drained here
        (void)hipStreamSynchronize(t->s_h2d);
        (void)hipStreamSynchronize(t->s_k);
        (void)hipStreamSynchronize(t->s_d2h);
        return rc;
    }
    out_offsets[n_docs] = tok_base;
    if (n_tokens) *n_tokens = tok_base;
    HIP_TRY(t, hipStreamSynchronize(t->s_k));
    if (first_err != TD_OK) {
        if ((rc = zero_wait(t, t->ctl.p, sizeof(Ctl), t->s_k))) return rc;
        return first_err;
    }
    // (the checks only: the ids went out chunk by chunk, unless a chunk's end lay beyond the capacity)
    return deliver_ids(t, tok_base, out_capacity, out_tokens, n_tokens, [] { return (int)TD_OK; });
}

// ---- tiny inputs: ONE launch, no hipMemcpy, no stream synchronisation ------------------------------
constexpr int64_t SMALL_MAX_BYTES = 4096, SMALL_MAX_DOCS = 1024;
static_assert(SMALL_MAX_DOCS == SM_MAXDOCS, "td_small_encode keeps the document offsets in LDS");
constexpr size_t SMALL_IN_BYTES = 64 + (SMALL_MAX_DOCS + 2) * 8 + SMALL_MAX_BYTES + 256;  // (64: td_small_resident's request header)
constexpr size_t SMALL_OUT_BYTES = 64 + (SMALL_MAX_DOCS + 2) * 8 + SMALL_MAX_BYTES * 4 + 256;
// returns TD_OK, a TD_E_* code, or -1: the kernel handed the call back (a piece above 1024 bytes); TD_INFO_SMALL_ENCODES / _HANDBACKS count which
int encode_batch_small(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode,
                       int32_t* out_tokens, int64_t out_capacity, int64_t* out_offsets, int64_t* n_tokens) {
    const int64_t n = doc_offsets[n_docs];
    if (!t->small_in.p) {  // (both or neither)
        PinnedBuf in, out;
        HIP_TRY(t, make_pinned(in, SMALL_IN_BYTES));
        HIP_TRY(t, make_pinned(out, SMALL_OUT_BYTES));
        memset(out.p, 0, SMALL_OUT_BYTES);
        t->small_in = std::move(in);
        t->small_out = std::move(out);
    }
    int rc;
    if ((rc = own_streams(t))) return rc;
    const size_t offs_bytes = (((size_t)(n_docs + 1) * 8) + 15) & ~(size_t)15;
    uint8_t* in = (uint8_t*)t->small_in.p;
    memcpy(in + 64, doc_offsets, (size_t)(n_docs + 1) * 8);
    memcpy(in + 64 + offs_bytes, text, (size_t)n);
    uint8_t* out = (uint8_t*)t->small_out.p;
    SmallArgs a;
    a.Tp = t->dTp;
    a.doc_offsets = (const int64_t*)(in + 64);
    a.text = in + 64 + offs_bytes;
    a.status = (SmallStatus*)out;
    a.out_offsets = (int64_t*)(out + 64);
    a.out_tokens = (int32_t*)(out + 64 + offs_bytes);
    a.seq = ++t->small_seq;
    a.n = (int)n;
    a.n_docs = (int)n_docs;
    a.use_fastpath = (mode == TD_MODE_ENCODE) || t->H.merge_closed;
    volatile unsigned long long* seqp = &a.status->seq;
    hipStream_t s = t->s_own;
    if (t->opt.small_resident) {
        // the request for td_small_resident: header fields, then the sequence number (release); the kernel is launched when the last one
        // has left (its generation stands at out + 40 then) — it reads tables and pinned buffers only, so it needs no ordering with the
        // handle's other work
        if (!t->s_res) HIP_TRY(t, make_stream(t->s_res));
        SmallMailbox* mb = (SmallMailbox*)in;
        mb->n = a.n; mb->n_docs = a.n_docs; mb->use_fastpath = a.use_fastpath; mb->offs_bytes = (int)offs_bytes;
        __atomic_store_n(&mb->seq, a.seq, __ATOMIC_RELEASE);
        volatile unsigned long long* exitp = (volatile unsigned long long*)(out + 40);
        auto launch = [&]() -> int {
            ++t->res_gen;
            HIP_TRY(t, launch_small_resident(t->dTp, in, out, t->res_gen, t->opt.small_idle_ticks, t->s_res));
            return TD_OK;
        };
        if (t->res_gen == 0 || __atomic_load_n(exitp, __ATOMIC_ACQUIRE) == t->res_gen) { if ((rc = launch())) return rc; }
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t spins = 0;; ++spins) {
            if (__atomic_load_n(seqp, __ATOMIC_ACQUIRE) == a.seq) break;
            if ((spins & 0x3Fu) == 0x3Fu && __atomic_load_n(exitp, __ATOMIC_ACQUIRE) == t->res_gen) {
                // the kernel left (idle time over) without having seen this request: the next generation answers it
                if (__atomic_load_n(seqp, __ATOMIC_ACQUIRE) == a.seq) break;
                if ((rc = launch())) return rc;
            }
            if ((spins & 0xFFFFu) == 0xFFFFu && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(5)) {
                HIP_TRY(t, hipStreamSynchronize(t->s_res));  // (a launch failure surfaces here)
                if (__atomic_load_n(seqp, __ATOMIC_ACQUIRE) == a.seq) break;
                t->err = "td_small_resident did not answer";
                return TD_E_HIP;
            }
        }
    } else {
    if ((rc = order_before(t, s))) return rc;
    HIP_TRY(t, launch_small_encode(a, s));
    // the kernel releases its sequence number (system scope) after everything else it wrote: spin on it
    if ((rc = wait_for_seq(t, seqp, a.seq, s, 0xFFFu, 5, "td_small_encode did not complete"))) return rc;
    }
    const SmallStatus st = *a.status;
    if (st.fallback) { ++t->small_encode_handbacks; return -1; }
    ++t->small_encodes;  // (an error the kernel reported is its answer too)
    if (st.err) {
        t->err = st.err == TD_E_UNKNOWN_BYTE ? device_error_text(st.err, st.err_pos, false) : "device error " + std::to_string(st.err);
        return st.err;
    }
    memcpy(out_offsets, a.out_offsets, (size_t)(n_docs + 1) * 8);
    return deliver_ids(t, (int64_t)st.n_tokens, out_capacity, out_tokens, n_tokens, [&] {
        memcpy(out_tokens, a.out_tokens, (size_t)st.n_tokens * 4);
        return (int)TD_OK;
    });
}

// Host batches of 4 KiB .. 4 MiB (a document, a file, a chat transcript — the calls /root/reference/tests/code_performance_benchmark.py:338-396
// times one by one).  Rounds 1-5: two pageable H2D copies, the step, then THREE copy-and-synchronise round trips (control block, offsets, ids):
// 64 KB of English took 226 us of which the kernels' work was under 20.  Round 6: text and offsets go through ONE pinned buffer and one
// asynchronous copy; the step's pack kernels write ids and offsets STRAIGHT into pinned host memory (they are its output buffers); a last
// one-workgroup kernel copies the control block there and releases a sequence number (system scope) the host spins on — no
// hipStreamSynchronize, no D2H copy on the way back.
constexpr int64_t MID_MAX_BYTES = 4ll << 20, MID_MAX_DOCS = 1ll << 18;
int encode_batch_mid(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode,
                     int32_t* out_tokens, int64_t out_capacity, int64_t* out_offsets, int64_t* n_tokens) {
    const int64_t n = doc_offsets[n_docs];
    int rc;
    const size_t offs_bytes = (((size_t)(n_docs + 1) * 8) + 63) & ~(size_t)63;
    const size_t in_bytes = offs_bytes + (size_t)n + 64;
    const size_t out_bytes = 512 + offs_bytes + (size_t)n * 4 + 64;
    if ((rc = pinned_ensure(t, t->mid_in, in_bytes))) return rc;
    if (!t->mid_out.p || t->mid_out.cap < out_bytes) {
        if ((rc = pinned_ensure(t, t->mid_out, out_bytes))) return rc;
        memset(t->mid_out.p, 0, 512);
    }
    if ((rc = ensure(t, t->mid_dev, in_bytes))) return rc;
    if ((rc = own_streams(t))) return rc;
    hipStream_t s = t->s_own;
    if ((rc = order_before(t, s))) return rc;
    uint8_t* in = (uint8_t*)t->mid_in.p;
    memcpy(in, doc_offsets, (size_t)(n_docs + 1) * 8);
    memcpy(in + offs_bytes, text, (size_t)n);
    HIP_TRY(t, hipMemcpyAsync(t->mid_dev.p, in, offs_bytes + (size_t)n, hipMemcpyHostToDevice, s));
    uint8_t* out = (uint8_t*)t->mid_out.p;  // [0, 256): control block | [256]: sequence number | 512: offsets | ids
    int64_t* h_offs = (int64_t*)(out + 512);
    int32_t* h_tok = (int32_t*)(out + 512 + offs_bytes);
    rc = encode_device_locked(t, (uint8_t*)t->mid_dev.p + offs_bytes, n, t->mid_dev.p, n_docs, mode, h_tok, std::max<int64_t>(n, 1), h_offs, s);
    if (rc) return rc;
    const unsigned long long seq = ++t->mid_seq;
    HIP_TRY(t, launch_mid_done(t->ctl.p, (uint32_t)sizeof(Ctl), out, (unsigned long long*)(out + 256), seq, s));
    if ((rc = wait_for_seq(t, (volatile unsigned long long*)(out + 256), seq, s, 0xFFFFu, 20, "td_encode_batch: the step did not complete"))) return rc;
    if (!t->has_last || t->last_stream == s) t->graveyard.clear();  // (the sequence number is written behind the step's last kernel: nothing of this handle is in flight)
    if ((rc = absorb_ctl(t, *(const Ctl*)out, s, nullptr))) return rc;
    memcpy(out_offsets, h_offs, (size_t)(n_docs + 1) * 8);
    const int64_t total = out_offsets[n_docs];
    return deliver_ids(t, total, out_capacity, out_tokens, n_tokens, [&] {
        memcpy(out_tokens, h_tok, (size_t)total * 4);
        return (int)TD_OK;
    });
}

}  // namespace

// out_starts (optional, capacity out_capacity): the start of every id in its document in `unit` (td_encode_batch_with_starts); such
// calls take the plain path below whatever the size
int td::encode_batch_locked(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode, int32_t* out_tokens,
                            int64_t out_capacity, int64_t* out_offsets, int64_t* n_tokens, int unit, int64_t* out_starts) {
    int rc;
    if ((rc = check_offsets(t, "doc_offsets", doc_offsets, n_docs, text))) return rc;
    const int64_t n = doc_offsets[n_docs];
    const bool plain = t->gx_prefix_host != nullptr || out_starts;  // (context prefixes of a generic pattern, starts: the plain path below, whatever the size)
    if (n > 0 && n <= SMALL_MAX_BYTES && n_docs <= SMALL_MAX_DOCS && t->opt.small_enabled && t->H.pattern_kind != PATTERN_GENERIC && !out_starts) {  // (the one-launch kernel knows the family's scanners only)
        rc = encode_batch_small(t, text, doc_offsets, n_docs, mode, out_tokens, out_capacity, out_offsets, n_tokens);
        if (rc != -1) return rc;  // (-1: a piece above 64 bytes; the general path below handles it)
    }
    if (n > 0 && n <= MID_MAX_BYTES && n_docs <= MID_MAX_DOCS && t->opt.mid_enabled && !plain)
        return encode_batch_mid(t, text, doc_offsets, n_docs, mode, out_tokens, out_capacity, out_offsets, n_tokens);
    if (n >= t->opt.pipe_chunk_bytes / 2 && out_tokens && !plain)  // (default: from 32 MiB on)
        return encode_batch_pipelined(t, text, doc_offsets, n_docs, mode, out_tokens, out_capacity, out_offsets, n_tokens);
    if ((rc = ensure(t, t->h2d_text, (size_t)n + 64))) return rc;
    if ((rc = ensure(t, t->h2d_offs, (size_t)(n_docs + 1) * 8))) return rc;
    if ((rc = ensure(t, t->d_offsets, (size_t)(n_docs + 1) * 8))) return rc;
    // worst case one token per byte; typical text needs a quarter of that
    const int64_t dev_cap = std::max<int64_t>(n, 1);
    if ((rc = ensure(t, t->d_tokens, (size_t)dev_cap * 4))) return rc;
    if ((rc = own_streams(t))) return rc;
    hipStream_t s = t->s_own;
    if ((rc = order_before(t, s))) return rc;
    if (n > 0) HIP_TRY(t, hipMemcpyAsync(t->h2d_text.p, text, (size_t)n, hipMemcpyHostToDevice, s));
    HIP_TRY(t, hipMemcpyAsync(t->h2d_offs.p, doc_offsets, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice, s));
    if (t->gx_prefix_host) {
        if ((rc = ensure(t, t->gx_prefix, (size_t)n_docs + 16))) return rc;
        HIP_TRY(t, hipMemcpyAsync(t->gx_prefix.p, t->gx_prefix_host, (size_t)n_docs, hipMemcpyHostToDevice, s));
        t->gx_prefix_dev = (const uint8_t*)t->gx_prefix.p;
    }
    rc = encode_device_locked(t, t->h2d_text.p, n, t->h2d_offs.p, n_docs, mode, t->d_tokens.p, dev_cap, t->d_offsets.p, s);
    t->gx_prefix_dev = nullptr;
    if (rc) return rc;
    if (out_starts) {
        if ((rc = ensure(t, t->off_starts, (size_t)dev_cap * 8))) return rc;
        if ((rc = encode_starts_locked(t, t->h2d_text.p, n, t->h2d_offs.p, n_docs, t->d_tokens.p, dev_cap, t->d_offsets.p, unit, t->off_starts.p, s)))
            return rc;
    }
    rc = device_status_locked(t, s, nullptr);
    if (rc) return rc;
    if ((rc = copy_wait(t, out_offsets, t->d_offsets.p, (size_t)(n_docs + 1) * 8, hipMemcpyDeviceToHost, s))) return rc;
    const int64_t total = out_offsets[n_docs];
    return deliver_ids(t, total, out_capacity, out_tokens, n_tokens, [&] {
        int rc2;
        if ((rc2 = copy_wait(t, out_tokens, t->d_tokens.p, (size_t)total * 4, hipMemcpyDeviceToHost, s))) return rc2;
        return out_starts ? copy_wait(t, out_starts, t->off_starts.p, (size_t)total * 8, hipMemcpyDeviceToHost, s) : (int)TD_OK;
    });
}

extern "C" {

int td_create(const char* pat_str, int64_t n_vocab, const uint8_t* token_bytes, const int64_t* token_offsets,
              const int32_t* ranks, int64_t n_special, const uint8_t* special_bytes, const int64_t* special_offsets,
              const int32_t* special_ids, int device, td_tokenizer** out) {
    if (!out) return TD_E_INVALID;
    *out = nullptr;
    if (!pat_str || !token_bytes || !token_offsets || !ranks || n_vocab <= 0 || n_special < 0) {
        g_create_err = "td_create: bad argument";
        return TD_E_INVALID;
    }
    td_tokenizer* t = new td_tokenizer;
    t->opt = Options::from_env();
    std::string err;
    int rc = build_tables(pat_str, n_vocab, token_bytes, token_offsets, ranks, n_special, special_bytes, special_offsets,
                          special_ids, t->H, err);
    if (rc != TD_OK) {
        g_create_err = err;
        delete t;
        return rc;
    }
    auto fail = [&](int code) {
        g_create_err = t->err;
        td_destroy(t);
        return code;
    };
    int ndev = 0;
    hipError_t he = hipGetDeviceCount(&ndev);
    if (he != hipSuccess || ndev <= 0) {
        t->err = std::string("no usable HIP device (") + hipGetErrorString(he) + "); this library has no CPU path";
        return fail(TD_E_HIP);
    }
    if (device < 0) {
        if (hipGetDevice(&device) != hipSuccess) device = 0;
    }
    if (device >= ndev) { t->err = "device index out of range"; return fail(TD_E_INVALID); }
    t->device = device;
    t->shared->device = device;
    DeviceGuard dg(device);  // uploads go to the handle's device; the caller's current device is restored on return
    {
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess || cur != device) { t->err = "hipSetDevice failed"; return fail(TD_E_HIP); }
    }
    if ((rc = own_streams(t))) return fail(rc);
    const HostTables& H = t->H;
    const Tables hv = H.view();
    Tables d;
    memset(&d, 0, sizeof d);
    d.piece_mask = H.piece_mask;
    d.pair_mask = H.pair_mask;
    d.max_id = H.max_id;
    d.pseudo_base = H.pseudo_base;
    d.max_token_len = H.max_token_len;
    d.piece12_mask = H.piece12_mask;
    d.pat_flags = hv.pat_flags;
    if ((rc = upload(t, H.ascii_cls.data(), H.ascii_cls.size(), &d.ascii_cls))) return fail(rc);
    if ((rc = upload(t, hv.ucls1, (size_t)4352, &d.ucls1))) return fail(rc);
    {
        // size of stage 2 = (max block index + 1) * 256
        unsigned maxb = 0;
        for (int i = 0; i < 4352; ++i) maxb = std::max<unsigned>(maxb, hv.ucls1[i]);
        if ((rc = upload(t, hv.ucls2, (size_t)(maxb + 1) * 256, &d.ucls2))) return fail(rc);
    }
    if ((rc = upload(t, H.byte_id.data(), H.byte_id.size(), &d.byte_id))) return fail(rc);
    if ((rc = upload(t, H.byte_pair.data(), H.byte_pair.size(), &d.byte_pair))) return fail(rc);
    if ((rc = upload(t, H.byte_pair_id.data(), H.byte_pair_id.size(), &d.byte_pair_id))) return fail(rc);
    if ((rc = upload(t, H.piece_slots.data(), H.piece_slots.size(), &d.piece_slots))) return fail(rc);
    if ((rc = upload(t, H.piece12_slots.data(), H.piece12_slots.size(), &d.piece12_slots))) return fail(rc);
    if ((rc = upload(t, H.pair_slots.data(), H.pair_slots.size(), &d.pair_slots))) return fail(rc);
    if ((rc = upload(t, H.tok_off.data(), H.tok_off.size(), &d.tok_off))) return fail(rc);
    if ((rc = upload(t, H.tok_bytes.data(), H.tok_bytes.size(), &d.tok_bytes))) return fail(rc);
    d.cseed = nullptr; d.cseed_pm = nullptr; d.cseed_nm = nullptr;
    if (!H.cseed.empty()) {  // characters that enter the merge loop whole (td_common.h: character seeds)
        if ((rc = upload(t, H.cseed.data(), H.cseed.size(), &d.cseed))) return fail(rc);
        if ((rc = upload(t, H.cseed_pm.data(), H.cseed_pm.size(), &d.cseed_pm))) return fail(rc);
        if ((rc = upload(t, H.cseed_nm.data(), H.cseed_nm.size(), &d.cseed_nm))) return fail(rc);
    }
    if (H.pattern_kind == PATTERN_GENERIC) {
        size_t n1 = 0, n2 = 0;
        const uint16_t* s1 = rx_stage1(&n1);
        const uint8_t* s2 = rx_stage2(&n2);
        if ((rc = upload(t, reinterpret_cast<const RxProgram*>(H.rx_program.data()), 1, &t->d_rx))) return fail(rc);
        if ((rc = upload(t, s1, n1, &t->d_rx_s1))) return fail(rc);
        if ((rc = upload(t, s2, n2, &t->d_rx_s2))) return fail(rc);
    }
    {
        // per id (specials included): characters = bytes that are not continuation bytes, << 1 | the first byte is one.  Not a
        // member of Tables (its argument footprint is tuned): the starts kernels take it as an argument of their own.
        std::vector<uint32_t> ctab((size_t)H.max_id + 1, 0);
        for (int32_t id = 0; id <= H.max_id; ++id) {
            const uint32_t lo = H.tok_off[(size_t)id], hi = H.tok_off[(size_t)id + 1];
            if (hi == lo) continue;
            uint32_t c = 0;
            for (uint32_t q = lo; q < hi; ++q) c += (H.tok_bytes[q] & 0xC0u) != 0x80u;
            ctab[(size_t)id] = c << 1 | ((H.tok_bytes[lo] & 0xC0u) == 0x80u ? 1u : 0u);
        }
        if ((rc = upload(t, ctab.data(), ctab.size(), &t->d_ctab))) return fail(rc);
    }
    t->dT = d;
    if ((rc = upload(t, &t->dT, 1, &t->dTp))) return fail(rc);
    if ((rc = ensure(t, t->ctl, CTL_BYTES + TD_GP_SCRATCH_BYTES))) return fail(rc);
    if ((rc = zero_wait(t, t->ctl.p, sizeof(Ctl), t->s_own))) return fail(rc);
    *out = t;
    return TD_OK;
}

int td_clone(td_tokenizer* src, td_tokenizer** out) {
    if (!out) return TD_E_INVALID;
    *out = nullptr;
    if (!src) { g_create_err = "td_clone: bad argument"; return TD_E_INVALID; }
    td_tokenizer* t = nullptr;
    {
        std::lock_guard<std::mutex> g(src->mu);  // (its options are read)
        t = new td_tokenizer(src->shared);
        t->dT = src->dT; t->dTp = src->dTp; t->device = src->device;
        t->d_rx = src->d_rx; t->d_rx_s1 = src->d_rx_s1; t->d_rx_s2 = src->d_rx_s2; t->d_ctab = src->d_ctab;
        t->opt = src->opt;
    }
    DeviceGuard dg(t->device);
    int rc = own_streams(t);
    if (rc == TD_OK) rc = ensure(t, t->ctl, CTL_BYTES + TD_GP_SCRATCH_BYTES);
    if (rc == TD_OK) rc = zero_wait(t, t->ctl.p, sizeof(Ctl), t->s_own);
    if (rc != TD_OK) {
        g_create_err = t->err;
        td_destroy(t);
        return rc;
    }
    *out = t;
    return TD_OK;
}

// The handle's members free themselves (owner types); what td_destroy adds is the condition that makes that safe: they are
// destroyed only after everything the handle has in flight is done (drain, the resident small-call kernel's stream — it reads
// the pinned small-path buffers), and with the handle's device current.
void td_destroy(td_tokenizer* t) {
    if (!t) return;
    if (g_thread_err_owner == t) g_thread_err_owner = nullptr;
    DeviceGuard dg(t->device);  // reached from finalisers at arbitrary points: the caller's device must survive
    drain(t);  // (not hipDeviceSynchronize: other handles' and the application's streams are none of this handle's business)
    if (t->s_res) (void)hipStreamSynchronize(t->s_res);  // (the resident small-call kernel leaves by itself within its idle time)
    delete t;
}

const char* td_last_error(const td_tokenizer* t) {
    if (!t) return g_create_err.c_str();
    // this thread's copy of the message of ITS last failing call on the handle (never a pointer into storage that
    // another thread's call may be rewriting)
    return g_thread_err_owner == t ? g_thread_err.c_str() : "";
}

int td_reserve(td_tokenizer* t, int64_t max_bytes, int64_t max_docs) {
    if (!t || max_bytes < 0 || max_docs < 0) return TD_E_INVALID;
    // (an encode_ordinary call on a vocabulary the merge loop does not reproduce merges EVERY piece: reserve for that, so that no
    // call after td_reserve allocates — ADVICE r4)
    return locked(t, [&] { return reserve_ws(t, std::max<int64_t>(max_bytes, 1), max_docs, !t->H.merge_closed); });
}

int td_encode_device(td_tokenizer* t, const void* d_text, int64_t n_bytes, const void* d_doc_offsets, int64_t n_docs,
                     int mode, void* d_out_tokens, int64_t out_capacity, void* d_out_offsets, void* hip_stream) {
    if (!t) return TD_E_INVALID;
    return locked(t, [&] {
        return encode_device_locked(t, d_text, n_bytes, d_doc_offsets, n_docs, mode, d_out_tokens, out_capacity,
                                    d_out_offsets, (hipStream_t)hip_stream);
    });
}

int td_device_status(td_tokenizer* t, void* hip_stream, int64_t* err_pos) {
    if (!t) return TD_E_INVALID;
    return locked(t, [&] { return device_status_locked(t, (hipStream_t)hip_stream, err_pos); });
}

int td_encode_batch(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode,
                    int32_t* out_tokens, int64_t out_capacity, int64_t* out_offsets, int64_t* n_tokens) {
    if (!t || !doc_offsets || n_docs < 0 || !out_offsets || out_capacity < 0) return TD_E_INVALID;
    if ((mode == TD_MODE_ENCODE || mode == TD_MODE_ORDINARY) && doc_offsets[0] == 0 && doc_offsets[n_docs] == 0) {
        // nothing but empty documents: no ids, and no reason to wake the device (enc.encode("") was 48 us)
        for (int64_t d = 0; d <= n_docs; ++d) out_offsets[d] = 0;
        if (n_tokens) *n_tokens = 0;
        return TD_OK;
    }
    return locked(t, [&] { return encode_batch_locked(t, text, doc_offsets, n_docs, mode, out_tokens, out_capacity, out_offsets, n_tokens); });
}

int64_t td_info(const td_tokenizer* t, int what) {
    if (!t) return -1;
    switch (what) {
        case TD_INFO_N_PAIRS: return (int64_t)t->H.n_pairs;
        case TD_INFO_MERGE_CLOSED: return t->H.merge_closed ? 1 : 0;
        case TD_INFO_MAX_ID: return t->H.max_id;
        case TD_INFO_TILE_BYTES: return K_TILE;
        case TD_INFO_WORKSPACE_BYTES: return (int64_t)t->ws_bytes;
        case TD_INFO_N_SPECIAL: return (int64_t)t->H.special_ids.size();
        case TD_INFO_LONG_PIECES: return t->last_long;
        case TD_INFO_FAR_PIECES: return t->last_far;
        case TD_INFO_DEFERRED_TILES: return t->last_deferred;
        case TD_INFO_FLAGGED_TILES: return t->last_flagged;
        case TD_INFO_DIRECT_TILES: return t->last_direct;
        case TD_INFO_LB_TIMEOUTS: return t->last_timeouts;
        case TD_INFO_REPEATS: return t->last_repeats;
        case TD_INFO_LISTED_PIECES: return t->last_listed;
        case TD_INFO_CHAR_SEEDS: return (int64_t)t->H.n_char_seeds;
        case TD_INFO_SPARSE: return t->last_sparse ? 1 : 0;
        case TD_INFO_WS_FILLED_BYTES: return t->ws_filled;
        case TD_INFO_SMALL_ENCODES: return t->small_encodes;
        case TD_INFO_SMALL_ENCODE_HANDBACKS: return t->small_encode_handbacks;
        case TD_INFO_SMALL_DECODES: return t->small_decodes;
        case TD_INFO_SMALL_DECODE_HANDBACKS: return t->small_decode_handbacks;
    }
    return -1;
}

int td_set_option(td_tokenizer* t, int what, int64_t value) {
    if (!t) return TD_E_INVALID;
    std::lock_guard<std::mutex> g(t->mu);
    Options& o = t->opt;
    auto relaunch = [t] { drop_graph(t); t->has_last_key = false; return (int)TD_OK; };  // (options that change the captured launches)
    switch (what) {
        case TD_OPT_LONG_POOL_BYTES: if (value < (1 << 20)) break; o.pool_bytes_opt = value; return TD_OK;
#ifdef TD_ABLATE
        case 99: t->stop_after = (int)value; return TD_OK;  // tuning builds only (tools/build_variant.sh -DTD_ABLATE): phase ablation, results are garbage when != 0
#endif
        case TD_OPT_FUSED: o.fused = value != 0; return TD_OK;
        case TD_OPT_DIRECT: o.direct = value != 0; return TD_OK;
        case TD_OPT_DEVICE_SPECIALS: o.device_specials = value != 0; return TD_OK;
        case TD_OPT_PACK_SPLIT: o.pack_split = value != 0; return relaunch();
        case TD_OPT_SPARSE: if (value < -1 || value > 1) break; o.sparse_opt = (int)value; return relaunch();
        case TD_OPT_OVERLAP: o.overlap = value != 0; return relaunch();
        case TD_OPT_GIANT_COOP_MIN: if (value < 1024) break; o.gp_coop_min = (uint32_t)std::min<int64_t>(value, 0x7FFFFFFF); return relaunch();
        case TD_OPT_DEDUPE: o.dedupe = value != 0; return relaunch();
        case TD_OPT_GRAPH: o.graphs = value != 0; return o.graphs ? (int)TD_OK : relaunch();
        case TD_OPT_PROFILE: t->profile = value != 0; return TD_OK;
        case TD_OPT_PIPE_CHUNK_BYTES: if (value < 4096) break; o.pipe_chunk_bytes = value; return TD_OK;
        case TD_OPT_SMALL_PATH: o.small_enabled = value != 0; return TD_OK;
        case TD_OPT_PIPE_THREADS: if (value < 1 || value > 256) break; o.pipe_threads = (int)value; return TD_OK;
        case TD_OPT_COUNTS_FLUSH_TILES: if (value < 0 || value > CNT_FLUSH_TILES) break; o.counts_flush_tiles = (int)value; return TD_OK;
        case TD_OPT_NGRAM_TAG_BITS: if (value < 0 || value > 31) break; o.ngram_tag_bits = (int)value; return TD_OK;
        case TD_OPT_WS_FILL: if (value < -1 || value > 255) break; o.ws_fill = (int)value; return TD_OK;
        case TD_OPT_COUNTS_SEATS: {  // a power of two from 2 to the production size, or 0 for it
            if (value == 0) { o.counts_seat_bits = 0; return TD_OK; }
            if (value < 2 || value > CNT_SEATS || (value & (value - 1))) break;
            int bits = 0;
            while ((int64_t(1) << bits) < value) ++bits;
            o.counts_seat_bits = bits;
            return TD_OK;
        }
    }
    return TD_E_INVALID;
}

static const char* const kProfSegments[TD_PROF_EVENTS - 1] = {"td_prepare+td_mark_docs", "td_split_tiles", "td_probe_tiles", "td_merge_pieces",
                                                              "td_long_pieces+td_giant_pieces+td_scan_tiles", "td_pack_tokens"};

int td_profile_read_ex(td_tokenizer* t, double* ms_sums, int n_segments, int64_t* launches) {
    if (!t || n_segments < 0 || (n_segments > 0 && !ms_sums)) return TD_E_INVALID;
    return locked(t, [&] {
        double sum[TD_PROF_EVENTS - 1] = {};
        int64_t n = 0;
        for (auto& ev : t->ev_pending) {
            HIP_TRY(t, hipEventSynchronize(ev.e[TD_PROF_EVENTS - 1]));
            for (int k = 0; k + 1 < TD_PROF_EVENTS; ++k) {
                float ms = 0;
                HIP_TRY(t, hipEventElapsedTime(&ms, ev.e[k], ev.e[k + 1]));
                sum[k] += ms;
            }
            ++n;
        }
        for (auto& ev : t->ev_pending) t->ev_free.push_back(std::move(ev));
        t->ev_pending.clear();
        for (int k = 0; k < n_segments; ++k) ms_sums[k] = k + 1 < TD_PROF_EVENTS ? sum[k] : 0.0;
        if (launches) *launches = n;
        return (int)TD_OK;
    });
}

const char* td_profile_segment_name(int i) { return (i >= 0 && i + 1 < TD_PROF_EVENTS) ? kProfSegments[i] : ""; }

int td_profile_read(td_tokenizer* t, double* split_ms_sum, double* encode_ms_sum, int64_t* launches) {
    double s[TD_PROF_EVENTS - 1] = {};
    const int rc = td_profile_read_ex(t, s, TD_PROF_EVENTS - 1, launches);
    if (split_ms_sum) *split_ms_sum = s[1];
    if (encode_ms_sum) *encode_ms_sum = s[2] + s[3];
    return rc;
}

int64_t td_special_count(const td_tokenizer* t) { return t ? (int64_t)t->H.special_ids.size() : 0; }

int td_special_get(const td_tokenizer* t, int64_t i, const char** str, int64_t* len, int32_t* id) {
    if (!t || i < 0 || i >= (int64_t)t->H.special_ids.size()) return TD_E_INVALID;
    if (str) *str = t->H.special_strs[(size_t)i].data();
    if (len) *len = (int64_t)t->H.special_strs[(size_t)i].size();
    if (id) *id = t->H.special_ids[(size_t)i];
    return TD_OK;
}

int td_token_bytes(const td_tokenizer* t, int32_t id, const uint8_t** bytes, int64_t* len) {
    if (!t) return TD_E_INVALID;
    const HostTables& H = t->H;
    if (id < 0 || id > H.max_id || H.tok_off[(size_t)id + 1] == H.tok_off[(size_t)id]) return TD_E_BAD_TOKEN;
    if (bytes) *bytes = H.tok_bytes.data() + H.tok_off[(size_t)id];
    if (len) *len = (int64_t)H.tok_off[(size_t)id + 1] - (int64_t)H.tok_off[(size_t)id];
    return TD_OK;
}

int td_single_token(const td_tokenizer* t, const uint8_t* bytes, int64_t len, int32_t* id) {
    if (!t || !bytes || len <= 0 || !id) return TD_E_INVALID;
    const HostTables& H = t->H;
    const Tables hv = H.view();
    int32_t r = NO_RANK;
    if (len == 1) {
        r = H.byte_id[bytes[0]];
        if (r >= H.pseudo_base) r = NO_RANK;
    } else if (len <= (int64_t)H.max_token_len) {
        r = piece_lookup(hv, piece_key_host(bytes, (uint32_t)len), (uint32_t)len, [bytes](uint32_t i) { return (uint32_t)bytes[i]; });
    }
    if (r == NO_RANK)
        for (size_t i = 0; i < H.special_ids.size(); ++i)
            if ((int64_t)H.special_strs[i].size() == len && memcmp(H.special_strs[i].data(), bytes, (size_t)len) == 0) { r = H.special_ids[i]; break; }
    if (r == NO_RANK) return TD_E_UNKNOWN_BYTE;
    *id = r;
    return TD_OK;
}

}  // extern "C"
