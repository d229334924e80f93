// What every translation unit of the host library (td_api*.cpp) needs of the handle: its owner types, the control block, the
// options, struct td_tokenizer itself and the helpers the areas share.  Private: not installed, no part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/tokendagger_hip.h"
#include "td_kernels.h"
#include "td_rewrite_args.h"
#include "td_tables.h"

namespace td {
// td_special.hip: what the host-buffer paths of td_encode_batch launch behind a step
hipError_t launch_mid_done(const void* ctl, uint32_t ctl_bytes, void* h_ctl, unsigned long long* h_seq, unsigned long long seq, hipStream_t stream);
hipError_t launch_pipe_copy_out(const void* src, void* dst, int64_t n_words, int blocks, hipStream_t stream);
hipError_t launch_pipe_publish(const void* ctl, uint32_t ctl_bytes, void* h_ctl, const int64_t* d_toff, int64_t n_off, int64_t* h_toff, hipStream_t stream);
}  // namespace td

#pragma GCC visibility push(hidden)  // (from here on: shared between the library's translation units, exported by none)
namespace td {

// Entry points switch to the handle's device for their own duration only: the caller's current HIP device (torch's,
// in a multi-GPU process) is what it was when the call returns, on every path, td_destroy from a finaliser included.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) switched = hipSetDevice(device) == hipSuccess;
    }
    ~DeviceGuard() {
        if (switched && prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

#define HIP_TRY(t, expr)                                                                      \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            (t)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                     \
            return TD_E_HIP;                                                                  \
        }                                                                                     \
    } while (0)

// Owners of the handle's HIP resources: each releases what it holds when it is destroyed or assigned another (move-only).
// A handle's members are therefore freed by `delete`; td_destroy makes that safe (see there).
template <hipError_t (*Free)(void*)>
struct Buf {  // device (DevBuf) or pinned host (PinnedBuf) memory of `cap` bytes
    void* p = nullptr;
    size_t cap = 0;
    Buf() = default;
    Buf(Buf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    Buf& operator=(Buf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }  // (o frees the old one)
    ~Buf() { if (p) (void)Free(p); }
};
using DevBuf = Buf<hipFree>;
using PinnedBuf = Buf<hipHostFree>;

template <class T, hipError_t (*Destroy)(T)>
struct Owned {  // a stream, an event or an executable graph
    T h = nullptr;
    Owned() = default;
    explicit Owned(T x) : h(x) {}
    Owned(Owned&& o) noexcept : h(o.h) { o.h = nullptr; }
    Owned& operator=(Owned&& o) noexcept { std::swap(h, o.h); return *this; }
    ~Owned() { if (h) (void)Destroy(h); }
    operator T() const { return h; }
};
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;
using GraphExec = Owned<hipGraphExec_t, hipGraphExecDestroy>;

// (each changes its owner only when it succeeds)
hipError_t make_stream(Stream& s);
hipError_t make_event(Event& ev);
hipError_t make_pinned(PinnedBuf& b, size_t bytes);

// Host threads that fill and drain the pinned bounce buffers of the td_encode_batch pipeline: a copy job is cut into
// segments that the workers take from one queue; copies into the pipeline and out of it run side by side.
class CopyPool {
public:
    struct Job { std::atomic<int> remaining{0}; };
    explicit CopyPool(int n) {
        for (int i = 0; i < n; ++i) workers_.emplace_back([this] { run(); });
    }
    ~CopyPool() {
        { std::lock_guard<std::mutex> g(mu_); stop_ = true; }
        cv_.notify_all();
        for (auto& w : workers_) w.join();
    }
    int size() const { return (int)workers_.size(); }
    std::shared_ptr<Job> copy(void* dst, const void* src, size_t bytes) {
        auto job = std::make_shared<Job>();
        if (bytes == 0) return job;
        const size_t seg = std::max<size_t>(1u << 20, ((bytes / (size_t)(2 * std::max(size(), 1))) + 4095) & ~(size_t)4095);
        int nseg = 0;
        for (size_t lo = 0; lo < bytes; lo += seg) ++nseg;
        job->remaining.store(nseg);
        {
            std::lock_guard<std::mutex> g(mu_);
            for (size_t lo = 0; lo < bytes; lo += seg) q_.push_back({(char*)dst + lo, (const char*)src + lo, std::min(seg, bytes - lo), job});
        }
        cv_.notify_all();
        return job;
    }
    void wait(const std::shared_ptr<Job>& job) {  // (the caller helps)
        while (job->remaining.load() > 0) {
            Seg sg;
            {
                std::unique_lock<std::mutex> g(mu_);
                if (q_.empty()) { done_.wait_for(g, std::chrono::microseconds(50)); continue; }
                sg = q_.front(); q_.pop_front();
            }
            memcpy(sg.dst, sg.src, sg.len);
            if (sg.job->remaining.fetch_sub(1) == 1) done_.notify_all();
        }
    }
private:
    struct Seg { char* dst; const char* src; size_t len; std::shared_ptr<Job> job; };
    void run() {
        for (;;) {
            Seg sg;
            {
                std::unique_lock<std::mutex> g(mu_);
                cv_.wait(g, [this] { return stop_ || !q_.empty(); });
                if (stop_ && q_.empty()) return;
                sg = q_.front(); q_.pop_front();
            }
            memcpy(sg.dst, sg.src, sg.len);
            if (sg.job->remaining.fetch_sub(1) == 1) done_.notify_all();
        }
    }
    std::vector<std::thread> workers_;
    std::mutex mu_;
    std::condition_variable cv_, done_;
    std::deque<Seg> q_;
    bool stop_ = false;
};

struct Ctl {  // small control block in device memory
    int err;
    int pad;
    long long err_pos;
    uint32_t long_count;   // --- from here on: reset before every call
    uint32_t slow_count;
    unsigned long long pool_used;
    uint32_t scan_done;
    uint32_t merge_next;   // td_merge_pieces: next tile nobody has taken yet
    uint32_t miss_count[6];  // entries on the miss lists (K_MISS_CLASSES of them)
    uint32_t flagged_count;  // tiles flagged TILE_HAS_MISS (on flagged_list: td_merge_pieces draws them from there)
    uint32_t gap_count;      // generic split patterns: stretches of text the pattern skipped
    uint32_t deferred_count; // fused tile loop: token tiles left to td_probe_tiles
    uint32_t giant_count;    // long pieces above 1 KiB
    uint32_t tile_draw;      // fused tile loop: tiles handed out beyond every workgroup's first two
    uint32_t direct_tiles;   // (statistics) pre-tokenizer tiles whose ids the fused loop wrote straight to the output
    uint32_t lb_timeouts;    // ... and tiles it staged because their base was not known in time (behind direct_tiles)
    uint32_t ovf_count;      // td_collect_misses: tiles with a length class that found its lists full
    uint32_t dd_stats[2];    // (statistics) repeats, pieces listed for the merge (td_copy_dups)
    uint32_t gp_ctl[4];      // td_giant_pieces over all workgroups: barrier arrivals, pieces listed, a barrier gave up, pieces above the limit
    uint32_t far_tiles;      // pre-tokenizer tiles without a synchronisation point in their left halo (td_split_far_tiles)
    uint32_t ph_bar;         // td_far_probe / td_tail: arrivals at their grid barriers
    uint32_t gs_done;        // td_giant_scan: workgroups that have left the giant pieces
    uint32_t lp_next;        // td_long_pieces: chunks of the long-piece list drawn so far
};
static_assert(K_MISS_CLASSES <= 6, "Ctl::miss_count");
constexpr size_t CTL_BYTES = 256;  // the control block's place in its buffer; behind it: td_giant_pieces' scratch (TD_GP_SCRATCH_BYTES)
static_assert(sizeof(Ctl) <= CTL_BYTES, "Ctl");

// What td_create builds and no call changes afterwards: the host tables and their copies in HBM (~30 MB for a 200 000-entry
// vocabulary).  Shared by the handles td_clone makes from one another; freed with the last of them.
struct SharedTables {
    HostTables H;
    std::vector<void*> table_allocs;
    int device = 0;
    ~SharedTables() {
        if (table_allocs.empty()) return;
        DeviceGuard dg(device);
        for (void* p : table_allocs) (void)hipFree(p);
    }
};

// What either text rewrite keeps on the device: the bad-offsets / full words, the tiles' output bytes and bases, flags where the caller
// has none; the host entry points' counts, rewritten text and its document offsets
struct RewriteBufs {
    DevBuf head, tiles, flags, counts, out, out_off;
};

// The tunables: td_create reads them from the environment (from_env), td_set_option changes most of them, td_clone copies them all.
struct Options {
    bool fused = true;            // pre-tokenizer and lookup in one pass over the text (TD_OPT_FUSED; TD_FUSED=0 turns it off)
    bool graphs = false;          // the last step as a hipGraph (encode_device_locked): opt-in (TD_OPT_GRAPH, TD_GRAPH=1)
    bool direct = false;          // the fused loop places a tile's ids itself when their output base is known in time (TD_OPT_DIRECT; TD_DIRECT)
    bool pack_split = true;       // td_pack_plain + td_pack_rest instead of td_pack_tokens (TD_OPT_PACK_SPLIT; TD_PACK_SPLIT=0 turns it off)
    bool dedupe = true;           // a missed piece whose bytes another one of the call has is merged once (TD_OPT_DEDUPE; TD_DEDUPE=0 turns it off)
    bool overlap = true;          // TD_OPT_OVERLAP (TD_OVERLAP=0 turns it off)
    bool mid_enabled = true;      // (TD_MID_PATH=0: the copies-and-synchronise path of rounds 1-5, A/B)
    bool small_enabled = true;    // TD_OPT_SMALL_PATH
    bool small_resident = false;  // (TD_SMALL_RESIDENT=1.  Built for VERDICT r5 item 5a, measured, OFF: 14.1 us against 13.6 for a one-byte call —
                                  // what a small call costs is the body's PCIe round trips and barriers, not the launch; tests/test_gpu_small_resident.py keeps it right)
    unsigned long long small_idle_ticks = 20000;  // (TD_SMALL_IDLE_US, default 200 us: 100 MHz ticks the resident kernel waits for the next request)
    int sparse_opt = -1;          // TD_OPT_SPARSE / TD_SPARSE: 1 = always the sparse sequence, 0 = never, -1 = by the last counters
    uint32_t gp_coop_min = 16384; // TD_OPT_GIANT_COOP_MIN (TD_GP_COOP_MIN): pieces above this many bytes get all workgroups of td_giant_pieces
    uint32_t dd_replicas = 4;     // (TD_DD_REPLICAS, tuning: a power of two)
    uint32_t dd_minlen = 2;       // (TD_DD_MINLEN, tuning: pieces below this many bytes are merged without a look at the table)
    uint32_t dd_entries_opt = 0;  // (TD_DD_ENTRIES=<power of two>, tests: seats of the table of distinct missed pieces)
    int coll_shrink = 1;          // (TD_COLL_SHRINK=<k>, tests: td_collect_misses' lists 1/k of their size)
    bool device_specials = true;  // host-buffer batches of a MiB and more search on the device (TD_OPT_DEVICE_SPECIALS)
    int64_t pool_bytes_opt = 0;   // TD_OPT_LONG_POOL_BYTES
    int64_t pipe_chunk_bytes = 64ll << 20;  // TD_OPT_PIPE_CHUNK_BYTES (a GiB of English host to host: 16 MiB chunks 33 GB/s, 32 MiB 39, 64 MiB 40.5, profiles/r5_bench/e2e_sweep.txt)
    int pipe_threads = 16;        // TD_OPT_PIPE_THREADS
    int counts_flush_tiles = 0;   // TD_OPT_COUNTS_FLUSH_TILES: tiles of a workgroup between two flushes of that table, 0 = CNT_FLUSH_TILES (tests shrink it)
    int counts_seat_bits = 0;     // TD_OPT_COUNTS_SEATS: log2 of the seats of td_cnt_tiles' on-chip table, 0 = the production size (tests force conflicts with 2)
    int ngram_tag_bits = 0;       // TD_OPT_NGRAM_TAG_BITS: hash bits td_ng_tiles compares before the ids, 0 = all 32 (tests force id compares with 1 to 4)
    int ws_fill = -1;             // TD_OPT_WS_FILL / TD_WS_FILL (debugging): -1 = off, 0..255 = the byte ensure() and every step fill the workspace with
    static Options from_env();
};

}  // namespace td
using namespace td;

struct td_tokenizer {
    std::shared_ptr<SharedTables> shared;
    HostTables& H;                           // = shared->H
    Tables dT;  // device pointers
    const Tables* dTp = nullptr;  // the same descriptor, in device memory
    int device = 0;
    std::vector<void*>& table_allocs;        // = shared->table_allocs (filled by td_create only)
    explicit td_tokenizer(std::shared_ptr<SharedTables> s = std::make_shared<SharedTables>())
        : shared(std::move(s)), H(shared->H), table_allocs(shared->table_allocs) {}
    std::string err;
    std::mutex mu;
    Options opt;
    bool profile = false;   // (TD_OPT_PROFILE; neither it nor stop_after is handed on by td_clone)
    int stop_after = 0;
    // workspace (grown on demand)
    DevBuf dd_table, rest_mask, coll_ctr, tile_state, slab, docbits, startbits, slow_list, tile_flag, tile_carry, stage, stage2, tile_count, tile_extra, miss_list, flagged_list, deferred_list, gap_list, gapbits, gx_exit, gx_state, tile_base, doc_slot, long_list, pool, ctl, tile_first_doc, chunk_pref;
    DevBuf h2d_text, h2d_offs, d_tokens, d_offsets;  // host-API staging
    DevBuf dec_tokens, dec_off, dec_out;
    // per-token starts (td_offsets.hip): the per-id character table (td_create, shared like the other tables) and the scratch
    const uint32_t* d_ctab = nullptr;
    DevBuf off_heads, off_chunks, off_docs, off_rank, off_starts;
    // training rows (td_rows.hip): the cu_seqlens scan's status words, the host entry points' outputs on the device
    DevBuf rows_scan, rows_out, rows_pos, rows_aux, rows_counts;
    DevBuf rows_lab_src, rows_lab;  // the labeled host entry points: the caller's label stream, the label rows
    // window rows (td_windows.hip): the scan words and first_row, the host entry points' per-row outputs on the device
    DevBuf win_scan, win_first, win_len, win_docs, win_starts;
    // document selection (td_select.hip): the scan words and src_base, the host entry points' list, offsets and documents on the device
    DevBuf sel_scan, sel_base, sel_in, sel_off, sel_docs;
    // field joins (td_join.hip): the scan words and the plan records, the host entry points' offsets, examples, field lengths and
    // types on the device (their ids and labels: rows_out, rows_lab)
    DevBuf join_scan, join_plan, join_off, join_ex, join_flen, join_types;
    bool rows_last = false;  // the last call launched the rows kernels (the unit of a TD_E_CAPACITY position)
    // loss labels (td_labels.hip): the counts and flags, the document-start bitmap, the tiles' events / states, their trained ids
    // and the lanes' (trained_offsets only); the host entry points' outputs on the device
    DevBuf lab_head, lab_bits, lab_tiles, lab_cnt, lab_aux, lab_out, lab_mask, lab_toff, lab_counts;
    // loss labels from byte ranges (td_ranges.hip; the rest of its scratch is the labels'): the first-range bitmap, the ranges' marked
    // bytes in front of them inside their chunk and the chunks', the carries into the tiles; the host entry points' range offsets,
    // ranges, starts and text offsets on the device
    DevBuf rng_bits, rng_cum, rng_chunks, rng_sums, rng_off, rng_ranges, rng_starts, rng_docs;
    // token counts (td_counts.hip): the host entry points' counts, info and document groups on the device
    DevBuf cnt_counts, cnt_info, cnt_groups;
    // decode rows (td_decode_rows.hip): the per-id table (with the listed ids above max_id behind it) and what it was built for, the
    // tiles' aggregates and bases; the host entry point's offsets, lengths, byte offsets, segment ids and info on the device
    DevBuf dcr_table, dcr_tiles, dcr_off, dcr_len, dcr_out_off, dcr_seg_ids, dcr_info;
    // n-gram matches (td_ngrams.hip): the bad-offsets word, doc_stats where the caller has none; the host entry points' cover, labels,
    // doc_stats, pattern counts and counts on the device
    DevBuf ng_head, ng_stats, ng_cover, ng_labels, ng_doc_stats, ng_pats, ng_counts;
    // MinHash signatures (td_minhash.hip): the bad-offsets word and the document counts, the permutation table and what it was built
    // for; the host entry points' signatures, band keys and counts on the device
    DevBuf mh_head, mh_table, mh_sig, mh_keys, mh_counts;
    // The text rewrites, NFC normalisation (td_nfc.hip) and UTF-8 validation and repair (td_utf8.hip): each one's RewriteBufs; changed
    // where the caller has none; a byte a window for the documents' edges, the host entry points' first_bad and n_bad on the device
    RewriteBufs nfc, utf8;
    DevBuf nfc_changed, utf8_dirty, utf8_first, utf8_nbad;
    // text statistics (td_textstats.hip): the bad-offsets word (its RewriteBufs' head alone), four last positions a tile; the host entry
    // points' stats and totals on the device
    RewriteBufs textstats;
    DevBuf ts_carry, ts_stats, ts_totals;
    int64_t mh_table_perm = 0;     // 0: no table yet
    uint64_t mh_table_seed = 0;
    std::vector<int64_t> dcr_key;  // flags, then the distinct listed ids with their bits (sorted); empty: no table yet
    // best-fit packing (td_pack.hip): the items, the sort's and the scan's scratch, the header + runs read back, the plan uploaded,
    // the segments; the host entry points' row lengths and segment documents on the device
    DevBuf pack_key, pack_val, pack_key2, pack_val2, pack_full, pack_pref, pack_tmp, pack_hdr, pack_plan, pack_seg, pack_len, pack_docs;
    PinnedBuf pack_h, pack_up;
    // The library never touches the legacy (null) stream on its own: a legacy-stream operation is illegal while ANY thread of
    // the process captures a blocking stream, and synchronises with every blocking stream of every other thread.  Copies the
    // host waits for, table uploads and the host-buffer entry points run on `s_own` (non-blocking, private to the handle);
    // small results come back through `h_ctl` (pinned).
    Stream s_own;
    Stream s_aux;                      // the long pieces beside the short ones (LaunchAux, td_kernels.h); with its two events
    Event e_fork, e_join;
    Stream s_cap;                      // hipGraph capture only (non-blocking: the CALLER's stream is never put into capture)
    PinnedBuf h_ctl;                   // 256 B: the control block / an 8-byte total on their way to the host
    // the last step as a hipGraph (encode_device_locked): opt-in (Options::graphs)
    int graph_failures = 0;
    GraphExec graph_exec;
    EncodeArgs graph_key, last_key;
    hipStream_t graph_stream = nullptr, last_key_stream = nullptr;
    bool has_last_key = false;
    // allowed special tokens on the device (td_encode_device_with_special): the sorted literal table of the last allowed set
    std::vector<int32_t> sp_key;     // the allowed ids it was built for (sorted, unique)
    DevBuf sp_bytes, sp_off, sp_len, sp_id, sp_parent, sp_first2, sp_hit, sp_acc, sp_cpos, sp_clit, sp_ccount;
    uint32_t sp_n = 0, sp_maxlen = 0;
    bool sp_active = false;          // this call cuts allowed specials (set around encode_device_locked)
    bool enc_keep_resident = false;  // (set around encode_special_strs_locked) ids that stay in d_tokens are not copied to the host as well
    bool enc_resident = false;       // the last encode_special_strs_locked left the ids and offsets it returned in d_tokens / d_offsets too
    // generic patterns with left-context assertions behind special cuts: per document of the NEXT host batch, the bytes at its
    // start that are context only (set around encode_batch_locked by encode_special_locked)
    const uint8_t* gx_prefix_host = nullptr;
    DevBuf gx_prefix;
    const uint8_t* gx_prefix_dev = nullptr;
    struct Ev3 {  // the profiling events of one step (owned: hipEventDestroy when it goes)
        hipEvent_t e[TD_PROF_EVENTS] = {};
        Ev3() = default;
        Ev3(Ev3&& o) noexcept { std::swap(e, o.e); }
        Ev3& operator=(Ev3&& o) noexcept { std::swap(e, o.e); return *this; }
        ~Ev3() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    };
    std::vector<Ev3> ev_pending, ev_free;
    int64_t last_repeats = 0, last_listed = 0;
    int64_t last_long = 0, last_far = 0, last_deferred = 0, last_flagged = 0, last_direct = 0, last_timeouts = 0;
    int64_t last_giant = 0;
    bool seen_counters = false;   // td_device_status / a host-buffer entry point has read a call's counters (what the launch sequence is chosen by)
    bool last_sparse = false;     // (TD_INFO_SPARSE)
    const RxProgram* d_rx = nullptr;      // generic split pattern: the compiled program and its tables in HBM
    const uint16_t* d_rx_s1 = nullptr;
    const uint8_t* d_rx_s2 = nullptr;
    size_t ws_bytes = 0;
    int64_t ws_filled = 0;        // TD_INFO_WS_FILLED_BYTES: what ensure() and the steps have filled (Options::ws_fill)
    // One workspace per handle: work of this handle may be in flight on one stream at a time.  A call on another
    // stream first waits (on the device, not the host) for the previous call's last kernel.
    Event last_done;
    hipStream_t last_stream = nullptr;
    bool has_last = false;
    std::vector<DevBuf> graveyard;  // workspace buffers replaced by larger ones; freed at the next synchronisation point
    // host-buffer pipeline (td_encode_batch on large inputs): four slots of pinned bounce buffers + device buffers, three
    // streams (H2D, kernels, D2H)
    struct PipeSlot {
        PinnedBuf h_text, h_offs, h_tok;   // h_offs: rebased document offsets in, token offsets out
        DevBuf d_text, d_offs, d_tok, d_toff;
        Event ev_h2d, ev_k, ev_off, ev_tok;
        PinnedBuf h_ctl;                   // copy of the device control block after the chunk's kernels
    };
    static constexpr int PIPE_SLOTS = 4;
    PipeSlot pipe[PIPE_SLOTS];
    Stream s_h2d, s_k, s_d2h;
    std::unique_ptr<CopyPool> pool_threads;
    // one-launch path for inputs of at most 4 KiB: pinned host buffers the kernel reads and writes directly
    PinnedBuf small_in, small_out;
    PinnedBuf small_dec_in, small_dec_out;  // td_small_decode: ids in, status + bytes out
    unsigned long long small_seq = 0;
    // which path answered, since the handle was made (TD_INFO_SMALL_*; td_clone's handle starts at 0): calls the one-launch kernels
    // answered themselves (an error they reported included) and calls they handed back to the general path
    int64_t small_encodes = 0, small_encode_handbacks = 0, small_decodes = 0, small_decode_handbacks = 0;
    // the resident form of the one-launch kernel (td_small_resident): its own stream, the generation of the last launch
    Stream s_res;
    unsigned long long res_gen = 0;
    // host batches between the one-launch path and the pipeline (td_encode_batch, 4 KiB .. 4 MiB): pinned in / out buffers
    PinnedBuf mid_in, mid_out;
    DevBuf mid_dev;               // [offsets | text] on the device
    unsigned long long mid_seq = 0;
};

namespace td {

// ---- defined in td_api.cpp ----------------------------------------------------------------------------------------------------------
int ensure(td_tokenizer* t, DevBuf& b, size_t bytes);           // grows a workspace buffer; the old one is parked (graveyard)
int pinned_ensure(td_tokenizer* t, PinnedBuf& b, size_t bytes);  // grows a pinned buffer (only after a synchronisation: nothing reads the old one)
int own_streams(td_tokenizer* t);
int copy_wait(td_tokenizer* t, void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s);
int zero_wait(td_tokenizer* t, void* dst, size_t bytes, hipStream_t s);
void drain(td_tokenizer* t);
// rc, with msg as what td_last_error(t) gives this thread (the slots are td_api.cpp's own): an argument error found before taking the lock
int fail_unlocked(td_tokenizer* t, int rc, const std::string& msg);
int order_before(td_tokenizer* t, hipStream_t stream);
int order_after(td_tokenizer* t, hipStream_t stream);
int check_offsets(td_tokenizer* t, const char* what, const int64_t* offs, int64_t n_docs, const void* payload);
// Spins (acquire loads) until *seqp == seq; every spin_mask + 1 spins it looks at the clock, and after limit_s seconds it synchronises
// s (a launch failure surfaces there), looks once more and fails with TD_E_HIP and `what`.
int wait_for_seq(td_tokenizer* t, const volatile unsigned long long* seqp, unsigned long long seq, hipStream_t s, uint32_t spin_mask,
                 int limit_s, const char* what);
int encode_device_locked(td_tokenizer* t, const void* d_text, int64_t n, const void* d_offs, int64_t n_docs, int mode, void* d_out,
                         int64_t out_cap, void* d_out_offs, hipStream_t stream);
int absorb_ctl(td_tokenizer* t, Ctl c, hipStream_t stream, int64_t* err_pos);
int device_status_locked(td_tokenizer* t, hipStream_t stream, int64_t* err_pos);
int encode_batch_locked(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode, int32_t* out_tokens,
                        int64_t out_capacity, int64_t* out_offsets, int64_t* n_tokens, int unit = TD_UNIT_BYTES, int64_t* out_starts = nullptr);
// ---- defined in td_api_special.cpp --------------------------------------------------------------------------------------------------
// td_encode_batch_with_special_strs under the caller's lock; sets t->enc_resident.
int encode_special_strs_locked(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, const uint8_t* allowed_bytes,
                               const int64_t* allowed_offsets, int64_t n_allowed, int32_t* out_tokens, int64_t out_capacity,
                               int64_t* out_offsets, int64_t* n_tokens);
// ---- defined in td_api_rows.cpp -----------------------------------------------------------------------------------------------------
// The checks of a caller's host ids and offsets (nothing allocated, nothing enqueued), and their upload into dec_tokens / d_offsets
// on the handle's own stream, which `s` becomes.
int rows_check_host_ids(td_tokenizer* t, const int32_t* ids, int64_t n_tokens, const int64_t* tok_offsets, int64_t n_docs);
int rows_stage_host_ids(td_tokenizer* t, const int32_t* ids, const int64_t* tok_offsets, int64_t n_docs, hipStream_t& s);
// td_encode_batch_span_label_rows: the checks of its row arguments (before the lock), and the labeled row call of sp->layout on ids
// and labels already on the device with their offsets (h_toff: the same on the host), into the caller's host outputs.
int label_rows_check(td_tokenizer* t, const char* fn, const td_rows_spec* sp, int64_t overlap, int64_t n_docs, const td_rows_labels* lab,
                     const td_label_rows_outputs* o, int64_t rows_capacity);
int label_rows_to_host(td_tokenizer* t, const void* d_ids, const void* d_src, const void* d_toff, const int64_t* h_toff, int64_t n_docs,
                       const td_rows_spec* sp, int64_t overlap, const td_rows_labels* lab, const td_label_rows_outputs& o,
                       int64_t rows_capacity, int64_t* counts, hipStream_t s);
// td_encode_batch_rows, _pack_rows, _window_rows, _select, _token_counts: the documents encoded on the handle's own stream, which `s`
// becomes, into d_tokens (room for dev_cap ids) / d_offsets; the encode's errors are returned as such before anything reads its ids.
int rows_encode_locked(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, int mode, int64_t& dev_cap,
                       hipStream_t& s);
// ---- defined in td_api_rewrite.cpp: what the text rewrites' entry points (td_api_nfc.cpp, td_api_utf8.cpp) share -------------------------
// The host forms' start (rows_encode_locked's too): the checks of the caller's text and offsets, and their upload into h2d_text /
// h2d_offs on the handle's own stream, which `s` becomes.
int stage_host_text(td_tokenizer* t, const uint8_t* text, const int64_t* doc_offsets, int64_t n_docs, hipStream_t& s);
// One launch sequence of a pass on `s`.  `a` is the pass's arguments, zeroed but for what the pass adds; the text, the offsets, the flags
// and the counts of c go into it with w's head and where errors are raised.  rewrite_check_locked (launch_*_check: c's outputs are not
// looked at) zeroes the head on `s`; rewrite_locked (launch_nfc / launch_utf8 with `phases`) zeroes it in front of a measure phase and
// adds c's outputs, w's tiles and, where c has no flags, w's.  launch() enqueues the pass's kernels.
struct RewriteCall {
    const void* d_text;
    int64_t n_bytes;
    const void* d_off;
    int64_t n_docs;
    void *d_flags, *d_counts, *d_out;
    int64_t out_capacity;
    void* d_out_off;
};
int rewrite_check_locked(td_tokenizer* t, RewriteBufs& w, RewriteArgs& a, const RewriteCall& c, hipStream_t s, const std::function<int()>& launch);
int rewrite_locked(td_tokenizer* t, RewriteBufs& w, RewriteArgs& a, const RewriteCall& c, int phases, hipStream_t s, const std::function<int()>& launch);
// check(): the pass's check of h2d_text / h2d_offs into w.flags and w.counts (both grown here); then the status, and w.counts to `counts`.
int rewrite_check_staged(td_tokenizer* t, RewriteBufs& w, int64_t n_docs, int64_t* counts, hipStream_t s, const std::function<int()>& check);
// run(d_out, out_capacity, phases): the pass's phases on h2d_text / h2d_offs (n bytes) into w.flags, w.counts, w.out_off and its own
// per-document buffers.  Measured first, w.counts comes back in `counts`; where `write` is set, then written into w.out / w.out_off.
// w.out is sized from counts[0], the bytes the text needs, not from the 3 x bound, which `what`'s total is held to.
int rewrite_staged(td_tokenizer* t, RewriteBufs& w, int64_t n, int64_t n_docs, int64_t* counts, bool write, const char* what, hipStream_t s,
                   const std::function<int(void* d_out, int64_t out_capacity, int phases)>& run);
// The end of td_encode_batch_nfc / _utf8: the rewritten text d_text (the caller's own `text` where it is still h2d_text) of n_enc bytes
// to out_text where there is one, its encode with d_off into d_tokens / d_offsets, the status, then the offsets and the ids.
int encode_rewritten(td_tokenizer* t, const uint8_t* text, const void* d_text, const void* d_off, int64_t n_enc, int64_t n_docs, int mode,
                     const char* text_name, uint8_t* out_text, int64_t text_capacity, int32_t* out_ids, int64_t ids_capacity,
                     int64_t* out_tok_offsets, hipStream_t s);
// ---- defined in td_api_labels.cpp ---------------------------------------------------------------------------------------------------
int labels_outputs_to_host(td_tokenizer* t, int64_t total, int64_t n_docs, int32_t* labels, uint8_t* mask, int64_t* trained_offsets,
                           int64_t* counts, hipStream_t s, const std::function<int(void*, void*, void*, void*)>& launch);
int encode_starts_locked(td_tokenizer* t, const void* d_text, int64_t n, const void* d_offs, int64_t n_docs, const void* d_tokens, int64_t cap,
                         const void* d_out_offs, int unit, void* d_starts, hipStream_t stream);

// The end of every host-buffer encode: the total to the caller, the capacity, the output pointer, then copy() brings the ids.
template <class F>
int deliver_ids(td_tokenizer* t, int64_t total, int64_t out_capacity, const int32_t* out_tokens, int64_t* n_tokens, F&& copy) {
    if (n_tokens) *n_tokens = total;
    if (total > out_capacity) {
        t->err = "output capacity too small: " + std::to_string(total) + " tokens needed";
        return TD_E_CAPACITY;
    }
    if (total == 0) return TD_OK;
    if (!out_tokens) { t->err = "null out_tokens"; return TD_E_INVALID; }
    return copy();
}

// Runs f() with the handle locked and its device current; a failure's message is published to this thread's slot.
template <class F>
int locked(td_tokenizer* t, F&& f) {
    std::lock_guard<std::mutex> g(t->mu);
    DeviceGuard dg(t->device);
    const int rc = f();
    return rc == TD_OK ? rc : fail_unlocked(t, rc, t->err);
}

}  // namespace td
#pragma GCC visibility pop
