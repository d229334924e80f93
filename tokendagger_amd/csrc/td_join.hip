// Field joins (td_join_fields*, td_encode_batch_join): ids + per-document token offsets, K documents (fields) an example -> the
// kept examples, each one output document: before_0 body_0 ... before_{K-1} body_{K-1} tail, with its labels and types.  The
// output is again ids + tok_offsets.  The shape is td_select.hip's, "scan, then gather by tiles":
//
//   td_join_count   1024 examples a workgroup: the K documents' offsets checked against each other and n_tokens, the kept lengths
//                   c_f by the shared rule (join_keep, td_join_args.h); the chunk's kept examples and kept slots into the scan
//                   words, the dropped and the truncated examples by one atomic a workgroup and kind
//   td_join_chunks  one workgroup: the chunks' sums -> their exclusive prefixes (chunks_excl_scan<2>); E, T, the capacity check,
//                   counts, and the "leave" mark (a bad example, or T above the capacity) the two kernels behind it read
//   td_join_first   kept example -> k: out_off[k], out_examples[k], out_field_len, and its plan record: the starts of its 2K + 1
//                   parts inside it and the source index of each body's first kept id; the slot kernel never redoes the truncation
//   td_join_slots   the slots.  Tiles of 4096 OUTPUT slots, four a lane stored as one int4.  Slot j belongs to the k with
//                   out_off[k] <= j < out_off[k + 1] (group_last_le, tile_table, last_le; last_le_global for a tile made of
//                   thousands of empty examples), and inside it to the last part that starts at or below it: a count over the
//                   record's at most 17 starts.  Four slots inside one body with their source in range are one rows_get4; anything
//                   else goes slot by slot, literals from the kernel's arguments.  Ids, labels and types are stored in the same
//                   pass; <LAB, TYP>: the streams the caller asked for.  No lane waits for another workgroup.
#include <hip/hip_runtime.h>

#include "td_join.h"
#include "td_rows_common.h"

namespace td {

namespace {

constexpr int JOIN_THREADS = RC_THREADS, JOIN_TILE = RC_TILE, JOIN_MAX_GRID = RC_MAX_GRID;

struct JoinEntry {
    int64_t lo[JOIN_MAX_FIELDS], c[JOIN_MAX_FIELDS], L[JOIN_MAX_FIELDS];
    int64_t slots;  // fixed + sum c_f
    bool bad, keep, truncated;
};

// Example x: nothing outside tok_off[0, n_ex * K] is read.
__device__ __forceinline__ void join_entry(const JoinArgs& a, int64_t x, JoinEntry& e) {
    e.bad = e.keep = e.truncated = false;
    e.slots = 0;
#pragma unroll
    for (int f = 0; f < JOIN_MAX_FIELDS; ++f) {
        e.lo[f] = e.L[f] = e.c[f] = 0;
        if (f >= a.rule.K) continue;
        const int64_t d = join_doc(a.rule, a.n_ex, x, f);
        const int64_t lo = a.tok_off[d], hi = a.tok_off[d + 1];
        if (lo < 0 || hi < lo || hi > a.n_tokens) e.bad = true;
        e.lo[f] = lo;
        e.L[f] = hi - lo;
    }
    if (e.bad) return;
    const int st = join_keep(a.rule, e.L, e.c);
    e.keep = st != JOIN_DROPPED;
    e.truncated = st == JOIN_TRUNCATED;
    e.slots = a.rule.fixed;
#pragma unroll
    for (int f = 0; f < JOIN_MAX_FIELDS; ++f)
        if (f < a.rule.K) e.slots += e.c[f];
}

__global__ __launch_bounds__(JOIN_THREADS) void td_join_count(const JoinArgs a) {
    __shared__ long long s_red[JOIN_THREADS / 64];
    const int tid = threadIdx.x;
    long long kept = 0, kept_slots = 0, n_drop = 0, n_trunc = 0, n_bad = 0;
    int64_t bad_at = 0;
    for (int q = 0; q < 4; ++q) {
        const int64_t x = (int64_t)blockIdx.x * RC_SCAN_CHUNK + tid * 4 + q;
        if (x >= a.n_ex) break;
        JoinEntry e;
        join_entry(a, x, e);
        if (e.bad && !n_bad) bad_at = x;
        n_bad += e.bad;
        kept += e.keep;
        kept_slots += e.keep ? e.slots : 0;
        n_drop += !e.bad && !e.keep;
        n_trunc += e.keep && e.truncated;
    }
    if (n_bad) rows_raise(a, TD_E_INVALID, bad_at);
    kept = block_sum(kept, s_red);
    kept_slots = block_sum(kept_slots, s_red);
    n_drop = block_sum(n_drop, s_red);
    n_trunc = block_sum(n_trunc, s_red);
    n_bad = block_sum(n_bad, s_red);
    if (tid == 0) {
        a.scan[JOIN_SCAN_HEAD + 2 * (int64_t)blockIdx.x] = (unsigned long long)kept;
        a.scan[JOIN_SCAN_HEAD + 2 * (int64_t)blockIdx.x + 1] = (unsigned long long)kept_slots;
        if (n_drop) atomicAdd(&a.scan[JOIN_N_DROPPED], (unsigned long long)n_drop);
        if (n_trunc) atomicAdd(&a.scan[JOIN_N_TRUNC], (unsigned long long)n_trunc);
        if (n_bad) atomicAdd(&a.scan[JOIN_BAD], 1ull);
    }
}

__global__ __launch_bounds__(JOIN_THREADS) void td_join_chunks(const JoinArgs a, int64_t nch) {
    __shared__ long long s_wave[JOIN_THREADS / 64];
    const int tid = threadIdx.x;
    long long carry[2];  // kept examples, kept slots
    chunks_excl_scan<2>(a.scan + JOIN_SCAN_HEAD, nch, s_wave, carry);
    if (tid == 0) {
        const long long carry_e = carry[0], carry_t = carry[1];
        const bool bad = a.scan[JOIN_BAD] != 0;
        const bool fits = !bad && carry_t <= a.ids_cap;
        if (!bad && !fits) rows_raise(a, TD_E_CAPACITY, carry_t);
        a.scan[JOIN_LEAVE] = fits ? 0ull : 1ull;
        a.scan[JOIN_E] = (unsigned long long)carry_e;
        a.scan[JOIN_T] = (unsigned long long)carry_t;
        a.counts[0] = bad ? 0 : carry_e;
        a.counts[1] = bad ? 0 : carry_t;
        a.counts[2] = bad ? 0 : (long long)a.scan[JOIN_N_DROPPED];
        a.counts[3] = bad ? 0 : (long long)a.scan[JOIN_N_TRUNC];
    }
}

__global__ __launch_bounds__(JOIN_THREADS) void td_join_first(const JoinArgs a) {
    __shared__ long long s_wave[JOIN_THREADS / 64];
    if (a.scan[JOIN_LEAVE]) return;  // (every example is valid behind this line)
    const int tid = threadIdx.x;
    const int K = a.rule.K;
    const int64_t words = join_plan_words(K);
    long long sum_e = 0, sum_t = 0;
    for (int q = 0; q < 4; ++q) {
        const int64_t x = (int64_t)blockIdx.x * RC_SCAN_CHUNK + tid * 4 + q;
        if (x >= a.n_ex) break;
        JoinEntry e;
        join_entry(a, x, e);
        sum_e += e.keep;
        sum_t += e.keep ? e.slots : 0;
    }
    long long total;
    long long k = (long long)a.scan[JOIN_SCAN_HEAD + 2 * (int64_t)blockIdx.x] + block_excl(sum_e, s_wave, total);
    long long off = (long long)a.scan[JOIN_SCAN_HEAD + 2 * (int64_t)blockIdx.x + 1] + block_excl(sum_t, s_wave, total);
    // (the examples once more, one at a time: four entries of 24 lengths each kept across the scan would not stay in registers)
    for (int q = 0; q < 4; ++q) {
        const int64_t x = (int64_t)blockIdx.x * RC_SCAN_CHUNK + tid * 4 + q;
        if (x >= a.n_ex) break;
        JoinEntry e;
        join_entry(a, x, e);
        if (!e.keep) continue;
        a.out_off[k] = off;
        if (a.out_examples) a.out_examples[k] = x;
        int64_t* rec = a.plan + k * words;
        int64_t at = 0;
#pragma unroll
        for (int f = 0; f < JOIN_MAX_FIELDS; ++f) {
            if (f >= K) continue;
            rec[2 * f] = at;
            at += a.rule.n_before[f];
            rec[2 * f + 1] = at;
            at += e.c[f];
            rec[2 * K + 1 + f] = e.lo[f] + ((a.rule.keep_tail >> f) & 1 ? e.L[f] - e.c[f] : 0);
            if (a.out_field_len) a.out_field_len[k * K + f] = e.c[f] > INT32_MAX ? INT32_MAX : (int32_t)e.c[f];
        }
        rec[2 * K] = at;
        ++k;
        off += e.slots;
    }
    if (blockIdx.x == 0 && tid == 0) a.out_off[a.scan[JOIN_E]] = (int64_t)a.scan[JOIN_T];
}

template <bool LAB, bool TYP>
__global__ __launch_bounds__(JOIN_THREADS) void td_join_slots(const JoinArgs a) {
    constexpr int ITERS = JOIN_TILE / (4 * JOIN_THREADS);
    __shared__ int32_t s_off[RC_LDS_DOCS];  // out_off[k0 + i] - s0, clamped to [0, JOIN_TILE + 1]
    const int tid = threadIdx.x;
    if (a.scan[JOIN_LEAVE]) return;
    const int64_t E = (int64_t)a.scan[JOIN_E], T = (int64_t)a.scan[JOIN_T];
    const int64_t ntiles = (T + JOIN_TILE - 1) / JOIN_TILE;
    const int nparts = 2 * a.rule.K + 1;
    const int64_t words = join_plan_words(a.rule.K);
    const auto off_of = [off = a.out_off](int64_t k) { return off[k]; };
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t s0 = tile * JOIN_TILE;
        const int64_t s1 = s0 + JOIN_TILE < T ? s0 + JOIN_TILE : T;
        const int32_t span = (int32_t)(s1 - s0);
        __syncthreads();  // (the previous tile's readers of s_off are done)
        // k0: the example of slot s0 (out_off[0] = 0 <= s0 < T = out_off[E])
        const int64_t k0 = group_last_le(off_of, 0, E, s0);
        bool lds;
        // examples [k0, k0 + nk) begin below s1 (out_off[E] = T >= s1 does not); in LDS: s_off[0, nk], the last the end of them all
        int64_t nk = tile_table(s_off, off_of, k0, E, s0, 0, JOIN_TILE + 1, span, lds);
        if (!lds) nk = group_last_le(off_of, k0, E, s1 - 1) - k0 + 1;
        // i: the last of the tile's examples that begins at or below slot j
        auto find = [&](int64_t j) -> int64_t {
            if (lds) return last_le(s_off, nk, (int32_t)(j - s0));
            return last_le_global([off = a.out_off + k0](int64_t i) { return off[i]; }, 0, nk, j);
        };
        int32_t v[ITERS][4] = {};
        [[maybe_unused]] int32_t lv[ITERS][4] = {};
        [[maybe_unused]] int32_t tv[ITERS][4] = {};
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
            const int64_t j0 = s0 + (int64_t)it * 4 * JOIN_THREADS + 4 * tid;
            if (j0 < s1) {
                int64_t pstart = 0, pend = 0, base = 0;  // the part's slots [pstart, pend), a body's first kept id
                int part = 0;
                // the part of slot j: the last of its example's parts that starts at or below it (empty parts share their start with
                // the next one and are stepped over)
                auto resolve = [&](int64_t j) {
                    const int64_t k = k0 + find(j);
                    const int64_t start = a.out_off[k], end = a.out_off[k + 1];
                    const int64_t* rec = a.plan + k * words;
                    const int64_t rel = j - start;
                    // (the count, then three loads that wait for it: one sweep that selects the part's start, end and source from
                    // loads known from k alone, 3K + 2 of them, measured 5 % slower at K = 2: DESIGN 4.19)
                    int p = 0;
                    for (int q = 1; q < nparts; ++q) p += rec[q] <= rel;
                    part = p;
                    pstart = start + rec[p];
                    pend = p + 1 < nparts ? start + rec[p + 1] : end;
                    base = (p & 1) ? rec[nparts + (p >> 1)] : 0;
                };
                auto put = [&](int q, int32_t id) {
                    v[it][q] = id;
                    if constexpr (LAB) lv[it][q] = (a.train >> part) & 1 ? id : a.ignore_index;
                    if constexpr (TYP) tv[it][q] = a.type_of[part >> 1];
                };
                resolve(j0);
                const int64_t src = base + (j0 - pstart);
                if ((part & 1) && j0 + 4 <= pend && j0 + 4 <= s1 && src >= 0 && src + 4 <= a.n_tokens) {
                    int32_t w[4];
                    rows_get4(a.ids, src, w);
#pragma unroll
                    for (int q = 0; q < 4; ++q) put(q, w[q]);
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int64_t j = j0 + q;
                        if (j < s1) {
                            if (j >= pend) resolve(j);
                            const int64_t r = j - pstart;
                            if (part & 1) {
                                const int64_t sq = base + r;
                                if (sq >= 0 && sq < a.n_tokens) put(q, a.ids[sq]);  // (checked offsets give nothing else: a second fence)
                            } else if (r >= 0 && r < JOIN_MAX_LITERAL) {
                                put(q, a.lit[part >> 1][r]);
                            }
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
            const int64_t j0 = s0 + (int64_t)it * 4 * JOIN_THREADS + 4 * tid;
            if (j0 < s1) {
                rows_put4(a.out, j0, s1, v[it]);
                if constexpr (LAB) rows_put4(a.out_labels, j0, s1, lv[it]);
                if constexpr (TYP) rows_put4(a.out_types, j0, s1, tv[it]);
            }
        }
    }
}

}  // namespace

int64_t join_scan_words(int64_t n_ex) { return JOIN_SCAN_HEAD + 2 * (n_ex > 0 ? (n_ex + RC_SCAN_CHUNK - 1) / RC_SCAN_CHUNK : 1); }

hipError_t launch_join(const JoinArgs& a, hipStream_t stream) {
    const int64_t nch = (join_scan_words(a.n_ex) - JOIN_SCAN_HEAD) / 2;
    hipLaunchKernelGGL(td_join_count, dim3((unsigned)nch), dim3(JOIN_THREADS), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(td_join_chunks, dim3(1), dim3(JOIN_THREADS), 0, stream, a, nch);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(td_join_first, dim3((unsigned)nch), dim3(JOIN_THREADS), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const int64_t tiles = a.ids_cap / JOIN_TILE + 1;
    const int grid = (int)(tiles < JOIN_MAX_GRID ? tiles : JOIN_MAX_GRID);
    const bool lab = a.out_labels != nullptr, typ = a.out_types != nullptr;
    if (lab && typ) hipLaunchKernelGGL((td_join_slots<true, true>), dim3(grid), dim3(JOIN_THREADS), 0, stream, a);
    else if (lab) hipLaunchKernelGGL((td_join_slots<true, false>), dim3(grid), dim3(JOIN_THREADS), 0, stream, a);
    else if (typ) hipLaunchKernelGGL((td_join_slots<false, true>), dim3(grid), dim3(JOIN_THREADS), 0, stream, a);
    else hipLaunchKernelGGL((td_join_slots<false, false>), dim3(grid), dim3(JOIN_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace td
