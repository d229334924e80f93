// Document selection (td_select_docs*, td_encode_batch_select): ids + per-document token offsets + sel[n_sel] document indices
// -> the ids of the listed documents in the list's order, their offsets and their documents; entries whose document has fewer
// than min_len or more than max_len ids are dropped.  A gather: the output is again ids + tok_offsets.
//
// Entry i contributes keep_i documents and keep_i * L ids, and its place in the output is the exclusive prefix sum of both: no
// closed form, nothing sequential.  Three small launches make out_offsets, out_docs and src_base, no lane waits for another
// workgroup in any of them; the chunk scan and the tile locator are td_rows_common.h's, shared with td_windows.hip:
//
//   td_sel_count    1024 entries a workgroup: sel[i] (or i) checked against n_docs, its two offsets against each other and
//                   n_tokens, keep and keep * L; the chunk's two sums into the scan words, the dropped entries by one atomic
//                   a workgroup and kind
//   td_sel_chunks   one workgroup: the chunks' sums -> their exclusive prefixes (chunks_excl_scan<2>); K, T, the capacity check,
//                   counts, and the "leave" mark (a bad entry, or T above the capacity) the two kernels behind it read
//   td_sel_first    kept entry -> k: out_off[k], out_docs[k], src_base[k] = tok_off[sel[i]]; out_off[K] = T
//   td_sel_slots    the slots.  Tiles of 4096 OUTPUT slots, four a lane stored as one int4, so a document of 100 000 ids is
//                   written by as many lanes as it has slots.  Slot j belongs to the k with out_off[k] <= j < out_off[k + 1], an
//                   upper-bound search: a run of kept empty documents shares one offset and is stepped over by the search,
//                   never walked.  group_last_le finds the tile's first k; tile_table puts the offsets behind it into LDS until
//                   one lies beyond the tile, and a lane bisects there (last_le).  A tile whose documents do not fit (thousands of
//                   empty ones) finds its last k by a second group_last_le, and its lanes bisect over the offsets themselves
//                   (last_le_global).
//                   A lane resolves and loads its sixteen slots first and stores them afterwards.  <SelectLabArgs>: the pair
//                   form, lab.src -> lab.dst by the same resolved source; <SelectArgs>: one stream.
#include <hip/hip_runtime.h>

#include "td_rows_common.h"
#include "td_select.h"

namespace td {

namespace {

constexpr int SEL_THREADS = RC_THREADS, SEL_TILE = RC_TILE, SEL_MAX_GRID = RC_MAX_GRID;

struct SelEntry {
    int64_t doc, lo, len;  // sel[i], tok_off[doc], L
    bool bad, keep, is_short, is_long;
};

// Entry i: nothing outside sel[0, n_sel) and tok_off[0, n_docs] is read.
__device__ __forceinline__ SelEntry sel_entry(const SelectArgs& a, int64_t i) {
    SelEntry e{};
    e.doc = a.sel ? a.sel[i] : i;
    if (e.doc < 0 || e.doc >= a.n_docs) {
        e.bad = true;
        return e;
    }
    e.lo = a.tok_off[e.doc];
    const int64_t hi = a.tok_off[e.doc + 1];
    if (e.lo < 0 || hi < e.lo || hi > a.n_tokens) {
        e.bad = true;
        return e;
    }
    e.len = hi - e.lo;
    e.is_short = e.len < a.min_len;
    e.is_long = !e.is_short && a.max_len >= 0 && e.len > a.max_len;
    e.keep = !e.is_short && !e.is_long;
    return e;
}

__global__ __launch_bounds__(SEL_THREADS) void td_sel_count(const SelectArgs a) {
    __shared__ long long s_red[SEL_THREADS / 64];
    const int tid = threadIdx.x;
    long long kept = 0, kept_ids = 0, n_short = 0, n_long = 0, n_bad = 0;
    int64_t bad_at = 0;
    for (int q = 0; q < 4; ++q) {
        const int64_t i = (int64_t)blockIdx.x * RC_SCAN_CHUNK + tid * 4 + q;
        if (i >= a.n_sel) break;
        const SelEntry e = sel_entry(a, i);
        if (e.bad && !n_bad) bad_at = i;
        n_bad += e.bad;
        kept += e.keep;
        kept_ids += e.keep ? e.len : 0;
        n_short += e.is_short;
        n_long += e.is_long;
    }
    if (n_bad) rows_raise(a, TD_E_INVALID, bad_at);
    kept = block_sum(kept, s_red);
    kept_ids = block_sum(kept_ids, s_red);
    n_short = block_sum(n_short, s_red);
    n_long = block_sum(n_long, s_red);
    n_bad = block_sum(n_bad, s_red);
    if (tid == 0) {
        a.scan[SEL_SCAN_HEAD + 2 * (int64_t)blockIdx.x] = (unsigned long long)kept;
        a.scan[SEL_SCAN_HEAD + 2 * (int64_t)blockIdx.x + 1] = (unsigned long long)kept_ids;
        if (n_short) atomicAdd(&a.scan[SEL_SHORT], (unsigned long long)n_short);
        if (n_long) atomicAdd(&a.scan[SEL_LONG], (unsigned long long)n_long);
        if (n_bad) atomicAdd(&a.scan[SEL_BAD], 1ull);
    }
}

__global__ __launch_bounds__(SEL_THREADS) void td_sel_chunks(const SelectArgs a, int64_t nch) {
    __shared__ long long s_wave[SEL_THREADS / 64];
    const int tid = threadIdx.x;
    long long carry[2];  // kept entries, kept ids
    chunks_excl_scan<2>(a.scan + SEL_SCAN_HEAD, nch, s_wave, carry);
    if (tid == 0) {
        const long long carry_k = carry[0], carry_t = carry[1];
        const bool bad = a.scan[SEL_BAD] != 0;
        const bool fits = !bad && carry_t <= a.ids_cap;
        if (!bad && !fits) rows_raise(a, TD_E_CAPACITY, carry_t);
        a.scan[SEL_LEAVE] = fits ? 0ull : 1ull;
        a.scan[SEL_K] = (unsigned long long)carry_k;
        a.scan[SEL_T] = (unsigned long long)carry_t;
        a.counts[0] = bad ? 0 : carry_k;
        a.counts[1] = bad ? 0 : carry_t;
        a.counts[2] = bad ? 0 : (long long)a.scan[SEL_SHORT];
        a.counts[3] = bad ? 0 : (long long)a.scan[SEL_LONG];
    }
}

__global__ __launch_bounds__(SEL_THREADS) void td_sel_first(const SelectArgs a) {
    __shared__ long long s_wave[SEL_THREADS / 64];
    if (a.scan[SEL_LEAVE]) return;  // (every entry is valid behind this line)
    const int tid = threadIdx.x;
    SelEntry e[4];
    long long sum_k = 0, sum_t = 0;
    for (int q = 0; q < 4; ++q) {
        const int64_t i = (int64_t)blockIdx.x * RC_SCAN_CHUNK + tid * 4 + q;
        e[q] = i < a.n_sel ? sel_entry(a, i) : SelEntry{};
        sum_k += e[q].keep;
        sum_t += e[q].keep ? e[q].len : 0;
    }
    long long total;
    long long k = (long long)a.scan[SEL_SCAN_HEAD + 2 * (int64_t)blockIdx.x] + block_excl(sum_k, s_wave, total);
    long long off = (long long)a.scan[SEL_SCAN_HEAD + 2 * (int64_t)blockIdx.x + 1] + block_excl(sum_t, s_wave, total);
    for (int q = 0; q < 4; ++q) {
        if (!e[q].keep) continue;
        a.out_off[k] = off;
        if (a.out_docs) a.out_docs[k] = e[q].doc;
        a.src_base[k] = e[q].lo;
        ++k;
        off += e[q].len;
    }
    if (blockIdx.x == 0 && tid == 0) a.out_off[a.scan[SEL_K]] = (int64_t)a.scan[SEL_T];
}

template <class A>
__global__ __launch_bounds__(SEL_THREADS) void td_sel_slots(const A a) {
    constexpr bool LAB = has_lab<A>;
    constexpr int ITERS = SEL_TILE / (4 * SEL_THREADS);
    __shared__ int32_t s_off[RC_LDS_DOCS];  // out_off[k0 + i] - s0, clamped to [0, SEL_TILE + 1]
    const int tid = threadIdx.x;
    if (a.scan[SEL_LEAVE]) return;
    const int64_t K = (int64_t)a.scan[SEL_K], T = (int64_t)a.scan[SEL_T];
    const int64_t ntiles = (T + SEL_TILE - 1) / SEL_TILE;
    const auto off_of = [off = a.out_off](int64_t k) { return off[k]; };
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t s0 = tile * SEL_TILE;
        const int64_t s1 = s0 + SEL_TILE < T ? s0 + SEL_TILE : T;
        const int32_t span = (int32_t)(s1 - s0);
        __syncthreads();  // (the previous tile's readers of s_off are done)
        // k0: the document of slot s0 (out_off[0] = 0 <= s0 < T = out_off[K])
        const int64_t k0 = group_last_le(off_of, 0, K, s0);
        const int64_t o0 = a.out_off[k0];
        bool lds;
        // documents [k0, k0 + nk) begin below s1 (out_off[K] = T >= s1 does not); in LDS: s_off[0, nk], the last the end of them all
        int64_t nk = tile_table(s_off, off_of, k0, K, s0, 0, SEL_TILE + 1, span, lds);
        if (!lds) nk = group_last_le(off_of, k0, K, s1 - 1) - k0 + 1;
        // i: the last of the tile's documents that begins at or below slot j
        auto find = [&](int64_t j) -> int64_t {
            if (lds) return last_le(s_off, nk, (int32_t)(j - s0));
            return last_le_global([off = a.out_off + k0](int64_t i) { return off[i]; }, 0, nk, j);
        };
        int32_t v[ITERS][4] = {};
        [[maybe_unused]] int32_t lv[ITERS][4] = {};
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
            const int64_t j0 = s0 + (int64_t)it * 4 * SEL_THREADS + 4 * tid;
            if (j0 < s1) {
                int64_t start = 0, end = 0, base = 0;  // the document's slots [start, end) (in LDS: clamped behind the tile), its first id
                auto resolve = [&](int64_t j) {
                    const int64_t i = find(j);
                    start = lds ? (i == 0 ? o0 : s0 + s_off[i]) : a.out_off[k0 + i];
                    end = lds ? s0 + s_off[i + 1] : a.out_off[k0 + i + 1];
                    base = a.src_base[k0 + i];
                };
                resolve(j0);
                const int64_t src = base + (j0 - start);
                if (j0 + 4 <= end && j0 + 4 <= s1 && src >= 0 && src + 4 <= a.n_tokens) {
                    rows_get4(a.ids, src, v[it]);
                    if constexpr (LAB) rows_get4(a.lab.src, src, lv[it]);
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int64_t j = j0 + q;
                        if (j < s1) {
                            if (j >= end) resolve(j);
                            const int64_t sq = base + (j - start);
                            if (sq >= 0 && sq < a.n_tokens) {  // (checked offsets give nothing else: a second fence)
                                v[it][q] = a.ids[sq];
                                if constexpr (LAB) lv[it][q] = a.lab.src[sq];
                            }
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int it = 0; it < ITERS; ++it) {
            const int64_t j0 = s0 + (int64_t)it * 4 * SEL_THREADS + 4 * tid;
            if (j0 < s1) {
                rows_put4(a.out, j0, s1, v[it]);
                lab_put4(a, j0, s1, lv[it]);
            }
        }
    }
}

}  // namespace

int64_t select_scan_words(int64_t n_sel) { return SEL_SCAN_HEAD + 2 * (n_sel > 0 ? (n_sel + RC_SCAN_CHUNK - 1) / RC_SCAN_CHUNK : 1); }

hipError_t launch_select(const SelectLabArgs& al, hipStream_t stream) {
    const SelectArgs& a = al;
    const int64_t nch = (select_scan_words(a.n_sel) - SEL_SCAN_HEAD) / 2;
    hipLaunchKernelGGL(td_sel_count, dim3((unsigned)nch), dim3(SEL_THREADS), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(td_sel_chunks, dim3(1), dim3(SEL_THREADS), 0, stream, a, nch);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(td_sel_first, dim3((unsigned)nch), dim3(SEL_THREADS), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const int64_t tiles = a.ids_cap / SEL_TILE + 1;
    const int grid = (int)(tiles < SEL_MAX_GRID ? tiles : SEL_MAX_GRID);
    if (al.lab.src) hipLaunchKernelGGL(td_sel_slots<SelectLabArgs>, dim3(grid), dim3(SEL_THREADS), 0, stream, al);
    else hipLaunchKernelGGL(td_sel_slots<SelectArgs>, dim3(grid), dim3(SEL_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace td
