// Whole documents packed into rows by best-fit decreasing (td_pack_rows*, td_encode_batch_pack_rows; TD_ROWS_BESTFIT).
//
// The placement is sequential by nature; it is kept small and on the host, and every per-document and per-slot step is here:
//   td_pack_items     one pass over tok_offsets: a document's slots n_d, its full chunks and its remainder, the offsets' checks
//                     (nothing outside [0, n_tokens) is ever read) and the totals F (full chunks), R (real slots), documents cut
//   rocPRIM           an exclusive scan of the full chunks (full row f -> its document), a stable radix sort of (S - remainder,
//                     document) over the bits of S only, and a run-length encode of the sorted keys: at most min(S, n_docs) runs
//   (host)            the header and the runs come back in one copy; pack_plan_runs places whole runs (td_pack.h)
//   td_pack_segments  every segment's start, document and first slot inside its document: full rows, the sorted remainders
//                     (each finds its placement by a search over the placements' first items) and the pad tails; cu_seqlens,
//                     seg_docs and row_lengths come out of the same pass
//   td_pack_slots     td_rows_concat's tile walk with segments in place of documents: a tile of 4096 output slots keeps the
//                     starts of the segments that overlap it in LDS (at most 4097: no segment is empty), every lane searches
//                     them once for its first slot (last_le, td_rows_common.h; the searches over global arrays here and in
//                     td_pack_segments are its last_le_global) and walks a cursor; ids are written as int4, positions only when asked for;
//                     <PackLabArgs>: the pair form, lab.src -> lab.dst beside the ids (td_rows_common.h), <PackArgs>: one stream
#include <hip/hip_runtime.h>

#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <functional>
#include <map>
#include <queue>

#include "td_pack.h"
#include "td_rows_common.h"

namespace td {

// ---- the host planner --------------------------------------------------------------------------------------------------------
void pack_plan_runs(int64_t S, int64_t full, int64_t real, const int64_t* lens, const int64_t* counts, int64_t n_runs, PackPlan& out) {
    out.S = S;
    out.full = full;
    out.real = real;
    out.pl.clear();
    out.fill.clear();
    out.seg0.clear();
    std::vector<int64_t> items;  // [mixed rows] items placed so far
    // free slot count -> the rows with it, lowest index first (rows with no free slot are not kept)
    std::map<int64_t, std::priority_queue<int64_t, std::vector<int64_t>, std::greater<int64_t>>> by_free;
    int64_t item = 0;
    for (int64_t r = 0; r < n_runs; ++r) {
        const int64_t l = lens[r];
        int64_t k = counts[r];
        while (k > 0) {
            auto it = by_free.lower_bound(l);
            int64_t row, f;
            if (it == by_free.end()) {  // no row has room: a new one
                row = full + (int64_t)out.fill.size();
                f = S;
                out.fill.push_back(0);
                items.push_back(0);
            } else {
                f = it->first;
                row = it->second.top();
                it->second.pop();
                if (it->second.empty()) by_free.erase(it);
            }
            const int64_t c = std::min(k, f / l), m = row - full;
            out.pl.push_back({l, row, out.fill[m], c, item, items[m]});  // (first_seg: the row's items before it, until below)
            out.fill[m] += c * l;
            items[m] += c;
            item += c;
            k -= c;
            if (f - c * l > 0) by_free[f - c * l].push(row);
        }
    }
    const int64_t mixed = (int64_t)out.fill.size();
    out.seg0.resize(mixed + 1);
    int64_t seg = full;
    for (int64_t m = 0; m < mixed; ++m) {
        out.seg0[m] = seg;
        seg += items[m] + (out.fill[m] < S);
    }
    out.seg0[mixed] = seg;
    for (PackPlacement& p : out.pl) p.first_seg += out.seg0[p.row - full];
    out.rows = full + mixed;
    out.segs = seg;
}

namespace {

constexpr int PACK_THREADS = RC_THREADS, PACK_TILE = RC_TILE, PACK_MAX_GRID = RC_MAX_GRID;

// body ids of document d after truncation
__device__ __forceinline__ int64_t pack_body(const PackArgs& a, int64_t L) {
    if (!a.truncate) return L;
    const int64_t room = a.S - a.b - a.e;
    return L < room ? L : room;
}

__global__ __launch_bounds__(PACK_THREADS) void td_pack_items(const PackArgs a) {
    __shared__ long long s_red[PACK_THREADS / 64];
    long long F = 0, R = 0, cut = 0, items = 0, bad = 0;  // bad: n_docs - (the lowest document with bad offsets)
    const int64_t S = a.S;
    for (int64_t d = (int64_t)blockIdx.x * PACK_THREADS + threadIdx.x; d < a.n_docs; d += (int64_t)gridDim.x * PACK_THREADS) {
        const int64_t o0 = a.tok_off[d], o1 = a.tok_off[d + 1];
        const bool ok = o0 >= 0 && o1 >= o0 && o1 <= a.n_tokens;
        if (!ok) bad = max(bad, (long long)(a.n_docs - d));
        const int64_t L = ok ? o1 - o0 : 0, body = pack_body(a, L), n = a.b + body + a.e;
        int64_t fl, rem;
        if (a.truncate) {  // (n <= S)
            fl = n == S;
            rem = n == S ? 0 : n;
            cut += body < L;
        } else {
            fl = n / S;
            rem = n - fl * S;
            cut += n > S;
        }
        R += n;
        F += fl;
        items += rem > 0;
        a.key[d] = (uint32_t)(rem ? S - rem : S);
        a.val[d] = (uint32_t)d;
        a.full[d] = fl;
    }
    F = block_sum(F, s_red);
    R = block_sum(R, s_red);
    cut = block_sum(cut, s_red);
    items = block_sum(items, s_red);
    bad = block_max(bad, s_red);
    if (threadIdx.x == 0) {
        unsigned long long* h = (unsigned long long*)a.hdr;
        if (F) atomicAdd(h + PH_FULL, (unsigned long long)F);
        if (R) atomicAdd(h + PH_REAL, (unsigned long long)R);
        if (cut) atomicAdd(h + PH_CUT, (unsigned long long)cut);
        if (items) atomicAdd(h + PH_ITEMS, (unsigned long long)items);
        if (bad) {
            atomicMax(h + PH_ERR, 1ull);
            atomicMax(h + PH_ERR_DOC, (unsigned long long)bad);
        }
    }
}

__device__ __forceinline__ void pack_put(const PackArgs& a, int64_t k, int64_t start, int64_t d, int64_t q0) {
    a.seg_start[k] = start;
    a.seg_doc[k] = d;
    a.seg_q0[k] = q0;
    if (a.cu) a.cu[k] = (int32_t)start;
    if (a.docs) a.docs[k] = d;
}

__global__ __launch_bounds__(PACK_THREADS) void td_pack_segments(const PackArgs a) {
    const int64_t S = a.S, F = a.full_rows;
    const int64_t n_work = F + a.n_items + a.n_mixed + a.rows;
    const int64_t g = (int64_t)blockIdx.x * PACK_THREADS + threadIdx.x;
    if (g == 0) {
        a.seg_start[a.segs] = a.rows * S;
        if (a.cu) a.cu[a.segs] = (int32_t)(a.rows * S);
    }
    for (int64_t idx = g; idx < n_work; idx += (int64_t)gridDim.x * PACK_THREADS) {
        int64_t x = idx;
        if (x < F) {  // full row f: the last document whose exclusive prefix of full chunks is <= f
            const int64_t lo = last_le_global([pref = a.pref](int64_t d) { return pref[d]; }, 0, a.n_docs, x);
            pack_put(a, x, x * S, lo, (x - a.pref[lo]) * S);
            continue;
        }
        x -= F;
        if (x < a.n_items) {  // sorted remainder item i: the last placement whose first item is <= i
            const PackPlacement p = a.pl[last_le_global([pl = a.pl](int64_t i) { return pl[i].first_item; }, 0, a.n_pl, x)];
            const int64_t j = x - p.first_item, d = a.sorted_doc[x];
            const int64_t n = a.b + pack_body(a, a.tok_off[d + 1] - a.tok_off[d]) + a.e;
            pack_put(a, p.first_seg + j, p.row * S + p.slot + j * p.len, d, n - p.len);  // (truncate: n = len, q0 = 0)
            continue;
        }
        x -= a.n_items;
        if (x < a.n_mixed) {  // a mixed row's pad tail
            const int64_t fl = a.fill[x];
            if (fl < S) pack_put(a, a.seg0[x + 1] - 1, (F + x) * S + fl, -1, 0);
            continue;
        }
        x -= a.n_mixed;
        if (a.lengths) a.lengths[x] = (int32_t)(x < F ? S : a.fill[x - F]);
    }
}

// the last segment k in [0, segs) with seg_start[k] <= j
__device__ __forceinline__ int64_t pack_seg_search(const PackArgs& a, int64_t j) {
    return last_le_global([st = a.seg_start](int64_t k) { return st[k]; }, 0, a.segs, j);
}

template <class A>
__global__ __launch_bounds__(PACK_THREADS) void td_pack_slots(const A a) {
    constexpr bool LAB = has_lab<A>;
    __shared__ int32_t s_rel[PACK_TILE + 2];  // starts of the tile's segments - t0 (the first clamped to 0), then the next one's
    const int tid = threadIdx.x;
    const int64_t S = a.S, total = a.rows * S;
    const int64_t ntiles = (total + PACK_TILE - 1) / PACK_TILE;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t t0 = tile * PACK_TILE;
        const int64_t t1 = t0 + PACK_TILE < total ? t0 + PACK_TILE : total;
        const int64_t ka = pack_seg_search(a, t0), kb = pack_seg_search(a, t1 - 1);
        const int nk = (int)(kb - ka + 1);  // segments that overlap the tile (<= PACK_TILE)
        __syncthreads();  // (the previous tile's readers of s_rel are done)
        for (int i = tid; i <= nk; i += PACK_THREADS) {
            const int64_t r = a.seg_start[ka + i] - t0;  // (ka + nk <= segs: the sentinel rows * S)
            s_rel[i] = r < 0 ? 0 : r > PACK_TILE ? PACK_TILE : (int32_t)r;
        }
        __syncthreads();
        for (int it = 0; it < PACK_TILE / (4 * PACK_THREADS); ++it) {
            const int64_t j0 = t0 + (int64_t)it * 4 * PACK_THREADS + 4 * tid;
            if (j0 >= t1) break;
            int i = last_le(s_rel, nk, (int32_t)(j0 - t0)), cur = -1;
            int64_t d = -1, start = 0, q0 = 0, base = 0, eos_at = 0;
            int32_t v[4], ps[4];
            [[maybe_unused]] int32_t lv[4];
            for (int q = 0; q < 4; ++q) {
                const int64_t j = j0 + q;
                if constexpr (LAB) lv[q] = a.lab.pad;  // (what every slot without a document holds)
                if (j >= t1) { v[q] = a.pad; ps[q] = 0; continue; }
                while (i + 1 < nk && s_rel[i + 1] <= (int32_t)(j - t0)) ++i;
                if (i != cur) {
                    cur = i;
                    const int64_t k = ka + i;
                    d = a.seg_doc[k];
                    start = a.seg_start[k];
                    q0 = a.seg_q0[k];
                    if (d >= 0) {
                        base = a.tok_off[d];
                        eos_at = a.b + pack_body(a, a.tok_off[d + 1] - base);
                    }
                }
                if (d < 0) { v[q] = a.pad; ps[q] = 0; continue; }
                const int64_t qq = q0 + (j - start);
                ps[q] = (int32_t)(j - start);
                if (a.b && qq == 0) {
                    v[q] = a.bos;
                    if constexpr (LAB) lv[q] = a.lab.bos;
                } else if (a.e && qq == eos_at) {
                    v[q] = a.eos;
                    if constexpr (LAB) lv[q] = a.lab.eos;
                } else {
                    const int64_t src = base + qq - a.b;
                    const bool in = src >= 0 && src < a.n_tokens;  // (always inside: the items kernel checked the offsets)
                    v[q] = in ? a.ids[src] : a.pad;
                    if constexpr (LAB) if (in) lv[q] = a.lab.src[src];
                }
            }
            rows_put4(a.out, j0, t1, v);
            lab_put4(a, j0, t1, lv);
            if (a.pos) rows_put4(a.pos, j0, t1, ps);
        }
    }
}

unsigned pack_grid(int64_t work, int64_t cap) {
    const int64_t g = (work + PACK_THREADS - 1) / PACK_THREADS;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(g, cap));
}

}  // namespace

hipError_t launch_pack_items(const PackArgs& a, hipStream_t stream) {
    if (a.n_docs == 0) return hipSuccess;
    hipLaunchKernelGGL(td_pack_items, dim3(pack_grid(a.n_docs, 1024)), dim3(PACK_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t pack_sort_runs(void* temp, size_t& temp_bytes, const PackArgs& a, uint32_t* key_out, uint32_t* val_out, int64_t* pref,
                          uint32_t* runs_key, uint32_t* runs_cnt, hipStream_t stream) {
    const unsigned n = (unsigned)a.n_docs;
    unsigned end_bit = 0;
    while (end_bit < 32 && ((uint64_t)a.S >> end_bit) != 0) ++end_bit;  // keys are 1 .. S
    unsigned* n_runs = (unsigned*)(a.hdr + PH_RUNS);
    if (!temp) {
        size_t b1 = 0, b2 = 0, b3 = 0;
        hipError_t e;
        if ((e = rocprim::exclusive_scan(nullptr, b1, a.full, pref, (int64_t)0, (size_t)n, rocprim::plus<int64_t>(), stream))) return e;
        if ((e = rocprim::radix_sort_pairs(nullptr, b2, a.key, key_out, a.val, val_out, n, 0u, end_bit, stream))) return e;
        if ((e = rocprim::run_length_encode(nullptr, b3, key_out, n, runs_key, runs_cnt, n_runs, stream))) return e;
        temp_bytes = std::max({b1, b2, b3, (size_t)256});
        return hipSuccess;
    }
    if (n == 0) return hipSuccess;
    hipError_t e;
    size_t sz = temp_bytes;
    if ((e = rocprim::exclusive_scan(temp, sz, a.full, pref, (int64_t)0, (size_t)n, rocprim::plus<int64_t>(), stream))) return e;
    sz = temp_bytes;
    if ((e = rocprim::radix_sort_pairs(temp, sz, a.key, key_out, a.val, val_out, n, 0u, end_bit, stream))) return e;
    sz = temp_bytes;
    return rocprim::run_length_encode(temp, sz, key_out, n, runs_key, runs_cnt, n_runs, stream);
}

hipError_t launch_pack_outputs(const PackLabArgs& al, hipStream_t stream) {
    const PackArgs& a = al;
    const int64_t work = a.full_rows + a.n_items + a.n_mixed + a.rows;
    hipLaunchKernelGGL(td_pack_segments, dim3(pack_grid(work, 4096)), dim3(PACK_THREADS), 0, stream, a);
    const int64_t ntiles = (a.rows * a.S + PACK_TILE - 1) / PACK_TILE;
    const dim3 grid((unsigned)std::min<int64_t>(ntiles, PACK_MAX_GRID));
    if (ntiles > 0 && al.lab.src) hipLaunchKernelGGL(td_pack_slots<PackLabArgs>, grid, dim3(PACK_THREADS), 0, stream, al);
    else if (ntiles > 0) hipLaunchKernelGGL(td_pack_slots<PackArgs>, grid, dim3(PACK_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace td
