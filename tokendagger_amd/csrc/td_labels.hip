// Loss labels for marked id spans (td_span_labels*, td_encode_batch_span_labels): ids + per-document token offsets ->
// labels[i] = ids[i] where the loss applies, ignore_index elsewhere; optionally the mask and the trained ids in front of every
// document.  The rule is the contract in include/tokendagger_hip.h; td_labels.h restates it as a scan: every position is NONE,
// IN (an opener ends here) or OUT (a closer, or the reset in front of a document's first id), the operator is "rightmost
// non-NONE", inside(i) is the exclusive scan at i.
//
// Memory-bound by design: the ids are read once and the labels written once (4 + 4 B an id, + 1 with the mask).  What a tile
// needs from its left is ONE bit, the state in front of it, and that is the last event of the tiles before it.  So the first
// pass does not read the ids: it looks for each tile's LAST event from the tile's end backwards, 256 ids a step, and stops at
// the first step that has one.  Real data has an event every few dozen ids (every document start is one), so that pass reads
// a sixteenth of the ids; a tile without any event is read whole, once: one document of millions of ids without an event
// costs 4 B an id more, never more than that.  No lane waits for another workgroup anywhere, so there is nothing to bound:
// (Measured, DESIGN 4.12: the bytes are not what bounds it yet.  td_lab_apply issues 85 vector and 94 scalar instructions an id
// and takes 4.2 x a copy of the same bytes; the passes around it are a tenth of the time.)
//
//   td_lab_docs         a lane a document: the offsets checks (nothing else runs when one fails), the starts of the non-empty
//                       documents as a bitmap over the ids (td_off_heads' form; no tile searches tok_offsets)
//   td_lab_tiles        a workgroup a tile: the tile's last event, backwards from its end
//   td_lab_carry        one workgroup: the exclusive "rightmost non-NONE" scan of the tiles' events = the state in front of
//                       every tile; the state at the very end (the last document may end inside)
//   td_lab_apply        a workgroup a tile of 4096 ids, sixteen consecutive ids a lane: ids and the 7 ids in front of the tile
//                       into LDS by int4 (padded: the lanes' sixteen-id runs fall on different banks), events per lane as three
//                       16-bit masks (the opener test compares the LAST id first: one compare an opener and id in the common
//                       case; a match may not reach across a document start, which the bitmap in front of the position says),
//                       the scan over lanes and wavefronts, the walk (lab_step) with the state known, labels back through LDS
//                       and out by int4, the mask sixteen bytes a lane.  The three counts by one atomic a workgroup.
//   td_lab_count_carry, only with trained_offsets: the exclusive sum of the tiles' trained ids;
//   td_lab_finish       counts[4]; with trained_offsets a lane a document boundary: the trained ids in front of the boundary's
//                       tile + in front of its lane + the lane's trained bits below it (td_lab_apply left the last two, 4 B a
//                       lane).  Empty documents are boundaries at one position like any other.
//
// Every scan over the lanes of a wavefront here (td_lab_carry, td_lab_apply's state and counts, td_lab_count_carry) is
// td_rows_common.h's wave_incl_scan, with lab_combine or an add as the combine.
#include <hip/hip_runtime.h>

#include "td_labels_args.h"
#include "td_rows_common.h"

namespace td {

namespace {

constexpr int LAB_PAD = 8;                      // ids in front of the tile in LDS (LAB_HALO, rounded to an int4)
constexpr int LAB_LDS_IDS = LAB_TILE + LAB_PAD;
constexpr int LAB_CARRY_THREADS = 1024, LAB_CARRY_PER = 16;
constexpr int LAB_MAX_GRID = 1 << 20;
static_assert(LAB_PER == 16 && LAB_PAD >= LAB_HALO && LAB_THREADS == RC_THREADS, "td_lab_apply");

__device__ __forceinline__ int lab_idx(int j) { return j + (j >> 4); }  // (a lane's run starts 17 words behind its neighbour's)

__device__ __forceinline__ int64_t lab_total(const LabelArgs& a) { return a.tok_off[a.n_docs]; }

// ids of q's document that end at q, at most 8: x = the document starts at q-7 .. q (bit 7 = q)
__device__ __forceinline__ int lab_avail(uint32_t x) { return x ? 8 - (31 - __clz(x)) : 8; }

__global__ __launch_bounds__(LAB_THREADS) void td_lab_docs(const LabelArgs a) {
    const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (gid == 0 && a.tok_off[0] != 0) {
        rows_raise(a, TD_E_INVALID, 0);
        atomicOr(&a.head[LAB_H_BAD], 1ull);
    }
    for (int64_t d = gid; d < a.n_docs; d += (int64_t)gridDim.x * blockDim.x) {
        const int64_t lo = a.tok_off[d], hi = a.tok_off[d + 1];
        if (lo < 0 || hi < lo || hi > a.n_tokens) {
            rows_raise(a, TD_E_INVALID, d);
            atomicOr(&a.head[LAB_H_BAD], 1ull);
        } else if (hi > lo) {
            atomicOr(&a.bits[lo >> 5], 1u << (lo & 31));
        }
    }
}

__global__ __launch_bounds__(LAB_THREADS) void td_lab_tiles(const LabelArgs a) {
    __shared__ long long s_red[LAB_THREADS / 64];
    if (a.head[LAB_H_BAD]) return;
    const int tid = threadIdx.x;
    const int64_t total = lab_total(a), ntiles = (total + LAB_TILE - 1) / LAB_TILE;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t t0 = t * LAB_TILE, t1 = t0 + LAB_TILE < total ? t0 + LAB_TILE : total;
        uint32_t last = LAB_NONE;
        for (int64_t hi = t1; hi > t0; hi -= LAB_THREADS) {
            const int64_t q = hi - 1 - tid;  // (lane 0 has the last id)
            long long key = 0;
            if (q >= t0) {
                const int32_t id = a.ids[q];
                const int64_t w = q >> 5;
                const int sh = (int)(q & 31);
                const uint32_t w1 = a.bits[w];
                const bool doc = (w1 >> sh) & 1u, close = lab_is_close(a.spec, id);
                const uint32_t cand = lab_last_mask(a.spec, id);
                bool open = false;
                if (cand) {
                    const unsigned long long two = ((unsigned long long)w1 << 32) | (w ? a.bits[w - 1] : 0u);
                    const int avail = lab_avail((uint32_t)(two >> (sh + 25)) & 0xFFu);
                    open = lab_open_match(a.spec, cand, [&](int64_t p) { return a.ids[p]; }, q, avail);
                }
                const uint32_t ev = lab_event(doc, open, close);
                if (ev) key = ((long long)(LAB_THREADS - tid) << 2) | ev;
            }
            const long long best = block_max(key, s_red);
            if (best) {
                last = (uint32_t)best & 3u;
                break;
            }
        }
        if (tid == 0) a.tiles[t] = (uint8_t)last;
    }
}

// One workgroup, sixteen tiles a lane: the exclusive scan of the tiles' events, in place as the state in front of each.
__global__ __launch_bounds__(LAB_CARRY_THREADS) void td_lab_carry(const LabelArgs a) {
    __shared__ uint32_t s_wave[LAB_CARRY_THREADS / 64];
    if (a.head[LAB_H_BAD]) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t total = lab_total(a), ntiles = (total + LAB_TILE - 1) / LAB_TILE;
    uint32_t carry = LAB_NONE;
    for (int64_t base = 0; base < ntiles; base += LAB_CARRY_THREADS * LAB_CARRY_PER) {
        const int64_t c0 = base + (int64_t)tid * LAB_CARRY_PER;
        uint4 raw = make_uint4(0, 0, 0, 0);
        if (c0 < ntiles) raw = *reinterpret_cast<const uint4*>(a.tiles + c0);  // (the buffer is rounded up to whole rounds)
        const uint32_t word[4] = {raw.x, raw.y, raw.z, raw.w};
        uint32_t ev[LAB_CARRY_PER], mine = LAB_NONE;
#pragma unroll
        for (int k = 0; k < LAB_CARRY_PER; ++k) {
            ev[k] = c0 + k < ntiles ? (word[k >> 2] >> (8 * (k & 3))) & 3u : LAB_NONE;
            mine = lab_combine(mine, ev[k]);
        }
        const uint32_t incl = wave_incl_scan(mine, lane, [](uint32_t x, uint32_t y) { return lab_combine(x, y); });
        __syncthreads();  // (the readers of the round before are done)
        if (lane == 63) s_wave[wv] = incl;
        __syncthreads();
        uint32_t st = carry, all = carry;
        for (int w = 0; w < LAB_CARRY_THREADS / 64; ++w) {
            if (w < wv) st = lab_combine(st, s_wave[w]);
            all = lab_combine(all, s_wave[w]);
        }
        const uint32_t prev = __shfl_up(incl, 1);
        if (lane) st = lab_combine(st, prev);
        uint32_t out[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < LAB_CARRY_PER; ++k) {
            out[k >> 2] |= (st == LAB_IN ? 1u : 0u) << (8 * (k & 3));
            st = lab_combine(st, ev[k]);
        }
        if (c0 < ntiles) *reinterpret_cast<uint4*>(a.tiles + c0) = make_uint4(out[0], out[1], out[2], out[3]);
        carry = all;
    }
    if (tid == 0) a.head[LAB_H_END] = carry == LAB_IN ? 1ull : 0ull;
}

__global__ __launch_bounds__(LAB_THREADS) void td_lab_apply(const LabelArgs a) {
    __shared__ int32_t s_ids[LAB_LDS_IDS + (LAB_LDS_IDS >> 4) + 1];
    __shared__ uint32_t s_dw[LAB_TILE / 32 + 2];  // the bitmap's words from the one in front of the tile's first
    __shared__ uint32_t s_wave[LAB_THREADS / 64];
    __shared__ long long s_red[LAB_THREADS / 64];
    if (a.head[LAB_H_BAD]) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t total = lab_total(a), ntiles = (total + LAB_TILE - 1) / LAB_TILE;
    const bool ids16 = (((uintptr_t)a.ids) & 15) == 0, out16 = (((uintptr_t)a.labels) & 15) == 0;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t t0 = t * LAB_TILE;
        __syncthreads();  // (the tile before is stored)
        if (tid < LAB_TILE / 32 + 2) {
            const int64_t gw = t0 / 32 - 1 + tid;
            s_dw[tid] = gw >= 0 && gw <= ((total - 1) >> 5) ? a.bits[gw] : 0u;
        }
        for (int r = tid; r < LAB_LDS_IDS / 4; r += LAB_THREADS) {
            const int64_t p = t0 - LAB_PAD + 4 * r;
            int32_t v[4];
            if (p >= 0 && p + 4 <= total && ids16) {
                const int4 q = *reinterpret_cast<const int4*>(a.ids + p);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] = p + c >= 0 && p + c < total ? a.ids[p + c] : -1;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) s_ids[lab_idx(4 * r + c)] = v[c];
        }
        __syncthreads();
        // ---- the lane's sixteen ids: events as masks -------------------------------------------------------------------
        const int jb = LAB_PAD + LAB_PER * tid;           // the LDS position of the lane's first id
        const int64_t p0 = t0 + LAB_PER * tid;
        const int nv = total - p0 >= LAB_PER ? LAB_PER : total - p0 > 0 ? (int)(total - p0) : 0;  // ids of the lane below total
        uint32_t dwin;  // document starts: bit b = LDS position 16 * tid + b, so bit 8 + i is the lane's id i
        {
            const int pos = LAB_PER * tid + 24, k = pos >> 5, sh = pos & 31;
            const unsigned long long two = s_dw[k] | ((unsigned long long)s_dw[k + 1] << 32);
            dwin = (uint32_t)(two >> sh) & 0xFFFFFFu;
        }
        uint32_t ob = 0, cb = 0;
        const uint32_t db = (dwin >> 8) & (nv >= 16 ? 0xFFFFu : (1u << nv) - 1u);
        for (int i = 0; i < nv; ++i) {
            const int32_t id = s_ids[lab_idx(jb + i)];
            cb |= lab_is_close(a.spec, id) ? 1u << i : 0u;
            const uint32_t cand = lab_last_mask(a.spec, id);
            if (cand) {
                const int avail = lab_avail((dwin >> (i + 1)) & 0xFFu);
                if (lab_open_match(a.spec, cand, [&](int64_t j) { return s_ids[lab_idx((int)j)]; }, jb + i, avail)) ob |= 1u << i;
            }
        }
        uint32_t ev = LAB_NONE;
        if (const uint32_t m = ob | cb | db) ev = (ob >> (31 - __clz(m))) & 1u ? LAB_IN : LAB_OUT;
        // ---- the state in front of the lane ---------------------------------------------------------------------------
        const uint32_t incl = wave_incl_scan(ev, lane, [](uint32_t x, uint32_t y) { return lab_combine(x, y); });
        if (lane == 63) s_wave[wv] = incl;
        __syncthreads();  // (and every lane has read what it needs of its neighbour's ids)
        uint32_t st = a.tiles[t] ? LAB_IN : LAB_NONE;
        for (int w = 0; w < wv; ++w) st = lab_combine(st, s_wave[w]);
        const uint32_t prev = __shfl_up(incl, 1);
        if (lane) st = lab_combine(st, prev);
        // ---- the walk -------------------------------------------------------------------------------------------------
        uint32_t inside = st == LAB_IN ? 1u : 0u, tb = 0, n_tr = 0, n_sp = 0, n_un = 0;
        const bool train_close = a.spec.train_close != 0;
        const int32_t ignore = a.spec.ignore;
        for (int i = 0; i < nv; ++i) {
            bool tr;
            inside = lab_step(inside, (db >> i) & 1u, (ob >> i) & 1u, (cb >> i) & 1u, train_close, tr, n_tr, n_sp, n_un);
            tb |= tr ? 1u << i : 0u;
            if (!tr) s_ids[lab_idx(jb + i)] = ignore;
        }
        if (a.mask && nv > 0) {
            uint8_t* mp = a.mask + p0;
            if (nv == LAB_PER && (((uintptr_t)mp) & 15) == 0) {
                uint32_t w[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const uint32_t n4 = (tb >> (4 * c)) & 15u;
                    w[c] = (n4 & 1u) | (n4 & 2u) << 7 | (n4 & 4u) << 14 | (n4 & 8u) << 21;
                }
                *reinterpret_cast<uint4*>(mp) = make_uint4(w[0], w[1], w[2], w[3]);
            } else {
                for (int i = 0; i < nv; ++i) mp[i] = (tb >> i) & 1u;
            }
        }
        // ---- counts (a tile has at most 4096 of each) -------------------------------------------------------------------
        const long long packed = (long long)n_tr | (long long)n_sp << 16 | (long long)n_un << 32;
        long long sums;
        if (a.trained_off) {  // the lanes' exclusive sums too
            const long long incl2 = wave_incl_scan(packed, lane, [](long long x, long long y) { return x + y; });
            if (lane == 63) s_red[wv] = incl2;
            __syncthreads();
            long long before = 0;
            sums = 0;
            for (int w = 0; w < LAB_THREADS / 64; ++w) {
                if (w < wv) before += s_red[w];
                sums += s_red[w];
            }
            a.aux[t * LAB_THREADS + tid] = (uint32_t)((before + incl2 - packed) & 0xFFFF) << 16 | tb;
            if (tid == 0) a.tile_cnt[t] = (unsigned long long)(sums & 0xFFFF);
        } else {
            sums = block_sum(packed, s_red);
        }
        if (tid == 0) {
            if (sums & 0xFFFF) atomicAdd(&a.head[LAB_H_TRAINED], (unsigned long long)(sums & 0xFFFF));
            if ((sums >> 16) & 0xFFFF) atomicAdd(&a.head[LAB_H_SPANS], (unsigned long long)((sums >> 16) & 0xFFFF));
            if ((sums >> 32) & 0xFFFF) atomicAdd(&a.head[LAB_H_UNTERM], (unsigned long long)((sums >> 32) & 0xFFFF));
        }
        __syncthreads();  // (the labels are in LDS)
        for (int r = tid; r < LAB_TILE / 4; r += LAB_THREADS) {
            const int64_t p = t0 + 4 * r;
            if (p >= total) break;
            int32_t v[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = s_ids[lab_idx(LAB_PAD + 4 * r + c)];
            if (p + 4 <= total && out16) {
                *reinterpret_cast<int4*>(a.labels + p) = make_int4(v[0], v[1], v[2], v[3]);
            } else {
                for (int c = 0; c < 4; ++c)
                    if (p + c < total) a.labels[p + c] = v[c];
            }
        }
    }
}

// One workgroup, sixteen tiles a lane: the exclusive sum of the tiles' trained ids, in place.
__global__ __launch_bounds__(LAB_CARRY_THREADS) void td_lab_count_carry(const LabelArgs a) {
    __shared__ unsigned long long s_wave[LAB_CARRY_THREADS / 64];
    if (a.head[LAB_H_BAD]) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t total = lab_total(a), ntiles = (total + LAB_TILE - 1) / LAB_TILE;
    unsigned long long carry = 0;
    for (int64_t base = 0; base < ntiles; base += LAB_CARRY_THREADS * LAB_CARRY_PER) {
        const int64_t c0 = base + (int64_t)tid * LAB_CARRY_PER;
        unsigned long long v[LAB_CARRY_PER], mine = 0;
#pragma unroll
        for (int k = 0; k < LAB_CARRY_PER; ++k) {
            v[k] = c0 + k < ntiles ? a.tile_cnt[c0 + k] : 0ull;
            mine += v[k];
        }
        const unsigned long long incl = wave_incl_scan(mine, lane, [](unsigned long long x, unsigned long long y) { return x + y; });
        __syncthreads();
        if (lane == 63) s_wave[wv] = incl;
        __syncthreads();
        unsigned long long run = carry, all = carry;
        for (int w = 0; w < LAB_CARRY_THREADS / 64; ++w) {
            if (w < wv) run += s_wave[w];
            all += s_wave[w];
        }
        run += incl - mine;
#pragma unroll
        for (int k = 0; k < LAB_CARRY_PER; ++k) {
            if (c0 + k < ntiles) a.tile_cnt[c0 + k] = run;
            run += v[k];
        }
        carry = all;
    }
}

__global__ __launch_bounds__(LAB_THREADS) void td_lab_finish(const LabelArgs a) {
    if (a.head[LAB_H_BAD]) return;
    const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const long long trained = (long long)a.head[LAB_H_TRAINED];
    if (gid == 0) {
        a.counts[0] = trained;
        a.counts[1] = (long long)a.head[LAB_H_SPANS];
        a.counts[2] = (long long)(a.head[LAB_H_UNTERM] + a.head[LAB_H_END]);
        a.counts[3] = 0;
    }
    if (!a.trained_off) return;
    const int64_t total = lab_total(a);
    for (int64_t d = gid; d <= a.n_docs; d += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = a.tok_off[d];
        long long v = trained;
        if (p < total) {
            const int64_t t = p / LAB_TILE;
            const uint32_t w = a.aux[t * LAB_THREADS + (p % LAB_TILE) / LAB_PER];
            v = (long long)a.tile_cnt[t] + (w >> 16) + __popc(w & ((1u << (p % LAB_PER)) - 1u));
        }
        a.trained_off[d] = v;
    }
}

}  // namespace

int64_t labels_tiles(int64_t n_tokens) { return n_tokens > 0 ? (n_tokens + LAB_TILE - 1) / LAB_TILE : 1; }

int64_t labels_tiles_rounded(int64_t n_tokens) {
    const int64_t round = (int64_t)LAB_CARRY_THREADS * LAB_CARRY_PER;
    return (labels_tiles(n_tokens) + round - 1) / round * round;
}

hipError_t launch_labels(const LabelArgs& a, hipStream_t stream) {
    const auto grid_of = [](int64_t n, int per) {
        const int64_t g = (n + per - 1) / per;
        return (unsigned)(g < 1 ? 1 : g < LAB_MAX_GRID ? g : LAB_MAX_GRID);
    };
    const unsigned g_docs = grid_of(a.n_docs + 1, LAB_THREADS) < 4096u ? grid_of(a.n_docs + 1, LAB_THREADS) : 4096u;
    const unsigned g_tiles = grid_of(labels_tiles(a.n_tokens), 1);
    hipError_t e;
    hipLaunchKernelGGL(td_lab_docs, dim3(g_docs), dim3(LAB_THREADS), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(td_lab_tiles, dim3(g_tiles), dim3(LAB_THREADS), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(td_lab_carry, dim3(1), dim3(LAB_CARRY_THREADS), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(td_lab_apply, dim3(g_tiles), dim3(LAB_THREADS), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return launch_labels_finish(a, stream);
}

hipError_t launch_labels_finish(const LabelArgs& a, hipStream_t stream) {
    const int64_t g = (a.n_docs + 1 + LAB_THREADS - 1) / LAB_THREADS;
    const unsigned g_docs = (unsigned)(g < 4096 ? g : 4096);
    if (a.trained_off) {
        hipLaunchKernelGGL(td_lab_count_carry, dim3(1), dim3(LAB_CARRY_THREADS), 0, stream, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(td_lab_finish, dim3(a.trained_off ? g_docs : 1u), dim3(LAB_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace td
