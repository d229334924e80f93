// Loss labels from byte ranges (td_range_labels*, td_encode_batch_range_labels): ids + per-document token offsets + per document
// a sorted list of byte ranges -> labels[i] = ids[i] for the ids the rule picks, ignore_index elsewhere; optionally the mask and
// the trained ids in front of every document.  The rule is the contract in include/tokendagger_hip.h, by marked BYTES:
// id i of document d lies at [s_i, e_i), m_i of its bytes are marked.  With cum[r] = the bytes of the ranges in front of r,
//     G(x) = cum[k] + clamp(x - begin[k], 0, end[k] - begin[k]),   k = the last range of d with begin <= x   (none: cum[first of d])
// is the marked bytes of d in front of x (+ a constant per document), so m_i = G(e_i) - G(s_i) and byte s_i is marked iff
// s_i < end[k]: all three rules from one search, and in the covered form e_i is the next id's s, so an id costs one search.
//
// The starts are never written: the covered form takes the carry into every tile from td_offsets.hip's own first two passes
// (launch_chunk_carries, on the bitmap td_rng_docs builds) and redoes the segmented scan inside the tile in registers; the
// explicit form is the same kernel with loads in place of the scan.
//
//   td_rng_docs     a lane a document: both offset arrays checked (nothing else writes when one fails), the starts of the non-empty
//                   documents as a bitmap over the ids, every document's first range as a bitmap over the ranges; covered form:
//                   a document without ids may have no range that ends above 0
//   td_rng_check    four ranges a lane: 0 <= begin <= end, begin >= the end before it in the same document (the lowest bad index
//                   by an atomic maximum), the lengths' exclusive sums inside the chunk and the chunk's total
//   td_rng_cum      one workgroup: the chunk totals to their prefixes (chunks_excl_scan), the marked bytes; raises the bad range
//   td_rng_apply    a workgroup a tile of 4096 ids, sixteen consecutive ids a lane (td_lab_apply's shape, so td_lab_count_carry and
//                   td_lab_finish take its results as they are): ids by int4 into registers, their lengths into LDS, the scan over
//                   lanes and wavefronts, the tile's documents by the shared locator (group_last_le, tile_table), the window of
//                   ranges the tile can touch (two workgroup searches, from the tile's first start and last end) into LDS when it
//                   has at most RNG_WIN entries, the walk, labels by int4 and the mask sixteen bytes a lane
//   td_rng_status   covered form: raises what td_rng_apply found at the documents' ends
#include <hip/hip_runtime.h>

#include "td_offsets_dev.h"
#include "td_ranges_args.h"
#include "td_rows_common.h"

namespace td {

namespace {

constexpr int RNG_THREADS = RC_THREADS, RNG_PER = RNG_TILE / RNG_THREADS;
constexpr unsigned long long RNG_TOP = 0x7FFFFFFFFFFFFFFFull;
static_assert(RNG_PER == 16 && RNG_PER == LAB_PER && RNG_THREADS == LAB_THREADS && RNG_CHUNK == RC_SCAN_CHUNK, "td_rng_apply, td_rng_check");

__device__ __forceinline__ int len_idx(int j) { return j + 2 * (j >> 4); }  // (16-bit entries: a lane's run starts 9 words behind its neighbour's)

__device__ __forceinline__ int64_t rng_total(const RangeArgs& a) { return a.tok_off[a.n_docs]; }
__device__ __forceinline__ void rng_lowest(const RangeArgs& a, int word, int64_t idx) { atomicMax(&a.head[word], RNG_TOP - (unsigned long long)idx); }
__device__ __forceinline__ void rng_bad_doc(const RangeArgs& a, int64_t d) {
    rows_raise(a, TD_E_INVALID, d);
    atomicOr(&a.head[LAB_H_BAD], 1ull);
}
// the first range in [r0, r1) (sorted: the ends do not decrease) that ends above x, given that the last one does
__device__ __forceinline__ int64_t rng_first_beyond(const RangeArgs& a, int64_t r0, int64_t r1, long long x) {
    if (a.ranges[2 * r0 + 1] > x) return r0;
    return last_le_global([&](int64_t r) { return a.ranges[2 * r + 1]; }, r0, r1, x) + 1;
}

__global__ __launch_bounds__(RNG_THREADS) void td_rng_docs(const RangeArgs a) {
    const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (gid == 0) {
        if (a.tok_off[0] != 0 || a.range_off[0] != 0) rng_bad_doc(a, 0);
        if (a.range_off[a.n_docs] != a.n_ranges) rng_bad_doc(a, a.n_docs > 0 ? a.n_docs - 1 : 0);
    }
    for (int64_t d = gid; d < a.n_docs; d += (int64_t)gridDim.x * blockDim.x) {
        const int64_t lo = a.tok_off[d], hi = a.tok_off[d + 1], r0 = a.range_off[d], r1 = a.range_off[d + 1];
        if (lo < 0 || hi < lo || hi > a.n_tokens || r0 < 0 || r1 < r0 || r1 > a.n_ranges) {
            rng_bad_doc(a, d);
            continue;
        }
        if (hi > lo) atomicOr(&a.bits[lo >> 5], 1u << (lo & 31));
        if (r1 > r0) atomicOr(&a.rbits[r0 >> 5], 1u << (r0 & 31));
        if (hi == lo && !a.starts) {  // no ids, no bytes
            if (r1 > r0 && a.ranges[2 * (r1 - 1) + 1] > 0) rng_lowest(a, RNG_H_BEYOND, rng_first_beyond(a, r0, r1, 0));
            if (a.doc_off && a.doc_off[d + 1] != a.doc_off[d]) rng_lowest(a, RNG_H_GAP, d);
        }
    }
}

__global__ __launch_bounds__(RNG_THREADS) void td_rng_check(const RangeArgs a) {
    __shared__ long long s_wave[RNG_THREADS / 64];
    if (a.head[LAB_H_BAD]) return;
    const int tid = threadIdx.x;
    const int64_t nch = (a.n_ranges + RNG_CHUNK - 1) / RNG_CHUNK;
    for (int64_t c = blockIdx.x; c < nch; c += gridDim.x) {
        const int64_t r0 = c * RNG_CHUNK + 4 * tid;
        long long len[4], sum = 0;
        uint32_t first = 0;  // (r0 % 4 == 0: the four bits share a word)
        if (r0 < a.n_ranges) first = (a.rbits[r0 >> 5] >> (r0 & 31)) & 15u;
        long long prev_end = r0 > 0 && r0 < a.n_ranges ? a.ranges[2 * r0 - 1] : 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            len[q] = 0;
            if (r0 + q >= a.n_ranges) continue;
            const longlong2 be = make_longlong2(a.ranges[2 * (r0 + q)], a.ranges[2 * (r0 + q) + 1]);  // (the caller's pointer: 8-byte aligned)
            if (be.x < 0 || be.y < be.x || (!((first >> q) & 1u) && be.x < prev_end)) rng_lowest(a, RNG_H_RANGE, r0 + q);
            else len[q] = be.y - be.x;
            prev_end = be.y;
            sum += len[q];
        }
        long long total;
        long long run = block_excl(sum, s_wave, total);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (r0 + q < a.n_ranges) a.cum[r0 + q] = run;
            run += len[q];
        }
        if (tid == 0) a.rchunks[c] = (unsigned long long)total;
    }
}

__global__ __launch_bounds__(RNG_THREADS) void td_rng_cum(const RangeArgs a) {
    __shared__ long long s_wave[RNG_THREADS / 64];
    if (a.head[LAB_H_BAD]) return;
    long long carry[1];
    chunks_excl_scan<1>(a.rchunks, (a.n_ranges + RNG_CHUNK - 1) / RNG_CHUNK, s_wave, carry);
    if (threadIdx.x == 0) {
        a.head[LAB_H_UNTERM] = (unsigned long long)carry[0];
        if (const unsigned long long bad = a.head[RNG_H_RANGE]) {
            rows_raise(a, TD_E_INVALID, (int64_t)(RNG_TOP - bad));
            a.head[LAB_H_BAD] = 1ull;
        }
    }
}

template <bool STARTS>
__global__ __launch_bounds__(RNG_THREADS) void td_rng_apply(const RangeArgs a) {
    __shared__ uint16_t s_len[RNG_TILE + 2 * (RNG_TILE >> 4) + 2];
    __shared__ int32_t s_tab[RC_LDS_DOCS];
    __shared__ long long s_wb[RNG_WIN], s_we[RNG_WIN], s_wc[RNG_WIN];
    __shared__ uint32_t s_f[RNG_THREADS / 64];
    __shared__ unsigned long long s_s[RNG_THREADS / 64];
    __shared__ long long s_red[RNG_THREADS / 64];
    __shared__ long long s_edge[2];
    __shared__ uint16_t s_tb[RNG_THREADS];
    if (a.head[LAB_H_BAD]) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t total = rng_total(a), ntiles = (total + RNG_TILE - 1) / RNG_TILE;
    const bool ids16 = (((uintptr_t)a.ids) & 15) == 0;
    const auto tok_key = [&](int64_t d) { return a.tok_off[d]; };
    const auto beg_key = [&](int64_t r) { return a.ranges[2 * r]; };
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t t0 = t * RNG_TILE;
        const int tlen = total - t0 < RNG_TILE ? (int)(total - t0) : RNG_TILE;
        __syncthreads();  // (the tile before is done with LDS)
        // ---- ids by int4 (they stay in registers for the labels), their lengths into LDS ---------------------------------------
        int32_t v[4][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = 4 * (tid + RNG_THREADS * k);
            const int64_t p = t0 + j;
            if (p + 4 <= total && ids16) {
                const int4 q = *reinterpret_cast<const int4*>(a.ids + p);
                v[k][0] = q.x; v[k][1] = q.y; v[k][2] = q.z; v[k][3] = q.w;
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) v[k][c] = p + c < total ? a.ids[p + c] : -1;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                uint32_t len = 0;
                if (p + c < total) {
                    len = tok_len(a, v[k][c]);
                    if (STARTS && len == 0) off_bad_token(a, p + c);  // (the covered form: td_off_scan<0> has said so)
                    if (len > 0xFFFFu) { rows_raise(a, TD_E_INVALID, p + c); len = 0xFFFFu; }  // (a token of 64 KiB: no vocabulary has one)
                }
                s_len[len_idx(j + c)] = (uint16_t)len;
            }
        }
        __syncthreads();
        // ---- the lane's sixteen ids: where the first one starts ----------------------------------------------------------------
        const int jb = RNG_PER * tid;
        const int64_t p0 = t0 + jb;
        const int nv = tlen - jb >= RNG_PER ? RNG_PER : tlen - jb > 0 ? tlen - jb : 0;
        uint32_t hb = 0;  // document starts: bit i = the lane's id i, bit 16 = the id behind them
        if (nv > 0) {
            const int64_t w = p0 >> 5;
            hb = (uint32_t)((a.bits[w] | (unsigned long long)a.bits[w + 1] << 32) >> (p0 & 31)) & 0x1FFFFu;
        }
        unsigned long long cur = 0;  // covered form: the start of the next id unless it is a document's first
        long long edge_s, edge_e;    // the lane's first start, its last end
        if constexpr (!STARTS) {
            Seg mine{0u, 0ull};
            for (int i = 0; i < nv; ++i) mine = seg_op(mine, Seg{(hb >> i) & 1u, s_len[len_idx(jb + i)]});
            const Seg incl = wave_scan(mine, lane);
            if (lane == 63) { s_f[wv] = incl.f; s_s[wv] = incl.s; }
            __syncthreads();
            Seg before{0u, a.chunk_sum[t]};
            for (int w = 0; w < wv; ++w) before = seg_op(before, Seg{s_f[w], s_s[w]});
            const uint32_t pf = __shfl_up(incl.f, 1);
            const unsigned long long ps = __shfl_up(incl.s, 1);
            const Seg r = seg_op(before, lane ? Seg{pf, ps} : Seg{0u, 0ull});
            cur = r.s;
            edge_s = (hb & 1u) ? 0ll : (long long)cur;
            edge_e = (long long)seg_op(r, mine).s;
        } else {
            edge_s = nv > 0 ? a.starts[p0] : 0ll;
            edge_e = nv > 0 ? a.starts[p0 + nv - 1] + s_len[len_idx(jb + nv - 1)] : 0ll;
        }
        if (tid == 0) s_edge[0] = edge_s;
        if (nv > 0 && jb + nv == tlen) s_edge[1] = edge_e;
        // ---- the tile's documents, and the window of ranges its ids can touch ------------------------------------------------------
        const int64_t d0 = group_last_le(tok_key, 0, a.n_docs, t0);  // (tok_off[0] = 0 <= t0)
        bool fits;
        const int nd = tile_table(s_tab, tok_key, d0, a.n_docs, t0, 0, RNG_TILE, tlen, fits);  // (its barriers publish s_edge too)
        const int64_t d_last = fits ? d0 + last_le(s_tab, nd, (int32_t)(tlen - 1)) : last_le_global(tok_key, d0, a.n_docs, t0 + tlen - 1);
        const int64_t f0 = a.range_off[d0], f1 = a.range_off[d0 + 1], l0 = a.range_off[d_last], l1 = a.range_off[d_last + 1];
        const int64_t w0 = group_last_le(beg_key, f0, f1, s_edge[0]);
        const int64_t w1 = l1 > l0 ? group_last_le(beg_key, l0, l1, s_edge[1]) + 1 : l0;
        const bool staged = w1 - w0 <= RNG_WIN;
        if (staged) {
            for (int i = tid; i < (int)(w1 - w0); i += RNG_THREADS) {
                const int64_t r = w0 + i;
                const longlong2 be = make_longlong2(a.ranges[2 * r], a.ranges[2 * r + 1]);
                s_wb[i] = be.x;
                s_we[i] = be.y;
                s_wc[i] = a.cum[r] + (long long)a.rchunks[r / RNG_CHUNK];
            }
        }
        __syncthreads();
        // ---- the walk ----------------------------------------------------------------------------------------------------------------
        int it = -1;                      // the current document: d0 + it in s_tab, or d
        int64_t d = -1, lo0 = 0, hi = 0;  // its ranges [lo0, hi) (inside the window when staged)
        int64_t k = -1;                   // the last of them with begin <= the position looked at last (lo0 - 1: none)
        long long kb = 0, ke = 0, kc = 0, base = 0;
        long long prev_e = 0, prev_g = 0;
        bool prev_in = false, have_prev = false;
        uint32_t tb = 0, n_tr = 0, n_pa = 0;
        const auto beg_at = [&](int64_t r) { return staged ? s_wb[r - w0] : a.ranges[2 * r]; };
        // marked bytes in front of x, whether byte x is marked; x does not decrease inside a document
        const auto eval = [&](long long x, long long& g, bool& in) {
            if (k + 1 < hi && beg_at(k + 1) <= x) {
                int64_t lo = k + 1, up = hi;
                while (up - lo > 1) {
                    const int64_t mid = lo + ((up - lo) >> 1);
                    if (beg_at(mid) <= x) lo = mid;
                    else up = mid;
                }
                k = lo;
                if (staged) { kb = s_wb[k - w0]; ke = s_we[k - w0]; kc = s_wc[k - w0]; }
                else { kb = a.ranges[2 * k]; ke = a.ranges[2 * k + 1]; kc = a.cum[k] + (long long)a.rchunks[k / RNG_CHUNK]; }
            }
            if (k < lo0) { g = base; in = false; return; }
            const long long off = x - kb, len = ke - kb;
            g = kc + (off < 0 ? 0 : off > len ? len : off);
            in = x >= kb && x < ke;
        };
        for (int i = 0; i < nv; ++i) {
            const int64_t p = p0 + i;
            const bool head = (hb >> i) & 1u;
            if (i == 0 || head) {  // the id's document and its ranges
                if (fits) {
                    const int32_t x = (int32_t)(jb + i);
                    if (it < 0) it = last_le(s_tab, nd, x);
                    while (it + 1 < nd && s_tab[it + 1] <= x) ++it;
                    d = d0 + it;
                } else {
                    d = last_le_global(tok_key, d < 0 ? d0 : d, a.n_docs, p);
                }
                lo0 = a.range_off[d];
                hi = a.range_off[d + 1];
                if (staged) {
                    lo0 = lo0 > w0 ? lo0 : w0;
                    hi = hi < w1 ? hi : w1;
                }
                k = lo0 - 1;
                base = 0;
                if (lo0 < hi) base = staged ? s_wc[lo0 - w0] : a.cum[lo0] + (long long)a.rchunks[lo0 / RNG_CHUNK];
                have_prev = false;
            }
            const long long len = s_len[len_idx(jb + i)];
            const long long s = STARTS ? a.starts[p] : head ? 0ll : (long long)cur;
            const long long e = s + len;
            cur = (unsigned long long)e;
            long long gs = prev_g, ge;
            bool in_s = prev_in, in_e;
            if (!have_prev || s != prev_e) eval(s, gs, in_s);
            eval(e, ge, in_e);
            prev_e = e; prev_g = ge; prev_in = in_e; have_prev = true;
            const long long m = ge - gs;
            const bool tr = a.rule == TD_RANGE_OVERLAP ? m > 0 : a.rule == TD_RANGE_INSIDE ? m == len : in_s;
            tb |= tr ? 1u << i : 0u;
            n_tr += tr;
            n_pa += m > 0 && m < len;
            if (!STARTS && (p + 1 == total || ((hb >> (i + 1)) & 1u))) {  // the document's last id: e is its covered bytes
                const int64_t r0 = a.range_off[d], r1 = a.range_off[d + 1];
                if (r1 > r0 && a.ranges[2 * (r1 - 1) + 1] > e) rng_lowest(a, RNG_H_BEYOND, rng_first_beyond(a, r0, r1, e));
                if (a.doc_off && a.doc_off[d + 1] - a.doc_off[d] != e) rng_lowest(a, RNG_H_GAP, d);
            }
        }
        s_tb[tid] = (uint16_t)tb;
        if (a.mask && nv > 0) {
            uint8_t* mp = a.mask + p0;
            if (nv == RNG_PER && (((uintptr_t)mp) & 15) == 0) {
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
        // ---- counts (a tile has at most 4096 of each), in td_lab_apply's form --------------------------------------------------------
        const long long packed = (long long)n_tr | (long long)n_pa << 16;
        long long sums;
        if (a.trained_off) {
            const long long incl2 = wave_incl_scan(packed, lane, [](long long x, long long y) { return x + y; });
            if (lane == 63) s_red[wv] = incl2;
            __syncthreads();
            long long before = 0;
            sums = 0;
            for (int w = 0; w < RNG_THREADS / 64; ++w) {
                if (w < wv) before += s_red[w];
                sums += s_red[w];
            }
            a.aux[t * RNG_THREADS + tid] = (uint32_t)((before + incl2 - packed) & 0xFFFF) << 16 | tb;
            if (tid == 0) a.tile_cnt[t] = (unsigned long long)(sums & 0xFFFF);
        } else {
            sums = block_sum(packed, s_red);
        }
        if (tid == 0) {
            if (sums & 0xFFFF) atomicAdd(&a.head[LAB_H_TRAINED], (unsigned long long)(sums & 0xFFFF));
            if ((sums >> 16) & 0xFFFF) atomicAdd(&a.head[LAB_H_SPANS], (unsigned long long)((sums >> 16) & 0xFFFF));
        }
        __syncthreads();  // (s_tb is whole)
        // ---- the labels: the ids still in registers, by the lanes' trained bits ---------------------------------------------------------
#pragma unroll
        for (int k4 = 0; k4 < 4; ++k4) {
            const int j = 4 * (tid + RNG_THREADS * k4);
            const int64_t p = t0 + j;
            if (p >= total) break;
            const uint32_t bits4 = (uint32_t)s_tb[j >> 4] >> (j & 15);
            int32_t o[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) o[c] = (bits4 >> c) & 1u ? v[k4][c] : a.ignore;
            rows_put4(a.labels, p, total, o);
        }
    }
}

// covered form, one lane: what the documents' ends showed (td_rng_docs for those without ids, td_rng_apply for the others)
__global__ void td_rng_status(const RangeArgs a) {
    if (a.head[LAB_H_BAD]) return;
    if (const unsigned long long r = a.head[RNG_H_BEYOND]) rows_raise(a, TD_E_INVALID, (int64_t)(RNG_TOP - r));
    else if (const unsigned long long d = a.head[RNG_H_GAP]) rows_raise(a, TD_E_INVALID, (int64_t)(RNG_TOP - d));
}

}  // namespace

hipError_t launch_range_labels(const RangeArgs& a, hipStream_t stream) {
    const auto grid_of = [](int64_t n, int64_t per, int64_t most) {
        const int64_t g = (n + per - 1) / per;
        return (unsigned)(g < 1 ? 1 : g < most ? g : most);
    };
    hipError_t e;
    hipLaunchKernelGGL(td_rng_docs, dim3(grid_of(a.n_docs, RNG_THREADS, 4096)), dim3(RNG_THREADS), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(td_rng_check, dim3(grid_of(a.n_ranges, RNG_CHUNK, RC_MAX_GRID)), dim3(RNG_THREADS), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(td_rng_cum, dim3(1), dim3(RNG_THREADS), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const unsigned g_tiles = grid_of(a.n_tokens, RNG_TILE, 1 << 20);
    if (a.n_tokens > 0 && !a.starts) {
        StartsArgs s{};
        s.tokens = a.ids;
        s.tok_off = a.tok_off;
        s.n_docs = a.n_docs;
        s.n_bound = a.n_tokens;
        s.len_off = a.len_off;
        s.max_id = a.max_id;
        s.kind = OFF_BYTES;
        s.heads = a.bits;
        s.chunk_sum = a.chunk_sum;
        s.chunk_head = reinterpret_cast<uint32_t*>(a.chunk_sum + (a.n_tokens / OFF_CHUNK + 2));
        s.err = a.err;
        s.err_pos = a.err_pos;
        if ((e = launch_chunk_carries(s, stream)) != hipSuccess) return e;
    }
    if (a.n_tokens > 0) {
        if (a.starts) hipLaunchKernelGGL(td_rng_apply<true>, dim3(g_tiles), dim3(RNG_THREADS), 0, stream, a);
        else hipLaunchKernelGGL(td_rng_apply<false>, dim3(g_tiles), dim3(RNG_THREADS), 0, stream, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (!a.starts) {
        hipLaunchKernelGGL(td_rng_status, dim3(1), dim3(1), 0, stream, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    LabelArgs f{};
    f.tok_off = a.tok_off;
    f.n_docs = a.n_docs;
    f.n_tokens = a.n_tokens;
    f.counts = a.counts;
    f.trained_off = a.trained_off;
    f.head = a.head;
    f.tile_cnt = a.tile_cnt;
    f.aux = a.aux;
    f.err = a.err;
    f.err_pos = a.err_pos;
    return launch_labels_finish(f, stream);
}

}  // namespace td
