// Per-token start offsets (td_token_starts, td_encode_*_with_starts).  The start of id i is where its bytes begin in its
// document: a SEGMENTED exclusive scan of token lengths (or character counts) over the ids, restarted at every document's
// first id.  Patterns that cover every byte need nothing else.  Generic patterns can skip text: a document whose ids cover
// fewer bytes than it has is mapped back through a bitmap of the covered bytes, built from the generic engine's piece-start
// and skipped-stretch bitmaps of the same call, with a two-level (tile, word) rank / select structure.
//
//   launch_token_starts   td_off_heads (bit per document start), launch_chunk_carries, td_off_scan<1> (the starts)
//   launch_chunk_carries  td_off_scan<0> (chunk totals), td_off_carry (one workgroup: carries into the chunks); td_ranges.hip
//                         launches it too, on a bitmap of its own, and redoes the scan inside a chunk in registers
//   launch_encode_starts  td_off_docs (ids against document lengths), for generic patterns td_off_rank_words / td_off_rank_tiles /
//                         td_off_cov_words / td_off_rank_tiles (covered bytes, characters), td_off_finish (gap documents, packed pairs)
#include <hip/hip_runtime.h>

#include "td_common.h"
#include "td_offsets.h"
#include "td_offsets_dev.h"  // Seg, seg_op, wave_scan, off_bad_token, tok_len

namespace td {

namespace {

__device__ __forceinline__ void off_raise(const StartsArgs& a, int code, int64_t pos) {
    if (atomicCAS(a.err, 0, code) == 0) *a.err_pos = pos;
}
__device__ __forceinline__ int64_t off_total(const StartsArgs& a) {
    const int64_t t = a.tok_off[a.n_docs];
    return t < 0 ? 0 : (t < a.n_bound ? t : a.n_bound);
}
__device__ __forceinline__ uint32_t tok_chars(const StartsArgs& a, int32_t id) {
    return (id >= 0 && id <= a.max_id) ? a.ctab[id] : 0u;
}

// A chunk of OFF_CHUNK ids, four a lane: the segmented scan inside the chunk.  Pass 0 writes the chunk's total, pass 1 the
// starts with the carry td_off_carry left in chunk_sum.
template <int PASS>
__global__ __launch_bounds__(1024) void td_off_scan(const StartsArgs a) {
    __shared__ uint32_t s_f[16];
    __shared__ unsigned long long s_s[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t total = off_total(a);
    const int64_t nchunks = (total + OFF_CHUNK - 1) / OFF_CHUNK;
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int64_t e0 = c * OFF_CHUNK + tid * 4;
        int32_t ids[4] = {-1, -1, -1, -1};
        if (e0 + 4 <= total && (((uintptr_t)a.tokens) & 15) == 0) {
            const int4 q = *reinterpret_cast<const int4*>(a.tokens + e0);
            ids[0] = q.x; ids[1] = q.y; ids[2] = q.z; ids[3] = q.w;
        } else {
            for (int k = 0; k < 4; ++k)
                if (e0 + k < total) ids[k] = a.tokens[e0 + k];
        }
        const uint32_t hw = e0 < total ? (a.heads[e0 >> 5] >> (e0 & 31)) & 15u : 0u;  // (e0 % 4 == 0: the four bits share a word)
        unsigned long long v[4];
        uint32_t cont[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = 0; cont[k] = 0;
            if (e0 + k >= total) continue;
            const uint32_t len = a.kind != OFF_CHARS ? tok_len(a, ids[k]) : 1u;
            const uint32_t ch = a.kind != OFF_BYTES ? tok_chars(a, ids[k]) : 1u;
            if (PASS == 0 && (len == 0 || ch == 0)) off_bad_token(a, e0 + k);
            cont[k] = ch & 1u;
            v[k] = a.kind == OFF_BYTES ? len : a.kind == OFF_CHARS ? (ch >> 1) : ((unsigned long long)(ch >> 1) << 32 | len);
        }
        Seg mine{0u, 0ull};
#pragma unroll
        for (int k = 0; k < 4; ++k) mine = seg_op(mine, Seg{(hw >> k) & 1u, v[k]});
        const Seg incl = wave_scan(mine, lane);
        if (lane == 63) { s_f[wv] = incl.f; s_s[wv] = incl.s; }
        __syncthreads();
        Seg before{0u, 0ull};  // the waves in front of this one
        for (int w = 0; w < wv; ++w) before = seg_op(before, Seg{s_f[w], s_s[w]});
        if (PASS == 0) {
            if (tid == 1023) {
                const Seg all = seg_op(before, incl);
                a.chunk_sum[c] = all.s;
                a.chunk_head[c] = all.f;
            }
        } else {
            const uint32_t pf = __shfl_up(incl.f, 1);
            const unsigned long long ps = __shfl_up(incl.s, 1);
            Seg r = seg_op(Seg{0u, a.chunk_sum[c]}, seg_op(before, lane ? Seg{pf, ps} : Seg{0u, 0ull}));
            long long o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t h = (hw >> k) & 1u;
                const unsigned long long e = h ? 0ull : r.s;
                r = seg_op(r, Seg{h, v[k]});
                o[k] = a.kind == OFF_CHARS ? ((long long)e - (long long)cont[k] > 0 ? (long long)e - (long long)cont[k] : 0ll) : (long long)e;
            }
            if (e0 + 4 <= total && (((uintptr_t)a.out) & 15) == 0) {
                *reinterpret_cast<longlong2*>(a.out + e0) = make_longlong2(o[0], o[1]);
                *reinterpret_cast<longlong2*>(a.out + e0 + 2) = make_longlong2(o[2], o[3]);
            } else {
                for (int k = 0; k < 4; ++k)
                    if (e0 + k < total) a.out[e0 + k] = o[k];
            }
        }
        __syncthreads();  // (s_f / s_s are rewritten by the next chunk)
    }
}

// one workgroup: exclusive segmented scan of the chunk totals, in place (the carry into every chunk)
__global__ __launch_bounds__(1024) void td_off_carry(const StartsArgs a) {
    __shared__ uint32_t s_f[16];
    __shared__ unsigned long long s_s[16];
    __shared__ uint32_t s_cf;
    __shared__ unsigned long long s_cs;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t nchunks = (off_total(a) + OFF_CHUNK - 1) / OFF_CHUNK;
    if (tid == 0) { s_cf = 0; s_cs = 0; }
    __syncthreads();
    for (int64_t c0 = 0; c0 < nchunks; c0 += 1024) {
        const int64_t c = c0 + tid;
        const Seg x = c < nchunks ? Seg{a.chunk_head[c], a.chunk_sum[c]} : Seg{0u, 0ull};
        const Seg incl = wave_scan(x, lane);
        if (lane == 63) { s_f[wv] = incl.f; s_s[wv] = incl.s; }
        __syncthreads();
        Seg before{s_cf, s_cs};
        for (int w = 0; w < wv; ++w) before = seg_op(before, Seg{s_f[w], s_s[w]});
        const uint32_t pf = __shfl_up(incl.f, 1);
        const unsigned long long ps = __shfl_up(incl.s, 1);
        const Seg ex = seg_op(before, lane ? Seg{pf, ps} : Seg{0u, 0ull});
        if (c < nchunks) a.chunk_sum[c] = ex.s;
        __syncthreads();
        if (tid == 1023) { const Seg all = seg_op(before, incl); s_cf = all.f; s_cs = all.s; }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void td_off_heads(const StartsArgs a) {
    const int64_t total = off_total(a);
    const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (gid == 0 && a.tok_off[a.n_docs] > a.n_bound) off_raise(a, TD_E_CAPACITY, a.tok_off[a.n_docs]);
    for (int64_t d = gid; d < a.n_docs; d += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t0 = a.tok_off[d], t1 = a.tok_off[d + 1];
        if (t0 >= 0 && t0 < t1 && t0 < total) atomicOr(&a.heads[t0 >> 5], 1u << (t0 & 31));
    }
}

// ---- encode: documents against their lengths ---------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long start_bytes(const StartsArgs& a, int64_t v) {
    return a.kind == OFF_PAIR ? (unsigned long long)v & 0xFFFFFFFFull : (unsigned long long)v;
}

__global__ __launch_bounds__(256) void td_off_docs(const StartsArgs a) {
    const int64_t total = off_total(a);
    for (int64_t d = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; d < a.n_docs; d += (int64_t)gridDim.x * blockDim.x) {
        int64_t t0 = a.tok_off[d], t1 = a.tok_off[d + 1];
        t0 = t0 < 0 ? 0 : (t0 > total ? total : t0);
        t1 = t1 < t0 ? t0 : (t1 > total ? total : t1);
        unsigned long long covered = 0;
        if (t1 > t0) covered = start_bytes(a, a.out[t1 - 1]) + tok_len(a, a.tokens[t1 - 1]);
        const unsigned long long len = (unsigned long long)(a.doc_off[d + 1] - a.doc_off[d]);
        const bool gap = covered < len;
        a.doc_gap[d] = gap ? 1 : 0;
        if (covered > len || (gap && !a.generic)) off_raise(a, TD_E_INVALID, a.doc_off[d]);  // (the pattern covers every byte: cannot happen)
    }
}

// ---- rank / select over the text -----------------------------------------------------------------------------------------
// 128 lanes, one bitmap word each (one tile): exclusive scans inside the workgroup
__device__ __forceinline__ uint32_t blk128_excl_sum(uint32_t x, uint32_t* s2, uint32_t& total) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint32_t y = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(y, d);
        if (lane >= d) y += t;
    }
    if (lane == 63) s2[wv] = y;
    __syncthreads();
    const uint32_t r = (wv ? s2[0] : 0u) + y - x;
    total = s2[0] + s2[1];
    __syncthreads();
    return r;
}
__device__ __forceinline__ uint32_t blk128_excl_max(uint32_t x, uint32_t* s2, uint32_t& all) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint32_t y = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(y, d);
        if (lane >= d) y = y > t ? y : t;
    }
    if (lane == 63) s2[wv] = y;
    __syncthreads();
    uint32_t ex = __shfl_up(y, 1);
    if (lane == 0) ex = 0;
    if (wv) ex = ex > s2[0] ? ex : s2[0];
    all = s2[0] > s2[1] ? s2[0] : s2[1];
    __syncthreads();
    return ex;
}
// the kind of the last piece start in a word: 1 a piece with tokens, 2 a skipped stretch, 0 none
__device__ __forceinline__ uint32_t word_kind(uint32_t s, uint32_t g) {
    if (!s) return 0u;
    const int top = 31 - __builtin_clz(s);
    return ((g >> top) & 1u) ? 2u : 1u;
}

// per tile: the kind of its last piece start (covered bytes), its non-continuation bytes (characters)
__global__ __launch_bounds__(128) void td_off_rank_words(const StartsArgs a, int need_cov, int need_nc) {
    __shared__ uint32_t s2[2];
    const int64_t nw = (a.n + 31) >> 5, ntiles = (a.n + OFF_TILE - 1) / OFF_TILE;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t w = tile * (OFF_TILE / 32) + threadIdx.x;
        if (need_cov) {
            const uint32_t k = w < nw ? word_kind(a.startbits[w], a.gapbits[w]) : 0u;
            uint32_t all;
            (void)blk128_excl_max(k ? ((threadIdx.x + 1u) << 2 | k) : 0u, s2, all);
            if (threadIdx.x == 0) a.tile_kind[tile] = all & 3u;
        }
        if (need_nc) {
            uint32_t m = 0;
            if (w < nw) {
                const int64_t b0 = w * 32;
                if (b0 + 32 <= a.n && (((uintptr_t)a.text) & 15) == 0) {
                    const uint4* p = reinterpret_cast<const uint4*>(a.text + b0);
                    const uint4 q0 = p[0], q1 = p[1];
                    const uint32_t q[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
                    for (int j = 0; j < 8; ++j)
#pragma unroll
                        for (int b = 0; b < 4; ++b)
                            if (((q[j] >> (8 * b)) & 0xC0u) != 0x80u) m |= 1u << (4 * j + b);
                } else {
                    for (int b = 0; b < 32 && b0 + b < a.n; ++b)
                        if ((a.text[b0 + b] & 0xC0u) != 0x80u) m |= 1u << b;
                }
                a.ncbits[w] = m;
            }
            uint32_t tot;
            const uint32_t ex = blk128_excl_sum((uint32_t)__popc(m), s2, tot);
            if (w < nw) a.nc_wpref[w] = (uint16_t)ex;
            if (threadIdx.x == 0) a.nc_tpref[tile] = tot;
        }
    }
}

// one workgroup over the tiles.  phase 0: the kind in force at every tile's start (exclusive max over (tile + 1) << 2 | kind) and the
// character prefix; phase 1: the covered-byte prefix
__global__ __launch_bounds__(1024) void td_off_rank_tiles(const StartsArgs a, int phase, int need_cov, int need_nc) {
    __shared__ unsigned long long s_w[16];
    __shared__ unsigned long long s_carry;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t ntiles = (a.n + OFF_TILE - 1) / OFF_TILE;
    for (int part = 0; part < 2; ++part) {
        const bool kinds = phase == 0 && part == 0;
        int64_t* pref = phase == 0 ? a.nc_tpref : a.cov_tpref;
        if (phase == 0 && ((part == 0 && !need_cov) || (part == 1 && !need_nc))) continue;
        if (phase == 1 && part == 1) break;
        if (tid == 0) s_carry = 0;
        __syncthreads();
        for (int64_t t0 = 0; t0 < ntiles; t0 += 1024) {
            const int64_t t = t0 + tid;
            unsigned long long x = 0;
            if (t < ntiles) x = kinds ? (a.tile_kind[t] ? ((unsigned long long)(t + 1) << 2 | a.tile_kind[t]) : 0ull) : (unsigned long long)pref[t];
            unsigned long long y = x;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned long long u = __shfl_up(y, d);
                if (lane >= d) y = kinds ? (y > u ? y : u) : y + u;
            }
            if (lane == 63) s_w[wv] = y;
            __syncthreads();
            unsigned long long before = s_carry;
            for (int w = 0; w < wv; ++w) before = kinds ? (before > s_w[w] ? before : s_w[w]) : before + s_w[w];
            unsigned long long ex = __shfl_up(y, 1);
            if (lane == 0) ex = 0;
            ex = kinds ? (before > ex ? before : ex) : before + ex;
            if (t < ntiles) {
                if (kinds) a.tile_kind[t] = (uint32_t)(ex & 3u);
                else pref[t] = (int64_t)ex;
            }
            __syncthreads();
            if (tid == 1023) s_carry = kinds ? (before > y ? before : y) : before + y;
            __syncthreads();
        }
        if (!kinds && tid == 0) pref[ntiles] = (int64_t)s_carry;
        __syncthreads();
    }
}

// per tile: the covered-byte bitmap (a byte is covered unless the last piece start at or in front of it is a skipped stretch;
// the first byte of a document always carries a start) and its word / tile counts
__global__ __launch_bounds__(128) void td_off_cov_words(const StartsArgs a) {
    __shared__ uint32_t s2[2];
    const int64_t nw = (a.n + 31) >> 5, ntiles = (a.n + OFF_TILE - 1) / OFF_TILE;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t w = tile * (OFF_TILE / 32) + threadIdx.x;
        const uint32_t s = w < nw ? a.startbits[w] : 0u, g = w < nw ? a.gapbits[w] : 0u;
        const uint32_t k = word_kind(s, g);
        uint32_t all;
        const uint32_t ex = blk128_excl_max(k ? ((threadIdx.x + 1u) << 2 | k) : 0u, s2, all);
        uint32_t in_gap = ex ? ((ex & 3u) == 2u) : (a.tile_kind[tile] == 2u);
        uint32_t cov = 0;
        int at = 0;
        for (uint32_t m = s; m; m &= m - 1u) {
            const int b = __builtin_ctz(m);
            if (!in_gap && b > at) cov |= (uint32_t)(((1ull << b) - 1ull) & ~((1ull << at) - 1ull));
            in_gap = (g >> b) & 1u;
            at = b;
        }
        if (!in_gap) cov |= (uint32_t)(0xFFFFFFFFull & ~((1ull << at) - 1ull));
        if (w * 32 + 32 > a.n) cov &= w * 32 >= a.n ? 0u : (uint32_t)((1ull << (a.n - w * 32)) - 1ull);
        if (w < nw) a.covbits[w] = cov;
        uint32_t tot;
        const uint32_t wp = blk128_excl_sum((uint32_t)__popc(cov), s2, tot);
        if (w < nw) a.cov_wpref[w] = (uint16_t)wp;
        if (threadIdx.x == 0) a.cov_tpref[tile] = tot;
    }
}

__device__ __forceinline__ int64_t rank_at(const uint32_t* bits, const uint16_t* wpref, const int64_t* tpref, int64_t p) {
    const int64_t w = p >> 5;
    return tpref[p / OFF_TILE] + wpref[w] + __popc(bits[w] & ((1u << (p & 31)) - 1u));
}
// position of the k-th covered byte (0-based), -1 if there are not that many
__device__ __forceinline__ int64_t cov_select(const StartsArgs& a, int64_t k) {
    const int64_t ntiles = (a.n + OFF_TILE - 1) / OFF_TILE, nw = (a.n + 31) >> 5;
    if (k < 0 || k >= a.cov_tpref[ntiles]) return -1;
    int64_t lo = 0, hi = ntiles;  // cov_tpref[lo] <= k < cov_tpref[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (a.cov_tpref[mid] <= k) lo = mid; else hi = mid;
    }
    const uint32_t r = (uint32_t)(k - a.cov_tpref[lo]);
    int64_t wl = lo * (OFF_TILE / 32), wh = wl + OFF_TILE / 32;
    if (wh > nw) wh = nw;
    while (wh - wl > 1) {  // last word of the tile whose prefix is <= r
        const int64_t mid = (wl + wh) >> 1;
        if (a.cov_wpref[mid] <= r) wl = mid; else wh = mid;
    }
    uint32_t m = a.covbits[wl];
    for (uint32_t j = r - a.cov_wpref[wl]; j; --j) m &= m - 1u;
    return wl * 32 + __builtin_ctz(m);
}
__device__ __forceinline__ int64_t chars_at(const StartsArgs& a, int64_t o0, int64_t p) {  // tiktoken's rule, in the source text
    const int64_t c = rank_at(a.ncbits, a.nc_wpref, a.nc_tpref, p) - rank_at(a.ncbits, a.nc_wpref, a.nc_tpref, o0) -
                      ((a.text[p] & 0xC0u) == 0x80u ? 1 : 0);
    return c > 0 ? c : 0;
}

// Four ids a lane.  OFF_PAIR in a covered document: the character start.  A document with skipped text (generic patterns):
// the id's byte position among the covered bytes -> the covered byte it is -> its source position (bytes) or characters
// in front of it.  convert: out holds document-relative byte starts of every document -> characters.
__global__ __launch_bounds__(256) void td_off_finish(const StartsArgs a, int convert) {
    const int64_t total = off_total(a);
    const bool by_doc = a.generic || convert;
    for (int64_t e0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) * 4; e0 < total; e0 += (int64_t)gridDim.x * blockDim.x * 4) {
        int64_t d = 0;
        if (by_doc) {  // the document of id e0: the last one whose first id is <= e0 (behind empty ones)
            int64_t lo = 0, hi = a.n_docs;
            while (hi - lo > 1) {
                const int64_t mid = (lo + hi) >> 1;
                if (a.tok_off[mid] <= e0) lo = mid; else hi = mid;
            }
            d = lo;
        }
        for (int64_t i = e0; i < e0 + 4 && i < total; ++i) {
            if (by_doc) while (d + 1 < a.n_docs && a.tok_off[d + 1] <= i) ++d;
            const int64_t v = a.out[i];
            if (convert || (a.generic && a.doc_gap[d])) {
                const int64_t o0 = a.doc_off[d], o1 = a.doc_off[d + 1];
                int64_t p;
                if (convert) p = o0 + v;
                else {
                    const int64_t k = rank_at(a.covbits, a.cov_wpref, a.cov_tpref, o0) + (int64_t)start_bytes(a, v);
                    p = cov_select(a, k);
                }
                if (p < o0 || p >= o1) { off_raise(a, TD_E_INVALID, o0); continue; }
                a.out[i] = a.chars ? chars_at(a, o0, p) : p - o0;
            } else if (a.kind == OFF_PAIR) {
                const long long c = (long long)((unsigned long long)v >> 32) - (long long)(tok_chars(a, a.tokens[i]) & 1u);
                a.out[i] = c > 0 ? c : 0;
            }
        }
    }
}

int off_blocks(int64_t work, int64_t per_block, int64_t most) {
    int64_t b = (work + per_block - 1) / per_block;
    if (b > most) b = most;
    return b < 1 ? 1 : (int)b;
}

}  // namespace

size_t off_rank_bytes(int64_t n) {
    const size_t nw = (size_t)((n + 31) >> 5) + 1, nt = (size_t)((n + OFF_TILE - 1) / OFF_TILE) + 2;
    return 2 * nw * 4 + 2 * ((nw * 2 + 15) & ~(size_t)15) + 2 * nt * 8 + nt * 4 + 64;
}
void off_rank_layout(StartsArgs& a, void* base, int64_t n) {
    const size_t nw = (size_t)((n + 31) >> 5) + 1, nt = (size_t)((n + OFF_TILE - 1) / OFF_TILE) + 2;
    char* p = (char*)base;
    a.cov_tpref = (int64_t*)p; p += nt * 8;
    a.nc_tpref = (int64_t*)p; p += nt * 8;
    a.covbits = (uint32_t*)p; p += nw * 4;
    a.ncbits = (uint32_t*)p; p += nw * 4;
    a.tile_kind = (uint32_t*)p; p += nt * 4;
    p = (char*)(((uintptr_t)p + 15) & ~(uintptr_t)15);
    a.cov_wpref = (uint16_t*)p; p += (nw * 2 + 15) & ~(size_t)15;
    a.nc_wpref = (uint16_t*)p;
}

hipError_t launch_chunk_carries(const StartsArgs& a, hipStream_t stream) {
    if (a.n_bound <= 0) return hipSuccess;
    hipLaunchKernelGGL(td_off_scan<0>, dim3(off_blocks(a.n_bound, OFF_CHUNK, 2048)), dim3(1024), 0, stream, a);
    hipLaunchKernelGGL(td_off_carry, dim3(1), dim3(1024), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_token_starts(const StartsArgs& a, hipStream_t stream) {
    const hipError_t me = hipMemsetAsync(a.heads, 0, (size_t)(a.n_bound / 32 + 2) * 4, stream);
    if (me != hipSuccess) return me;
    hipLaunchKernelGGL(td_off_heads, dim3(off_blocks(a.n_docs, 256, 4096)), dim3(256), 0, stream, a);
    if (a.n_bound <= 0) return hipGetLastError();
    const hipError_t ce = launch_chunk_carries(a, stream);
    if (ce != hipSuccess) return ce;
    hipLaunchKernelGGL(td_off_scan<1>, dim3(off_blocks(a.n_bound, OFF_CHUNK, 2048)), dim3(1024), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_encode_starts(const StartsArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(td_off_docs, dim3(off_blocks(a.n_docs, 256, 4096)), dim3(256), 0, stream, a);
    if (a.generic) {
        const int tb = off_blocks(a.n, OFF_TILE, 16384);
        hipLaunchKernelGGL(td_off_rank_words, dim3(tb), dim3(128), 0, stream, a, 1, a.chars);
        hipLaunchKernelGGL(td_off_rank_tiles, dim3(1), dim3(1024), 0, stream, a, 0, 1, a.chars);
        hipLaunchKernelGGL(td_off_cov_words, dim3(tb), dim3(128), 0, stream, a);
        hipLaunchKernelGGL(td_off_rank_tiles, dim3(1), dim3(1024), 0, stream, a, 1, 1, 0);
    }
    if (a.generic || a.kind == OFF_PAIR)
        hipLaunchKernelGGL(td_off_finish, dim3(off_blocks(a.n_bound, 1024, 8192)), dim3(256), 0, stream, a, 0);
    return hipGetLastError();
}

hipError_t launch_chars_by_rank(const StartsArgs& a, hipStream_t stream) {
    const int tb = off_blocks(a.n, OFF_TILE, 16384);
    hipLaunchKernelGGL(td_off_rank_words, dim3(tb), dim3(128), 0, stream, a, 0, 1);
    hipLaunchKernelGGL(td_off_rank_tiles, dim3(1), dim3(1024), 0, stream, a, 0, 0, 1);
    hipLaunchKernelGGL(td_off_finish, dim3(off_blocks(a.n_bound, 1024, 8192)), dim3(256), 0, stream, a, 1);
    return hipGetLastError();
}

}  // namespace td
