// Word-list matches (td_word_matches_device and what ends in it): text + document offsets + a word set -> stats[n_docs][WL_COLS],
// totals and the entries' hits.  The rule is the contract in include/tokendagger_hip.h; td_wordlist_args.h has the byte classes, the
// fold, the hash and the table's word, which the set's builder and the host statement (td_word_matches_host) compile too.
//
// The windows, the tiles, the offsets check and the tile's table of documents are the text passes' frame (td_rewrite_common.h); this pass
// only reads the text.  What is its own: an entry is at most 64 bytes, so a tile decides every occurrence that STARTS in it from its own
// bytes, one byte in front and max_len bytes behind.  Nothing is exchanged between tiles and nothing is carried.  A call is
//   td_wl_docs      the frame's offsets check
//   td_wl_reset     stats 0 with FIRST_HIT all ones (which is -1), totals and entry_hits 0
//   td_wl_tiles<R>  a workgroup a tile.  The lanes load their windows and put them, with the halo, into LDS.  A lane makes the 16-bit
//                   mask of its window's word bytes by dword tests (ma_in, ma_eq, ma_pack), takes the byte in front from the lane in
//                   front (from LDS at a wavefront's first lane), and with the documents that start in the window has its START bits.
//                   A workgroup scan of the popcounts places the starts in a list in LDS (WL_LIST at a sweep), and the lanes take them
//                   from there one at a time: prose has a start every six bytes, a run of punctuation one a byte, and a lane that walked
//                   its own window's starts would wait for the slowest window.  Under TD_WL_ANYWHERE every byte is a start and the lanes
//                   stride over the bytes.  THE WALK of a wavefront is in step: at length L every lane that is still inside its document
//                   and below max_len folds one more byte from LDS into its hash; where L is a length of the set and the byte behind is
//                   an END (the edge or no word byte; the byte is the next one of the walk, so it is classed as it is read and no END
//                   mask is kept), the lane probes the table and, on a tag it knows, compares the entry's bytes.  R = 1: the set's blob
//                   was copied into LDS by the workgroup and is probed there; R = 0: it is probed in global memory.  A lane keeps the
//                   sums of the document it is in; at the tile's end a workgroup whose tile lies in one document reduces them a
//                   wavefront by shuffles; what is left goes to a table in LDS (the tile's first WL_SLOTS documents: add, OR, minimum)
//                   and from there, or at once for later documents, to stats by 64-bit atomics: one flush a document and tile.
//                   entry_hits gets one add for all lanes of a wavefront that hit the same entry at the same step: to global memory, or,
//                   for a set of at most WL_FEW entries, to the workgroup's counters in LDS, which it flushes once at its end.
//   td_wl_totals    a lane a document: sums, the OR of GROUPS and the documents with a hit into totals
// Nothing outside text[0, doc_off[n_docs]) and doc_off[0, n_docs] is read.  Only stores (td_wl_reset), adds, ORs and minima touch the
// outputs: the results do not depend on the order of the lanes, nor on the hash.
#include <hip/hip_runtime.h>

#include "td_rewrite_common.h"
#include "td_wordlist.h"

namespace td {

namespace {

constexpr int WL_WAVES = RW_THREADS / 64;
constexpr int WL_SLOTS = 32;   // documents of a tile whose sums meet in LDS
constexpr int WL_FRONT = 16;   // s_txt[WL_FRONT + r]: byte r of the tile; s_txt[WL_FRONT - 1]: the byte in front of it
constexpr int WL_TXT = WL_FRONT + RW_TILE + WL_ENTRY_BYTES + 16;
constexpr int WL_FEW = 64;     // a set of at most this many entries (stop words) counts its entries' hits in LDS: every few words is a hit, and
                               // adds from every wavefront to eight words of global memory are served one after the other
constexpr int WL_MAX_GRID = 2048;  // eight workgroups a CU: a workgroup copies a resident set once and strides over its tiles
static_assert(WL_LIST % RW_THREADS == 0 && RW_TILE <= 65536, "a sweep is whole steps of the workgroup; a start is 16 bits");
static_assert(RC_LDS_DOCS * 4 + WL_TXT + WL_LIST * 2 + WL_SLOTS * WL_COLS * 8 + WL_FEW * 8 + WL_LDS_BYTES + 256 <= 160 * 1024 / 4, "four workgroups a CU");

__device__ __forceinline__ void wl_add(unsigned long long* p, unsigned long long v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void wl_or(unsigned long long* p, unsigned long long v) {
    __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void wl_min(unsigned long long* p, unsigned long long v) {
    __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(RW_THREADS) void td_wl_docs(const WlArgs a) {
    rewrite_docs(a, blockIdx.x * (int64_t)blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

__global__ __launch_bounds__(RW_THREADS) void td_wl_reset(const WlArgs a) {
    if (a.head[RW_H_BAD]) return;
    const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    if (a.totals && gid < WL_COLS) a.totals[gid] = 0;
    if (a.entry_hits)
        for (int64_t i = gid; i < (int64_t)a.set.n_entries; i += step) a.entry_hits[i] = 0;
    for (int64_t i = gid; i < a.n_docs * WL_COLS; i += step) a.stats[i] = (i & (WL_COLS - 1)) == WL_FIRST_HIT ? ~0ull : 0ull;
}
static_assert((WL_COLS & (WL_COLS - 1)) == 0, "td_wl_reset: a column is the index's low bits");

// a lane's sums for the document it is in
struct WlAcc {
    int64_t D;
    unsigned long long hits, groups, first, bytes;
};

// the set's words and bytes: in LDS (R = 1) or where the blob lies
template <int R>
__device__ __forceinline__ uint32_t wl_w(const uint32_t* s_set, const uint32_t* blob, uint32_t i) {
    if constexpr (R) return s_set[i];
    else return blob[i];
}
template <int R>
__device__ __forceinline__ uint32_t wl_b(const uint32_t* s_set, const uint32_t* blob, uint32_t i) {
    if constexpr (R) return reinterpret_cast<const uint8_t*>(s_set)[i];
    else return reinterpret_cast<const uint8_t*>(blob)[i];
}

// The entry that equals the L folded bytes at tx, whose hash is h, or -1.  The tag says where to look; the bytes decide.
template <int R>
__device__ __forceinline__ int wl_probe(const WlSet& S, const uint32_t* s_set, const uint8_t* tx, int L, uint32_t h, bool fold) {
    const uint32_t x = wl_finish(h, L), tag = wl_tag(x);
#pragma unroll 1
    for (uint32_t at = x & S.slot_mask;; at = (at + 1) & S.slot_mask) {  // (at most half the slots are taken: an empty one ends it)
        const uint32_t v = wl_w<R>(s_set, S.blob, at);
        if (!v) return -1;
        if ((v >> 16) != tag) continue;
        const uint32_t e = v & 0xFFFFu, o = wl_w<R>(s_set, S.blob, S.off_at + e);
        if (wl_w<R>(s_set, S.blob, S.off_at + e + 1) - o != (uint32_t)L) continue;
        bool same = true;
#pragma unroll 1
        for (int j = 0; j < L && same; ++j) same = wl_b<R>(s_set, S.blob, 4 * S.bytes_at + o + j) == wl_fold(tx[j], fold);
        if (same) return (int)e;  // (the entries are distinct: no other one can equal these bytes)
    }
}

template <int R>
__global__ __launch_bounds__(RW_THREADS) void td_wl_tiles(const WlArgs a) {
    __shared__ int32_t s_off[RC_LDS_DOCS];
    __shared__ __attribute__((aligned(16))) uint8_t s_txt[WL_TXT];
    __shared__ uint16_t s_list[WL_LIST];
    __shared__ unsigned long long s_acc[WL_SLOTS * WL_COLS];
    __shared__ long long s_red[WL_WAVES];
    __shared__ uint32_t s_first[8];
    __shared__ unsigned long long s_hits[WL_FEW];  // the entries' hits of this workgroup, where the set has at most WL_FEW entries
    __shared__ uint32_t s_set[R ? WL_LDS_BYTES / 4 : 1];
    if (rewrite_bad_offsets(a, true)) return;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 8) s_first[tid] = a.set.first[tid];
    if (tid < WL_FEW) s_hits[tid] = 0;
    const bool few = a.set.n_entries <= (uint32_t)WL_FEW;
    if constexpr (R)
        for (uint32_t i = tid; i < a.set.blob_words; i += RW_THREADS) s_set[i] = a.set.blob[i];
    for (int i = tid; i < WL_SLOTS * WL_COLS; i += RW_THREADS) s_acc[i] = (i & (WL_COLS - 1)) == WL_FIRST_HIT ? ~0ull : 0ull;
    const int64_t total = a.doc_off[a.n_docs];
    const int shift = (int)(((uintptr_t)a.text) & 15);
    const int64_t ntiles = total > 0 ? (total + shift + RW_TILE - 1) / RW_TILE : 0;
    const bool fold = (a.set.flags & WL_FOLD) != 0, anywhere = (a.set.flags & WL_ANYWHERE) != 0;
    const int max_len = (int)a.set.max_len, halo = (max_len + 15) >> 4;  // (windows behind the tile)
    const uint64_t lengths = a.set.lengths;
    const auto off_of = [off = a.doc_off](int64_t d) { return off[d]; };
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const RwTile tl = rw_tile(t, shift, total);
        const int64_t b0 = tl.base + 16 * tid, b = b0 < 0 ? 0 : b0, we = b0 + 16 < total ? b0 + 16 : total;
        const bool owns = b < we;
        const int k0 = (int)(b - b0), k1 = (int)(we - b0);
        uint32_t w[4] = {0, 0, 0, 0};
        if (owns) rw_load(a.text, b0, b, we, w);
        __syncthreads();  // (the tile before has read its bytes, table and list and emptied s_acc; s_first, s_set and s_acc are written)
        *reinterpret_cast<uint4*>(s_txt + WL_FRONT + 16 * tid) = make_uint4(w[0], w[1], w[2], w[3]);
        if (tid < halo) {  // what lies outside the text is 0 here and is never a byte of an occurrence: the document's end comes first
            const int64_t x0 = tl.base + RW_TILE + 16 * tid, xe = x0 + 16 < total ? x0 + 16 : total;
            uint32_t xw[4] = {0, 0, 0, 0};
            if (x0 < xe) rw_load(a.text, x0, x0, xe, xw);
            *reinterpret_cast<uint4*>(s_txt + WL_FRONT + RW_TILE + 16 * tid) = make_uint4(xw[0], xw[1], xw[2], xw[3]);
        }
        if (tid == 8) s_txt[WL_FRONT - 1] = tl.base > 0 ? a.text[tl.base - 1] : (uint8_t)0;
        const RwTable tb = rw_table(s_off, off_of, a.n_docs, tl);
        __syncthreads();
        // the common case: the whole tile lies in one document
        const int64_t ds0 = a.doc_off[tb.kb], de0 = a.doc_off[tb.kb + 1];
        const bool uni = ds0 <= tl.t0 && de0 >= tl.s1;
        // ---- the START bits: the byte in front is the edge or no word byte ----
        const uint32_t whole = owns ? ((1u << k1) - 1u) & ~((1u << k0) - 1u) : 0u;
        uint32_t starts = whole;
        if (!anywhere) {
            uint32_t wm = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t x = w[j];
                wm |= ma_pack(ma_in(x, '0', '9') | ma_in(x | 0x20202020u, 'a', 'z') | ma_eq(x, '_') | (x & 0x80808080u)) << 4 * j;
            }
            uint32_t pred = (__shfl(wm, (lane + 63) & 63) >> 15) & 1u;
            if (lane == 0) pred = wl_word(s_txt[WL_FRONT + 16 * tid - 1]);
            uint32_t dstart = 0;
            if (owns && uni) {
                if (b == ds0) dstart = 1u << k0;
            } else if (owns) {
                for (int64_t k = rw_doc_of(a.doc_off, s_off, tb, tl.t0, b); k <= a.n_docs; ++k) {
                    const int64_t s = a.doc_off[k];
                    if (s >= we) break;
                    if (s >= b) dstart |= 1u << (int)(s - b0);
                }
            }
            starts = (~(wm << 1 | pred) | dstart) & whole;
        }
        long long n_starts = tl.s1 - tl.t0;
        const long long at = anywhere ? 0 : block_excl(__builtin_popcount(starts), s_red, n_starts);
        const int sweep = anywhere ? RW_TILE : WL_LIST, r_first = (int)(tl.t0 - tl.base);
        WlAcc A = {-1, 0, 0, ~0ull, 0};
        const auto put = [&](const WlAcc& X) {
            const int64_t slot = X.D - tb.kb;
            if (slot < WL_SLOTS) {
                atomicAdd(&s_acc[slot * WL_COLS + WL_HITS], X.hits);
                atomicOr(&s_acc[slot * WL_COLS + WL_GROUPS], X.groups);
                atomicMin(&s_acc[slot * WL_COLS + WL_FIRST_HIT], X.first);
                atomicAdd(&s_acc[slot * WL_COLS + WL_HIT_BYTES], X.bytes);
            } else {
                unsigned long long* row = a.stats + X.D * WL_COLS;
                wl_add(row + WL_HITS, X.hits);
                wl_or(row + WL_GROUPS, X.groups);
                wl_min(row + WL_FIRST_HIT, X.first);
                wl_add(row + WL_HIT_BYTES, X.bytes);
            }
        };
#pragma unroll 1
        for (long long s0 = 0; s0 < n_starts; s0 += sweep) {  // (n_starts, and so every trip count below, is the same in every lane)
            const int m = (int)(n_starts - s0 < sweep ? n_starts - s0 : sweep);
            if (!anywhere) {
                if (s0 > 0) __syncthreads();  // (the sweep before has read the list)
                long long q = at - s0;
                for (uint32_t x = starts; x; x &= x - 1, ++q)
                    if (q >= 0 && q < WL_LIST) s_list[q] = (uint16_t)(16 * tid + __builtin_ctz(x));
                __syncthreads();
            }
#pragma unroll 1
            for (int c0 = 0; c0 < m; c0 += RW_THREADS) {
                bool has = c0 + tid < m;
                const int r = !has ? r_first : anywhere ? r_first + c0 + tid : (int)s_list[c0 + tid];
                const uint8_t* tx = s_txt + WL_FRONT + r;
                if (has) {  // no entry begins with this byte: most starts of prose under a short list
                    const uint32_t c = wl_fold(tx[0], fold);
                    has = (s_first[c >> 5] >> (c & 31)) & 1u;
                }
                const int64_t p = tl.base + r;
                int64_t D = tb.kb, ds = ds0, de = de0;
                if (has && !uni) {
                    D = rw_doc_of(a.doc_off, s_off, tb, tl.t0, p);
                    ds = a.doc_off[D];
                    de = a.doc_off[D + 1];
                }
                const int lim = !has ? 0 : de - p < max_len ? (int)(de - p) : max_len;
                uint32_t h = WL_HASH_INIT;
#pragma unroll 1
                for (int L = 1; L <= max_len; ++L) {
                    const bool act = L <= lim;
                    if (!__any(act)) break;
                    int hit = -1;
                    if (act) {
                        h = wl_step(h, wl_fold(tx[L - 1], fold));
                        if (((lengths >> (L - 1)) & 1ull) && (anywhere || p + L == de || !wl_word(tx[L]))) hit = wl_probe<R>(a.set, s_set, tx, L, h, fold);
                    }
                    if (hit >= 0) {
                        if (D != A.D) {
                            if (A.hits) put(A);
                            A = WlAcc{D, 0, 0, ~0ull, 0};
                        }
                        const unsigned long long rel = (unsigned long long)(p - ds);
                        A.hits += 1;
                        A.groups |= 1ull << wl_b<R>(s_set, a.set.blob, 4 * a.set.groups_at + (uint32_t)hit);
                        A.first = rel < A.first ? rel : A.first;
                        A.bytes += (unsigned long long)L;
                    }
                    if (a.entry_hits) {  // one add for the lanes that hit the same entry
                        for (uint64_t pend = __ballot(hit >= 0); pend;) {
                            const int src = __builtin_ctzll(pend);
                            const uint64_t same = __ballot(hit == __shfl(hit, src));
                            if (lane == src) {
                                if (few) atomicAdd(&s_hits[hit], (unsigned long long)__builtin_popcountll(same));
                                else wl_add(a.entry_hits + hit, (unsigned long long)__builtin_popcountll(same));
                            }
                            pend &= ~same;
                        }
                    }
                }
            }
        }
        // ---- the lanes' sums: a tile inside one document adds them up a wavefront first ----
        if (uni) {
            for (int d = 32; d >= 1; d >>= 1) {
                A.hits += (unsigned long long)__shfl_xor((long long)A.hits, d);
                A.bytes += (unsigned long long)__shfl_xor((long long)A.bytes, d);
                A.groups |= (unsigned long long)__shfl_xor((long long)A.groups, d);
                const unsigned long long f = (unsigned long long)__shfl_xor((long long)A.first, d);
                A.first = f < A.first ? f : A.first;
            }
            A.D = tb.kb;
            if (lane == 0 && A.hits) put(A);
        } else if (A.hits) {
            put(A);
        }
        __syncthreads();
        if (tid < WL_SLOTS && s_acc[tid * WL_COLS + WL_HITS]) {
            unsigned long long* row = a.stats + (tb.kb + tid) * WL_COLS;
            wl_add(row + WL_HITS, s_acc[tid * WL_COLS + WL_HITS]);
            wl_or(row + WL_GROUPS, s_acc[tid * WL_COLS + WL_GROUPS]);
            wl_min(row + WL_FIRST_HIT, s_acc[tid * WL_COLS + WL_FIRST_HIT]);
            wl_add(row + WL_HIT_BYTES, s_acc[tid * WL_COLS + WL_HIT_BYTES]);
            s_acc[tid * WL_COLS + WL_HITS] = s_acc[tid * WL_COLS + WL_GROUPS] = s_acc[tid * WL_COLS + WL_HIT_BYTES] = 0;
            s_acc[tid * WL_COLS + WL_FIRST_HIT] = ~0ull;
        }
    }
    __syncthreads();
    if (a.entry_hits && few && tid < (int)a.set.n_entries && s_hits[tid]) wl_add(a.entry_hits + tid, s_hits[tid]);
}

__global__ __launch_bounds__(RW_THREADS) void td_wl_totals(const WlArgs a) {
    if (a.head[RW_H_BAD] || !a.totals) return;
    unsigned long long hits = 0, groups = 0, docs = 0, bytes = 0;
    for (int64_t d = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; d < a.n_docs; d += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long* row = a.stats + d * WL_COLS;
        hits += row[WL_HITS];
        groups |= row[WL_GROUPS];
        docs += row[WL_HITS] != 0;
        bytes += row[WL_HIT_BYTES];
    }
    for (int d = 32; d >= 1; d >>= 1) {
        hits += (unsigned long long)__shfl_xor((long long)hits, d);
        groups |= (unsigned long long)__shfl_xor((long long)groups, d);
        docs += (unsigned long long)__shfl_xor((long long)docs, d);
        bytes += (unsigned long long)__shfl_xor((long long)bytes, d);
    }
    if ((threadIdx.x & 63) == 0 && hits) {
        wl_add(a.totals + WL_HITS, hits);
        wl_or(a.totals + WL_GROUPS, groups);
        wl_add(a.totals + WL_FIRST_HIT, docs);
        wl_add(a.totals + WL_HIT_BYTES, bytes);
    }
}

}  // namespace

hipError_t launch_wordlist(const WlArgs& a, bool resident, hipStream_t stream) {
    hipError_t e;
    if ((e = rewrite_launch(td_wl_docs, rewrite_grid(a.n_docs + 1, RW_THREADS, 4096), a, stream)) != hipSuccess) return e;
    const int64_t cells = a.n_docs * WL_COLS + WL_COLS;
    if ((e = rewrite_launch(td_wl_reset, rewrite_grid(cells > (int64_t)a.set.n_entries ? cells : (int64_t)a.set.n_entries, RW_THREADS, 4096), a, stream)) != hipSuccess) return e;
    const unsigned tiles = rewrite_grid(a.n_bytes + 16, RW_TILE, WL_MAX_GRID);
    if ((e = rewrite_launch(resident ? td_wl_tiles<1> : td_wl_tiles<0>, tiles, a, stream)) != hipSuccess) return e;
    return rewrite_launch(td_wl_totals, rewrite_grid(a.n_docs, RW_THREADS, 1024), a, stream);
}

}  // namespace td
