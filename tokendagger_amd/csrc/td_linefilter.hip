// Line filtering (td_line_filter_device and what ends in it): text + document offsets + rules -> the text without the lines that fail,
// its document offsets, stats[n_docs][LF_COLS] and totals.  The rule is the contract in include/tokendagger_hip.h; td_linefilter_args.h
// has the piece summaries, their append and combine, the phrase compare, the terminal mark and the decision, which the host statement
// (td_line_filter_host) compiles too.  No table: everything is compares on bytes.
//
// The windows, the tiles, the offsets check, the tile's table of documents, the scan of the tiles' sizes and the cooperative copy are
// the text passes' frame (td_rewrite_common.h).  What is this pass's own: a byte's fate is its LINE's, and a line can begin any number
// of tiles in front of the byte and end any number behind it.  A call is
//   td_lf_docs      the frame's offsets check
//   td_lf_reset     stats, totals and counts 0
//   td_lf_carry     a workgroup a tile: the lanes fold their windows to elements {break, head piece, tail piece}, the workgroup
//                   combines them in lane order (shuffles in a wavefront, the wavefronts through LDS) to the tile's element, elems[t]
//   td_lf_prefix    ONE workgroup, a chunk of tiles a lane: for every tile the open piece that ends in front of it (the exclusive
//                   prefix's open piece) and the piece that begins behind it and runs to its line's end (the exclusive suffix's head):
//                   carry[2 t], carry[2 t + 1]
//   td_lf_tiles<0>  MEASURE, a workgroup a tile: the lanes' elements once more, their exclusive scan, then every lane walks its window
//                   behind the open piece in front of it and decides each line at its LAST byte, the one byte the line's counts
//                   belong to; a line that began in front of the tile is completed with carry[2 t].  The fate of a line's bytes goes
//                   backwards to them: in the lane, by ballots in the wavefront, through LDS across wavefronts, and for the line that
//                   leaves the tile from the decision on piece in front + tile + carry[2 t + 1].  Left behind: 16 bits a window in
//                   masks, the tile's kept bytes in tile_base, the per-document columns (a wavefront that ends in one document adds
//                   up by shuffles, the rest meets in LDS over the tile's first LF_SLOTS documents, then 64-bit adds).
//   td_lf_scan      the frame's: tile_base to its prefixes, counts[0], TD_E_CAPACITY
//   td_lf_totals    a lane a document: the columns' sums into totals
//   td_lf_tiles<1>  WRITE: the masks' population counts place the lanes; a tile that is all kept is one cooperative copy, any other is
//                   compacted lane by lane; the lane that has a document's first byte writes its output offset.
// Phrases carry nothing: the lane at byte i compares forward in the text, up to its document's end, behind a 256-bit screen of the
// phrases' first bytes in LDS; the terminal mark is read from the text at the line's last non-space position.  Nothing outside
// text[0, doc_off[n_docs]) and doc_off[0, n_docs] is read.  Only stores of values that do not depend on the lanes' order and integer
// adds touch the outputs.
#include <hip/hip_runtime.h>

#include "td_linefilter.h"
#include "td_rewrite_common.h"

namespace td {

namespace {

using P32 = LfPiece<int32_t>;
using E32 = LfElem<int32_t>;
using P64 = LfPiece<int64_t>;
using E64 = LfElem<int64_t>;

constexpr int LF_WAVES = RW_THREADS / 64;
constexpr int LF_SLOTS = 32;  // documents of a tile whose sums meet in LDS

struct LfLds {  // the rules as the lanes read them
    uint32_t first[8];  // bit c: a phrase begins with byte c
    uint8_t len[TD_LF_MAX_PHRASES], kind[TD_LF_MAX_PHRASES];
    uint8_t bytes[TD_LF_MAX_PHRASES][TD_LF_PHRASE_BYTES];
};

// by the whole workgroup; the caller's next barrier publishes it
__device__ __forceinline__ void lf_load_rules(const LfArgs& a, LfLds& s) {
    const int tid = threadIdx.x;
    if (tid < 8) s.first[tid] = 0;
    for (int i = tid; i < TD_LF_MAX_PHRASES * TD_LF_PHRASE_BYTES; i += RW_THREADS)
        s.bytes[i / TD_LF_PHRASE_BYTES][i % TD_LF_PHRASE_BYTES] = a.rules.phrases[i / TD_LF_PHRASE_BYTES].bytes[i % TD_LF_PHRASE_BYTES];
    if (tid < TD_LF_MAX_PHRASES) {
        s.len[tid] = a.rules.phrases[tid].len;
        s.kind[tid] = a.rules.phrases[tid].kind;
    }
    __syncthreads();
    if (tid < a.rules.n_phrases) atomicOr(&s.first[a.rules.phrases[tid].bytes[0] >> 5], 1u << (a.rules.phrases[tid].bytes[0] & 31));
}

// the phrases that occur at p, whose byte is c: a drop-line phrase is the result, the count-doc phrases are added to hits
template <bool COUNT>
__device__ __forceinline__ bool lf_hits(const LfLds& s, int n_phrases, const uint8_t* text, int64_t p, int64_t de, uint32_t c, uint32_t& hits) {
    const uint32_t lc = lf_lower(c);
    if (!((s.first[lc >> 5] >> (lc & 31)) & 1u)) return false;
    bool drop = false;
    for (int j = 0; j < n_phrases; ++j) {
        const bool line = s.kind[j] == TD_LF_PHRASE_DROP_LINE;
        if (s.bytes[j][0] != lc || (!COUNT && !line) || (line && drop) || !lf_occurs(text, p, de, s.bytes[j], s.len[j])) continue;
        if (line) drop = true;
        else ++hits;
    }
    return drop;
}

template <class S>
__device__ __forceinline__ S lf_shfl(const S& v, int src) {
    static_assert(sizeof(S) % 4 == 0, "whole dwords");
    uint32_t w[sizeof(S) / 4];
    __builtin_memcpy(w, &v, sizeof(S));
#pragma unroll
    for (unsigned i = 0; i < sizeof(S) / 4; ++i) w[i] = __shfl(w[i], src);
    S r;
    __builtin_memcpy(&r, w, sizeof(S));
    return r;
}

// v of the workgroup's lanes, in lane order, to what the lanes in front of each (REV: behind each) combine to, the identity at the end;
// all: all of them combined.  s_wave: LF_WAVES elements of LDS.
template <bool REV, class T>
__device__ __forceinline__ void lf_block_excl(LfElem<T>& v, LfElem<T>* s_wave, LfElem<T>& all) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    LfElem<T> incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const LfElem<T> o = lf_shfl(incl, (REV ? lane + d : lane + 64 - d) & 63);
        if (REV ? lane + d < 64 : lane >= d) incl = REV ? lf_combine(incl, o) : lf_combine(o, incl);
    }
    __syncthreads();  // (the readers of an earlier call are done)
    if (lane == (REV ? 0 : 63)) s_wave[wv] = incl;
    __syncthreads();
    LfElem<T> side = lf_identity<T>();
    all = lf_identity<T>();
    for (int x = 0; x < LF_WAVES; ++x) {
        const LfElem<T> sw = s_wave[x];
        if (REV ? x > wv : x < wv) side = lf_combine(side, sw);
        all = lf_combine(all, sw);
    }
    const LfElem<T> nb = lf_shfl(incl, (REV ? lane + 1 : lane + 63) & 63);
    v = REV ? (lane < 63 ? lf_combine(nb, side) : side) : (lane > 0 ? lf_combine(side, nb) : side);
}

__device__ __forceinline__ void lf_add(unsigned long long* p, unsigned long long v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct LfDoc {  // the document a lane's walk is in
    int64_t D, ds, de;
};
struct LfWin {  // a window as the walks see it: a bit a byte, bit k is byte b0 + k
    uint32_t space, end, drop;  // a space byte; its line's last byte; a drop-line phrase occurs at it
    bool first_brk;             // a break lies in front of the window's first byte
};

__device__ __forceinline__ void lf_next_doc(const int64_t* doc_off, int64_t p, LfDoc& doc) {
    do {
        ++doc.D;
        doc.ds = doc.de;
        doc.de = doc_off[doc.D + 1];
    } while (p >= doc.de);
}

// The window [b, we) (w: its bytes from b0 on) to its element, positions from `base`, and to m.  COUNT: the count-doc phrases' occurrences
// too, into hits; put(D, hits) when the walk leaves document D.
template <bool COUNT, class Put>
__device__ __forceinline__ E32 lf_window(const LfArgs& a, const LfLds& s, int64_t base, int64_t b0, int64_t b, int64_t we, const uint32_t w[4],
                                         LfDoc& doc, LfWin& m, uint32_t& hits, Put put) {
    uint64_t lo = w[0] | (uint64_t)w[1] << 32, hi = w[2] | (uint64_t)w[3] << 32;
    const int k0 = (int)(b - b0), k1 = (int)(we - b0);
    for (int k = 0; k < k0; ++k) {
        lo = lo >> 8 | hi << 56;
        hi >>= 8;
    }
    bool brk = b == 0 || b == doc.ds || a.text[b - 1] == 0x0A;
    m = LfWin{0, 0, 0, brk};
    E32 e = lf_identity<int32_t>();
    P32 cur = lf_empty<int32_t>();
#pragma unroll 1
    for (int k = k0; k < k1; ++k) {
        const int64_t p = b0 + k;
        const uint32_t c = (uint32_t)lo & 0xFFu;
        lo = lo >> 8 | hi << 56;
        hi >>= 8;
        if (p >= doc.de) {
            if (COUNT && hits) put(doc.D, hits);
            hits = 0;
            lf_next_doc(a.doc_off, p, doc);
        }
        if (brk) {
            if (!e.brk) e.head = cur;
            e.brk = 1;
            cur = lf_empty<int32_t>();
        }
        const bool sp = lf_space(c), drop = lf_hits<COUNT>(s, a.rules.n_phrases, a.text, p, doc.de, c, hits);
        lf_append(cur, sp, drop, (int32_t)(p - base));
        brk = c == 0x0A || p + 1 == doc.de;
        m.space |= (uint32_t)sp << k;
        m.drop |= (uint32_t)drop << k;
        m.end |= (uint32_t)brk << k;
    }
    if (e.brk) e.tail = cur;
    else e.head = cur;
    return e;
}

__device__ __forceinline__ int64_t lf_tiles_of(const LfArgs& a, int64_t& total, int& shift) {
    total = a.doc_off[a.n_docs];
    shift = (int)(((uintptr_t)a.text) & 15);
    return total > 0 ? (total + shift + RW_TILE - 1) / RW_TILE : 0;
}

__global__ __launch_bounds__(RW_THREADS) void td_lf_docs(const LfArgs a) {
    rewrite_docs(a, blockIdx.x * (int64_t)blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

__global__ __launch_bounds__(RW_THREADS) void td_lf_reset(const LfArgs a) {
    if (a.head[RW_H_BAD]) return;
    const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    if (gid < RW_C_WORDS) a.counts[gid] = 0;
    if (a.totals && gid < LF_COLS) a.totals[gid] = 0;
    for (int64_t i = gid; i < a.n_docs * LF_COLS; i += step) a.stats[i] = 0;
}

// ---- the tiles' elements, and what lies in front of and behind every tile -----------------------------------------------------------------
__global__ __launch_bounds__(RW_THREADS) void td_lf_carry(const LfArgs a) {
    __shared__ int32_t s_off[RC_LDS_DOCS];
    __shared__ E32 s_wave[LF_WAVES];
    __shared__ LfLds s_rules;
    if (rewrite_bad_offsets(a, true)) return;
    const int tid = threadIdx.x;
    lf_load_rules(a, s_rules);
    int64_t total;
    int shift;
    const int64_t ntiles = lf_tiles_of(a, total, shift);
    const auto off_of = [off = a.doc_off](int64_t d) { return off[d]; };
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const RwTile tl = rw_tile(t, shift, total);
        const int64_t b0 = tl.base + 16 * tid, b = b0 < 0 ? 0 : b0, we = b0 + 16 < total ? b0 + 16 : total;
        const bool owns = b < we;
        uint32_t w[4] = {0, 0, 0, 0};
        if (owns) rw_load(a.text, b0, b, we, w);
        __syncthreads();  // (the tile before has read its table; s_rules is written)
        const RwTable tb = rw_table(s_off, off_of, a.n_docs, tl);
        __syncthreads();
        E32 e = lf_identity<int32_t>(), all;
        if (owns) {
            LfDoc doc;
            doc.D = rw_doc_of(a.doc_off, s_off, tb, tl.t0, b);
            doc.ds = a.doc_off[doc.D];
            doc.de = a.doc_off[doc.D + 1];
            LfWin m;
            uint32_t hits = 0;
            e = lf_window<false>(a, s_rules, tl.base, b0, b, we, w, doc, m, hits, [](int64_t, uint32_t) {});
        }
        lf_block_excl<false>(e, s_wave, all);
        if (tid == 0) a.elems[t] = E64{lf_widen(all.head, tl.base), lf_widen(all.tail, tl.base), all.brk};
    }
}

__global__ __launch_bounds__(RW_THREADS) void td_lf_prefix(const LfArgs a) {
    __shared__ E64 s_wave[LF_WAVES];
    if (a.head[RW_H_BAD]) return;
    int64_t total;
    int shift;
    const int64_t ntiles = lf_tiles_of(a, total, shift);
    const int64_t per = (ntiles + RW_THREADS - 1) / RW_THREADS;
    const int64_t t0 = threadIdx.x * per < ntiles ? threadIdx.x * per : ntiles, t1 = t0 + per < ntiles ? t0 + per : ntiles;
    E64 T = lf_identity<int64_t>(), all;
#pragma unroll 1
    for (int64_t t = t0; t < t1; ++t) T = lf_combine(T, a.elems[t]);
    E64 front = T, behind = T;
    lf_block_excl<false>(front, s_wave, all);
    lf_block_excl<true>(behind, s_wave, all);
#pragma unroll 1
    for (int64_t t = t0; t < t1; ++t) {
        a.carry[2 * t] = lf_open(front);
        front = lf_combine(front, a.elems[t]);
    }
#pragma unroll 1
    for (int64_t t = t1 - 1; t >= t0; --t) {
        a.carry[2 * t + 1] = behind.head;
        behind = lf_combine(a.elems[t], behind);
    }
}

// ---- the decision and the write -----------------------------------------------------------------------------------------------------------
// row's sums for document D: into the tile's table in LDS where D is among its first LF_SLOTS documents, to stats otherwise
template <class S>
__device__ __forceinline__ void lf_put(const LfArgs& a, unsigned long long* s_acc, int64_t kb, int64_t D, const S (&row)[LF_COLS]) {
    const int64_t slot = D - kb;
#pragma unroll
    for (int c = 0; c < LF_COLS; ++c) {
        if (!row[c]) continue;
        if (slot < LF_SLOTS) atomicAdd(&s_acc[slot * LF_COLS + c], (unsigned long long)row[c]);
        else lf_add(a.stats + D * LF_COLS + c, (unsigned long long)row[c]);
    }
}

template <int WRITE>
__global__ __launch_bounds__(RW_THREADS) void td_lf_tiles(const LfArgs a) {
    __shared__ int32_t s_off[RC_LDS_DOCS];
    __shared__ long long s_red[LF_WAVES];
    __shared__ E32 s_wave[LF_WAVES];
    __shared__ unsigned long long s_acc[LF_SLOTS * LF_COLS];
    __shared__ LfLds s_rules;
    __shared__ uint32_t s_next[LF_WAVES + 1];  // a wavefront's first line end: 1 | its fate << 1, 0: none; [LF_WAVES]: the line that leaves the tile
    if (rewrite_bad_offsets(a, false)) return;
    if (WRITE && a.head[RW_H_FULL]) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if constexpr (!WRITE) {
        lf_load_rules(a, s_rules);
        for (int i = tid; i < LF_SLOTS * LF_COLS; i += RW_THREADS) s_acc[i] = 0;
    }
    int64_t total;
    int shift;
    const int64_t ntiles = lf_tiles_of(a, total, shift);
    const auto off_of = [off = a.doc_off](int64_t d) { return off[d]; };
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const RwTile tl = rw_tile(t, shift, total);
        const int64_t b0 = tl.base + 16 * tid, b = b0 < 0 ? 0 : b0, we = b0 + 16 < total ? b0 + 16 : total;
        const bool owns = b < we;
        const int k0 = (int)(b - b0), k1 = (int)(we - b0);
        uint32_t w[4] = {0, 0, 0, 0};
        if (owns && (!WRITE || a.out)) rw_load(a.text, b0, b, we, w);
        __syncthreads();  // (the tile before has read its table and emptied s_acc; s_rules and s_acc are written)
        RwTable tb = {0, 0, true};
        if (!WRITE || a.out_doc_off) {
            tb = rw_table(s_off, off_of, a.n_docs, tl);
            __syncthreads();
        }
        if constexpr (!WRITE) {
            LfDoc doc = {0, 0, 0}, doc0 = doc;
            LfWin m = {0, 0, 0, false};
            uint32_t hits = 0;
            E32 e = lf_identity<int32_t>(), all;
            if (owns) {
                doc.D = rw_doc_of(a.doc_off, s_off, tb, tl.t0, b);
                doc.ds = a.doc_off[doc.D];
                doc.de = a.doc_off[doc.D + 1];
                doc0 = doc;
                e = lf_window<true>(a, s_rules, tl.base, b0, b, we, w, doc, m, hits, [&](int64_t D, uint32_t n) {
                    const uint32_t row[LF_COLS] = {0, 0, 0, 0, 0, 0, 0, n};
                    lf_put(a, s_acc, tb.kb, D, row);
                });
            }
            lf_block_excl<false>(e, s_wave, all);  // e: the lanes in front
            const P64 pre = a.carry[2 * t];
            // the walk behind the open piece in front of the window: every line is decided at its last byte
            uint32_t keep = 0, acc[LF_COLS] = {0, 0, 0, 0, 0, 0, 0, 0};
            if (owns) {
                doc = doc0;
                P32 cur = lf_open(e);
                bool outer = !e.brk, brk = m.first_brk;  // outer: the line began in front of the tile
#pragma unroll 1
                for (int k = k0; k < k1; ++k) {
                    const int64_t p = b0 + k;
                    if (p >= doc.de) {
                        lf_put(a, s_acc, tb.kb, doc.D, acc);
#pragma unroll
                        for (int c = 0; c < LF_COLS; ++c) acc[c] = 0;
                        lf_next_doc(a.doc_off, p, doc);
                    }
                    if (brk) {
                        cur = lf_empty<int32_t>();
                        outer = false;
                    }
                    lf_append(cur, (m.space >> k) & 1u, (m.drop >> k) & 1u, (int32_t)(p - tl.base));
                    brk = (m.end >> k) & 1u;
                    if (!brk) continue;
                    P64 l = lf_widen(cur, tl.base);
                    if (outer) l = lf_join(pre, l);
                    const int fail = lf_decide(a.rules.min_words, a.rules.max_word_bytes, a.rules.flags, a.text, l, p + 1 - l.len);
                    keep |= (uint32_t)(fail == 0) << k;
                    if (outer) {  // (its bytes may pass 2^32: one line a tile at the most)
                        unsigned long long row[LF_COLS] = {0, 0, 0, 0, 0, 0, 0, 0};
                        lf_count(row, fail, l.len);
                        lf_put(a, s_acc, tb.kb, doc.D, row);
                    } else {
                        lf_count(acc, fail, l.len);
                    }
                }
                acc[LF_DOC_HITS] = hits;
            }
            // a byte's fate is that of the first line end at or behind it: in the lane, the wavefront, the workgroup, behind the tile
            const uint32_t fk = m.end ? (keep >> __builtin_ctz(m.end)) & 1u : 0u;
            const unsigned long long has = __ballot(m.end != 0), fkm = __ballot(fk != 0);
            if (lane == 0) s_next[wv] = has ? 1u | (uint32_t)((fkm >> __builtin_ctzll(has)) & 1ull) << 1 : 0u;
            if (tid == 0) {
                P64 open = lf_widen(lf_open(all), tl.base);
                if (!all.brk) open = lf_join(pre, open);
                const P64 full = lf_join(open, a.carry[2 * t + 1]);
                s_next[LF_WAVES] = lf_decide(a.rules.min_words, a.rules.max_word_bytes, a.rules.flags, a.text, full, tl.s1 - open.len) == 0;
            }
            __syncthreads();
            const unsigned long long above = (has >> lane) >> 1;
            uint32_t run;
            if (above) {
                run = (uint32_t)((fkm >> (lane + 1 + __builtin_ctzll(above))) & 1ull);
            } else {
                run = s_next[LF_WAVES];
                for (int x = LF_WAVES - 1; x > wv; --x)
                    if (s_next[x] & 1u) run = s_next[x] >> 1;
            }
            uint32_t mask = 0;
            for (int k = k1 - 1; k >= k0; --k) {
                if ((m.end >> k) & 1u) run = (keep >> k) & 1u;
                mask |= run << k;
            }
            if (owns) a.masks[t * RW_THREADS + tid] = (uint16_t)mask;
            const long long sum = block_sum(__builtin_popcount(mask), s_red);
            if (tid == 0) a.tile_base[t] = (unsigned long long)sum;
            // the lanes' sums for the documents they end in: a wavefront that ends in one document adds them up first
            const int64_t Dw = __shfl((long long)doc.D, 0);
            if (__all(!owns || doc.D == Dw)) {
#pragma unroll
                for (int c = 0; c < LF_COLS; ++c)
                    for (int d = 32; d >= 1; d >>= 1) acc[c] += __shfl_xor(acc[c], d);
                if (lane == 0 && owns) lf_put(a, s_acc, tb.kb, doc.D, acc);
            } else if (owns) {
                lf_put(a, s_acc, tb.kb, doc.D, acc);
            }
            __syncthreads();
            for (int i = tid; i < LF_SLOTS * LF_COLS; i += RW_THREADS) {
                const unsigned long long v = s_acc[i];
                if (!v) continue;
                lf_add(a.stats + (tb.kb + i / LF_COLS) * LF_COLS + i % LF_COLS, v);
                s_acc[i] = 0;
            }
        } else {
            const uint32_t whole = owns ? ((1u << k1) - 1u) & ~((1u << k0) - 1u) : 0u;
            const uint32_t mask = owns ? a.masks[t * RW_THREADS + tid] : 0u;
            long long sum;
            int64_t opos = (int64_t)a.tile_base[t] + block_excl(__builtin_popcount(mask), s_red, sum);
            // the output offsets of the documents that start in the window: the kept bytes of the window in front of each
            if (owns && a.out_doc_off) {
                for (int64_t k = b > 0 ? rw_doc_of(a.doc_off, s_off, tb, tl.t0, b - 1) + 1 : 0; k <= a.n_docs; ++k) {
                    const int64_t s = a.doc_off[k];
                    if (s >= we) break;
                    a.out_doc_off[k] = opos + __builtin_popcount(mask & ((1u << (int)(s - b0)) - 1u));
                }
            }
            if (__syncthreads_and(mask == whole)) {
                if (a.out) rewrite_group_copy(a.out + a.tile_base[t], a.text + tl.t0, tl.s1 - tl.t0);
            } else if (a.out && mask) {
                uint64_t lo = w[0] | (uint64_t)w[1] << 32, hi = w[2] | (uint64_t)w[3] << 32;
                for (uint32_t left = mask, k = 0; left; left >>= 1, ++k) {
                    if (left & 1u) a.out[opos++] = (uint8_t)lo;
                    lo = lo >> 8 | hi << 56;
                    hi >>= 8;
                }
            }
        }
    }
}

__global__ __launch_bounds__(RW_THREADS) void td_lf_scan(const LfArgs a) { rewrite_scan(a); }

__global__ __launch_bounds__(RW_THREADS) void td_lf_totals(const LfArgs a) {
    __shared__ long long s_red[LF_WAVES];
    if (a.head[RW_H_BAD] || !a.totals) return;
    long long v[LF_COLS] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t d = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; d < a.n_docs; d += (int64_t)gridDim.x * blockDim.x) {
#pragma unroll
        for (int c = 0; c < LF_COLS; ++c) v[c] += (long long)a.stats[d * LF_COLS + c];
    }
#pragma unroll
    for (int c = 0; c < LF_COLS; ++c) {
        const long long r = block_sum(v[c], s_red);
        if (threadIdx.x == 0 && r) lf_add(a.totals + c, (unsigned long long)r);
    }
}

}  // namespace

hipError_t launch_linefilter(const LfArgs& a, hipStream_t stream, int phases) {
    hipError_t e;
    const unsigned tiles = rewrite_grid(a.n_bytes + 16, RW_TILE, RW_MAX_GRID);
    if (phases & RW_RUN_MEASURE) {
        if ((e = rewrite_launch(td_lf_docs, rewrite_grid(a.n_docs + 1, RW_THREADS, 4096), a, stream)) != hipSuccess) return e;
        if ((e = rewrite_launch(td_lf_reset, rewrite_grid(a.n_docs * LF_COLS + LF_COLS, RW_THREADS, 4096), a, stream)) != hipSuccess) return e;
        if ((e = rewrite_launch(td_lf_carry, tiles, a, stream)) != hipSuccess) return e;
        if ((e = rewrite_launch(td_lf_prefix, 1, a, stream)) != hipSuccess) return e;
        if ((e = rewrite_launch(td_lf_tiles<0>, tiles, a, stream)) != hipSuccess) return e;
        if ((e = rewrite_launch(td_lf_scan, 1, a, stream)) != hipSuccess) return e;
        if ((e = rewrite_launch(td_lf_totals, rewrite_grid(a.n_docs, RW_THREADS, 1024), a, stream)) != hipSuccess) return e;
    }
    return phases & RW_RUN_WRITE ? rewrite_launch(td_lf_tiles<1>, tiles, a, stream) : hipGetLastError();
}

}  // namespace td
