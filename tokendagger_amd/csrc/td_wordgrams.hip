// Per-document word n-gram repetition statistics (td_word_ngrams_device and what ends in it): text + document offsets ->
// stats[n_docs][WG_COLS] and totals[WG_COLS].  The rule is the contract in include/tokendagger_hip.h; td_wordgrams_args.h has the rule of
// one byte, a word's record, the keys and the host statement.
//
// The windows, the tiles, the offsets check and the tile's table of documents are the text passes' frame (td_rewrite_common.h); the scan
// of a word's hash across windows, wavefronts and tiles is td_repetition's (td_repetition_scan.h), with one kind of unit, the word.  The
// second element of that scan's pair carries {-1, word ends, 1, word characters}: under rp_combine such elements add, so a byte also
// knows the rank of its word and the word characters in front of it.  A call is
//   td_wg_docs      the frame's offsets check
//   td_wg_summary   a workgroup a tile: the lanes' elements combined in order into carry[t]; the words of the call counted into head
//   td_rp_prefix    ONE workgroup (td_repetition's kernel): carry to its inclusive prefixes; more words than max_words raise TD_E_CAPACITY
//   td_wg_reset     stats and totals to 0, first_word of the documents at the text's end (nothing when an error was raised)
//   td_wg_tiles     a workgroup a tile: a lane whose window holds a word's last byte writes the word's record at its rank and the word
//                   characters up to it behind it (cum); the lane that holds a document's first byte writes first_word of it and of the
//                   empty documents in front of it; the documents' characters go to CHARS by adds (in LDS for the tile's first documents)
//   td_wg_long      ONE workgroup, a chunk of documents a lane: the list of the documents of the global path (more than WG_LDS_WORDS
//                   words, or all under WG_NO_LDS) with their words in front of each; the global table's size from their words
//   td_wg_short     a workgroup WG_DOC_BLOCK documents: WORDS and WORD_CHARS of each; then the ones of 2 .. WG_LDS_WORDS words one after
//                   another (ONE document a workgroup at a time), for each n asked for: the table in LDS cleared (as many slots as the
//                   document needs), an occurrence a lane inserted (one CAS claims an empty slot; a slot with the same tag is compared
//                   word by word against the text) and counted, a barrier, then TOP (the maximum count, then the maximum of the
//                   characters among those that reach it) or DUP (flags, a barrier, a look-back over n flags a word)
//   td_wg_insert, td_wg_count, td_wg_cover   the same three steps for the documents of the list, a lane an occurrence, with one table in
//                   global memory shared by all of them (the document is mixed into the key and checked on compare), cleared by
//                   td_wg_cover for the next n; TOP by two rounds of atomic maxima on the document's columns, DUP by adds
//   td_wg_totals    a lane a document: the columns' sums and maxima into totals
// An n-gram's key is formed from its n word hashes directly (at most ten reads), not rolled along consecutive occurrences.
// Nothing outside text[0, doc_off[n_docs]) and doc_off[0, n_docs] is read.  Only stores, adds and maxima touch the outputs, and two
// n-grams are the same by their bytes alone: the results do not depend on the order of the lanes or on the hash.  No kernel waits for
// another workgroup.
#include <hip/hip_runtime.h>

#include "td_repetition_scan.h"
#include "td_wordgrams.h"

namespace td {

namespace {

constexpr int WG_DOC_BLOCK = 32;  // documents a workgroup of td_wg_short takes at a time
constexpr int WG_ACC = 32;        // documents of a tile whose characters meet in LDS
constexpr int WG_MAX_GRID = 2048;

// a lane's window: its 16 bytes and the byte behind them (a space where the text ends)
struct WgWindow {
    uint64_t lo, hi;
    uint32_t next;
};

// The bytes [b, we) of the window at b0 behind E (E[0]: the open word, E[1]: the word ends and word characters in front of b), cur the
// document of b; all are moved on.  on_doc(p, cur, E[1]) in front of a document's first byte p, on_end(p, E[0], cur, E[1]) where a word
// ends with byte p (E[1]: its rank, the word characters up to p), on_chars(D, n) for the n characters of document D the lane has seen.
template <class Doc, class End, class Chars>
__device__ __forceinline__ void wg_walk(const int64_t* doc_off, WgWindow W, int64_t b0, int64_t b, int64_t we, RpCursor& cur, RpElem (&E)[2],
                                        Doc on_doc, End on_end, Chars on_chars) {
    unsigned chars = 0;
#pragma unroll 1
    for (int k = 0; k < 16; ++k) {
        const int64_t p = b0 + k;
        const uint32_t x = (uint32_t)W.lo & 0xFFu;
        W.lo = (W.lo >> 8) | (W.hi << 56);
        W.hi >>= 8;
        const uint32_t nx = k < 15 ? (uint32_t)W.lo & 0xFFu : W.next;
        if (p < b || p >= we) continue;
        if (p >= cur.de && chars) {
            on_chars(cur.D, chars);
            chars = 0;
        }
        rp_advance(doc_off, p, cur);
        if (p == cur.ds) {
            E[0] = rp_open(p);
            on_doc(p, cur, E[1]);
        }
        chars += rp_is_char(x);
        if (wg_is_space(x)) {
            E[0] = rp_open(p + 1);
            continue;
        }
        rp_append(E[0], x);
        E[1].c += rp_is_char(x);
        if (p + 1 == cur.de || wg_is_space(nx)) {  // (p + 1 < cur.de: nx is text[p + 1])
            on_end(p, E[0], cur, E[1]);
            E[1].h += 1;
        }
    }
    if (chars) on_chars(cur.D, chars);
}

// A lane's part of a tile: its window, its document, and the fold of its bytes from the identity into E.
struct WgLane {
    int64_t b0, b, we;
    bool owns;
    WgWindow W;
    RpCursor cur;  // the document of b
};
__device__ __forceinline__ void wg_lane(const WgArgs& a, int32_t* s_off, const RwTile& tl, int64_t total, WgLane& L, RwTable& tb, RpElem (&E)[2]) {
    const auto off_of = [off = a.doc_off](int64_t d) { return off[d]; };
    L.b0 = tl.base + 16 * (int64_t)threadIdx.x;
    L.b = L.b0 < 0 ? 0 : L.b0;
    L.we = L.b0 + 16 < total ? L.b0 + 16 : total;
    L.owns = L.b < L.we;
    L.W = WgWindow{0, 0, 0x20u};
    if (L.owns) {
        uint32_t w[4];
        rw_load(a.text, L.b0, L.b, L.we, w);
        L.W.lo = w[0] | ((uint64_t)w[1] << 32);
        L.W.hi = w[2] | ((uint64_t)w[3] << 32);
        if (L.b0 + 16 < total) L.W.next = a.text[L.b0 + 16];
    }
    __syncthreads();  // (the tile before has read its table)
    tb = rw_table(s_off, off_of, a.n_docs, tl);
    __syncthreads();
    E[0] = E[1] = rp_identity();
    L.cur = RpCursor{-1, 0, 0};
    if (L.owns) {
        L.cur.D = rw_doc_of(a.doc_off, s_off, tb, tl.t0, L.b);
        L.cur.ds = a.doc_off[L.cur.D];
        L.cur.de = a.doc_off[L.cur.D + 1];
        RpCursor c = L.cur;
        wg_walk(a.doc_off, L.W, L.b0, L.b, L.we, c, E, [](int64_t, const RpCursor&, const RpElem&) {},
                [](int64_t, const RpElem&, const RpCursor&, const RpElem&) {}, [](int64_t, unsigned) {});
    }
}

__device__ __forceinline__ bool wg_stopped(const WgArgs& a) { return a.head[RW_H_BAD] || a.head[RW_H_FULL]; }

__global__ __launch_bounds__(RW_THREADS) void td_wg_docs(const WgArgs a) {
    rewrite_docs(a, blockIdx.x * (int64_t)blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

__global__ __launch_bounds__(RW_THREADS) void td_wg_summary(const WgArgs a) {
    __shared__ int32_t s_off[RC_LDS_DOCS];
    __shared__ RpElem s_wave[2 * RP_WAVES];
    if (rewrite_bad_offsets(a, true)) return;
    int64_t total;
    int shift;
    const int64_t ntiles = rp_tiles(a, total, shift);
    unsigned long long words = 0;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const RwTile tl = rw_tile(t, shift, total);
        WgLane L;
        RwTable tb;
        RpElem E[2], all[2];
        wg_lane(a, s_off, tl, total, L, tb, E);
        rp_block_excl(E, s_wave, all);
        if (threadIdx.x == 0) {
            a.carry[2 * t] = all[0];
            a.carry[2 * t + 1] = all[1];
        }
        words += all[1].h;
    }
    if (threadIdx.x == 0 && words) __hip_atomic_fetch_add(&a.head[RP_H_UNITS], words, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(RW_THREADS) void td_wg_reset(const WgArgs a) {
    if (wg_stopped(a)) return;
    const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    if (a.totals && gid < WG_COLS) a.totals[gid] = 0;
    if (gid == 0) a.cum[0] = 0;
    for (int64_t i = gid; i < a.n_docs * WG_COLS; i += step) a.stats[i] = 0;
    // the documents that start at the text's end (the entry behind the last one among them): no window holds them
    const int64_t total = a.doc_off[a.n_docs];
    const long long words = (long long)a.head[RP_H_UNITS];
    for (int64_t d = gid; d <= a.n_docs; d += step)
        if (a.doc_off[d] == total) a.first_word[d] = words;
}

__global__ __launch_bounds__(RW_THREADS) void td_wg_tiles(const WgArgs a) {
    __shared__ int32_t s_off[RC_LDS_DOCS];
    __shared__ RpElem s_wave[2 * RP_WAVES];
    __shared__ unsigned long long s_acc[WG_ACC];
    if (wg_stopped(a)) return;
    const int tid = threadIdx.x;
    if (tid < WG_ACC) s_acc[tid] = 0;
    int64_t total;
    int shift;
    const int64_t ntiles = rp_tiles(a, total, shift);
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const RwTile tl = rw_tile(t, shift, total);
        WgLane L;
        RwTable tb;
        RpElem E[2], all[2];
        wg_lane(a, s_off, tl, total, L, tb, E);  // (its first barrier: the tile before has emptied s_acc)
        rp_block_excl(E, s_wave, all);
        if (L.owns) {
            if (t > 0) {
                E[0] = rp_combine(a.carry[2 * (t - 1)], E[0]);
                E[1] = rp_combine(a.carry[2 * (t - 1) + 1], E[1]);
            }
            wg_walk(
                a.doc_off, L.W, L.b0, L.b, L.we, L.cur, E,
                [&](int64_t p, const RpCursor& c, const RpElem& e1) {
                    a.first_word[c.D] = (long long)e1.h;
                    for (int64_t k = c.D - 1; k >= 0 && a.doc_off[k] == p; --k) a.first_word[k] = (long long)e1.h;  // (empty ones)
                },
                [&](int64_t p, const RpElem& R, const RpCursor& c, const RpElem& e1) {
                    if (R.s < c.ds || R.s > p || e1.h >= (uint64_t)a.max_units) return;  // (a word begins in its document; a fence)
                    a.rec[e1.h] = wg_word(R.h, R.s, p - R.s + 1);
                    a.cum[e1.h + 1] = e1.c;
                },
                [&](int64_t D, unsigned n) {
                    const int64_t slot = D - tb.kb;
                    if ((uint64_t)slot < (uint64_t)WG_ACC) atomicAdd(&s_acc[slot], (unsigned long long)n);
                    else __hip_atomic_fetch_add(a.stats + D * WG_COLS + WG_CHARS, (unsigned long long)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                });
        }
        __syncthreads();
        if (tid < WG_ACC) {
            const unsigned long long v = s_acc[tid];
            if (v) {
                __hip_atomic_fetch_add(a.stats + (tb.kb + tid) * WG_COLS + WG_CHARS, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                s_acc[tid] = 0;
            }
        }
    }
}

__global__ __launch_bounds__(RW_THREADS) void td_wg_long(const WgArgs a) {
    __shared__ long long s_wave[RP_WAVES];
    if (wg_stopped(a)) return;
    const long long most = (a.wflags & WG_NO_LDS) ? 0 : WG_LDS_WORDS;
    const auto words_of = [&](int64_t d) {  // of a document of the global path, 0 of any other
        const long long w = a.first_word[d + 1] - a.first_word[d];
        return w >= WG_TOP_LO && w > most ? w : 0ll;
    };
    const int64_t per = (a.n_docs + RW_THREADS - 1) / RW_THREADS;
    const int64_t d0 = threadIdx.x * per < a.n_docs ? threadIdx.x * per : a.n_docs, d1 = d0 + per < a.n_docs ? d0 + per : a.n_docs;
    long long docs = 0, words = 0, all_docs, all_words;
    for (int64_t d = d0; d < d1; ++d) {
        const long long w = words_of(d);
        docs += w > 0;
        words += w;
    }
    docs = block_excl(docs, s_wave, all_docs);
    words = block_excl(words, s_wave, all_words);
    for (int64_t d = d0; d < d1; ++d) {
        const long long w = words_of(d);
        if (!w) continue;
        a.long_doc[docs] = d;
        a.long_first[docs] = words;
        docs += 1;
        words += w;
    }
    if (threadIdx.x == 0) {
        a.long_first[all_docs] = all_words;
        a.lhead[WG_L_DOCS] = (unsigned long long)all_docs;
        a.lhead[WG_L_WORDS] = (unsigned long long)all_words;
        a.head[RP_H_MASK] = rp_slots(all_words) - 1;
    }
}

// ---- equal words, equal n-grams -------------------------------------------------------------------------------------------------------------
// two words of a document that ends at de
__device__ __forceinline__ bool wg_word_equal(const uint8_t* text, const WgWord& u, const WgWord& v, int64_t de) {
    if (u.h != v.h || ((u.sl ^ v.sl) & WG_LEN_SAT)) return false;
    const int64_t su = wg_start(u), sv = wg_start(v), len = (int64_t)(u.sl & WG_LEN_SAT);
    if (su == sv) return true;
    if (!rp_equal(text + su, text + sv, len)) return false;
    if (len < (int64_t)WG_LEN_SAT) return true;
    for (int64_t k = len;; ++k) {  // both are at least that long: on to the end of either
        const bool eu = su + k >= de || wg_is_space(text[su + k]), ev = sv + k >= de || wg_is_space(text[sv + k]);
        if (eu || ev) return eu && ev;
        if (text[su + k] != text[sv + k]) return false;
    }
}
// the n-grams whose first words have the ranks ra and rb, both inside a document that ends at de
__device__ __forceinline__ bool wg_same(const WgArgs& a, int64_t ra, int64_t rb, int n, int64_t de) {
    if (ra == rb) return true;
    for (int j = 0; j < n; ++j)
        if (!wg_word_equal(a.text, a.rec[ra + j], a.rec[rb + j], de)) return false;
    return true;
}

// ---- short documents: one workgroup, a table in LDS -------------------------------------------------------------------------------------
struct WgLds {
    uint64_t hw[WG_LDS_WORDS];                          // the words' hashes
    unsigned int key[2 * WG_LDS_WORDS], cnt[2 * WG_LDS_WORDS];  // a slot: 22 bits of tag (never 0) above the occurrence that claimed it; its count
    uint16_t occ[WG_LDS_WORDS];                         // an occurrence's slot
    uint8_t flag[WG_LDS_WORDS];                         // its n-gram occurs twice
    long long red[RP_WAVES];
};
static_assert(WG_LDS_WORDS <= 1024 && 2 * WG_LDS_WORDS <= 65536, "an occurrence is 10 bits of a slot's word, a slot 16 bits of occ");

// the document D of W words (2 <= W <= WG_LDS_WORDS), by the whole workgroup
__device__ __forceinline__ void wg_short_doc(const WgArgs& a, WgLds& s, int64_t D, int W) {
    const int tid = threadIdx.x;
    const int64_t f = a.first_word[D], de = a.doc_off[D + 1];
    unsigned long long* row = a.stats + D * WG_COLS;
    __syncthreads();  // (the document before is done with s)
    for (int i = tid; i < W; i += RW_THREADS) s.hw[i] = a.rec[f + i].h;
    for (int n = WG_TOP_LO; n <= WG_DUP_HI && n <= W; ++n) {
        if (!wg_asked(a.groups, n)) continue;
        const int occs = W - n + 1;
        unsigned smask = 63;
        while (smask + 1 < 2u * (unsigned)occs) smask = 2 * smask + 1;
        __syncthreads();  // (hw is there; the n before is done with the table)
        for (unsigned i = tid; i <= smask; i += RW_THREADS) s.key[i] = s.cnt[i] = 0;
        __syncthreads();
        for (int i = tid; i < occs; i += RW_THREADS) {
            const uint64_t key = wg_key([&](int j) { return s.hw[i + j]; }, n, D);
            const unsigned word = ((unsigned)(key >> 42) | 1u) << 10 | (unsigned)i;
            unsigned slot = (unsigned)key & smask;
            for (unsigned c = 0; c <= smask; ++c, slot = (slot + 1) & smask) {
                unsigned cur = __hip_atomic_load(&s.key[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (cur == 0) {
                    cur = atomicCAS(&s.key[slot], 0u, word);
                    if (cur == 0) break;
                }
                if ((cur ^ word) >> 10) continue;  // another tag
                if (wg_same(a, f + i, f + (cur & 1023u), n, de)) break;
            }
            atomicAdd(&s.cnt[slot], 1u);
            s.occ[i] = (uint16_t)slot;
        }
        __syncthreads();
        if (n <= WG_TOP_HI) {
            long long best = 0, chars = 0;
            for (int i = tid; i < occs; i += RW_THREADS) best = max(best, (long long)s.cnt[s.occ[i]]);
            best = block_max(best, s.red);
            for (int i = tid; i < occs; i += RW_THREADS)
                if ((long long)s.cnt[s.occ[i]] == best) chars = max(chars, (long long)(a.cum[f + i + n] - a.cum[f + i]));
            chars = block_max(chars, s.red);
            if (tid == 0) {
                row[wg_col(n)] = (unsigned long long)best;
                row[wg_col(n) + 1] = (unsigned long long)chars;
            }
        } else {
            for (int i = tid; i < W; i += RW_THREADS) s.flag[i] = i < occs && s.cnt[s.occ[i]] >= 2;
            __syncthreads();
            long long sum = 0;
            for (int j = tid; j < W; j += RW_THREADS) {
                bool covered = false;
                for (int k = j - n + 1 < 0 ? 0 : j - n + 1; k <= j; ++k) covered |= s.flag[k] != 0;
                if (covered) sum += (long long)(a.cum[f + j + 1] - a.cum[f + j]);
            }
            sum = block_sum(sum, s.red);
            if (tid == 0) row[wg_col(n)] = (unsigned long long)sum;
        }
    }
}

__global__ __launch_bounds__(RW_THREADS) void td_wg_short(const WgArgs a) {
    __shared__ WgLds s;
    __shared__ int s_w[WG_DOC_BLOCK];
    if (wg_stopped(a)) return;
    const int tid = threadIdx.x;
    const long long most = (a.wflags & WG_NO_LDS) ? 0 : WG_LDS_WORDS;
    for (int64_t base = blockIdx.x * (int64_t)WG_DOC_BLOCK; base < a.n_docs; base += gridDim.x * (int64_t)WG_DOC_BLOCK) {
        __syncthreads();  // (the block before has read s_w)
        if (tid < WG_DOC_BLOCK) {
            const int64_t d = base + tid;
            int w = 0;
            if (d < a.n_docs) {
                const long long f = a.first_word[d], W = a.first_word[d + 1] - f;
                a.stats[d * WG_COLS + WG_WORDS] = (unsigned long long)W;
                a.stats[d * WG_COLS + WG_WORD_CHARS] = a.cum[f + W] - a.cum[f];
                if (W >= WG_TOP_LO && W <= most) w = (int)W;
            }
            s_w[tid] = w;
        }
        __syncthreads();
        for (int k = 0; k < WG_DOC_BLOCK; ++k)
            if (s_w[k]) wg_short_doc(a, s, base + k, s_w[k]);
    }
}

// ---- long documents: a lane an occurrence, one table in global memory -----------------------------------------------------------------------
// the q-th word of the global path: its document, the document's first word and words, the word's place in it
struct WgOcc {
    int64_t D, f, W, j;
};
__device__ __forceinline__ WgOcc wg_locate(const WgArgs& a, int64_t q, int64_t n_long) {
    int64_t lo = 0, hi = n_long;  // the last entry of long_first[0, n_long) at or below q
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (a.long_first[mid] <= q) lo = mid;
        else hi = mid;
    }
    WgOcc o;
    o.D = a.long_doc[lo];
    o.f = a.first_word[o.D];
    o.W = a.first_word[o.D + 1] - o.f;
    o.j = q - a.long_first[lo];
    return o;
}

__global__ __launch_bounds__(RW_THREADS) void td_wg_insert(const WgArgs a) {
    if (wg_stopped(a)) return;
    const int64_t n_words = (int64_t)a.lhead[WG_L_WORDS], n_long = (int64_t)a.lhead[WG_L_DOCS];
    const uint64_t mask = a.head[RP_H_MASK];
    const int n = a.n;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n_words; q += (int64_t)gridDim.x * blockDim.x) {
        const WgOcc o = wg_locate(a, q, n_long);
        if (o.j + n > o.W) continue;
        const int64_t r = o.f + o.j, de = a.doc_off[o.D + 1];
        const uint64_t key = wg_key([&](int j) { return a.rec[r + j].h; }, n, o.D), word = wg_slot_word(key, r);
        uint64_t slot = key & mask;
        // (the table has more slots than the call has occurrences, so an empty one is met; the walk is bounded by the slots all the same)
        for (uint64_t c = 0; c <= mask; ++c, slot = (slot + 1) & mask) {
            unsigned long long cur = __hip_atomic_load(&a.table[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == 0) {
                cur = atomicCAS(&a.table[slot], 0ull, (unsigned long long)word);
                if (cur == 0) break;
            }
            if ((cur ^ word) >> RP_START_BITS) continue;  // another tag
            const int64_t rb = (int64_t)(cur & ((1ull << RP_START_BITS) - 1));
            if (rb < o.f || rb + n > o.f + o.W) continue;  // another document
            if (wg_same(a, r, rb, n, de)) break;
        }
        __hip_atomic_fetch_add(&a.cnt[slot], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        a.occ[r] = slot;
    }
}

__global__ __launch_bounds__(RW_THREADS) void td_wg_count(const WgArgs a) {
    if (wg_stopped(a)) return;
    const int64_t n_words = (int64_t)a.lhead[WG_L_WORDS], n_long = (int64_t)a.lhead[WG_L_DOCS];
    const int n = a.n;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n_words; q += (int64_t)gridDim.x * blockDim.x) {
        const WgOcc o = wg_locate(a, q, n_long);
        const int64_t r = o.f + o.j;
        unsigned long long c = 0;
        if (o.j + n <= o.W) a.occ[r] = c = a.cnt[a.occ[r]];
        if (n > WG_TOP_HI) a.flag[r] = c >= 2;
        else if (c) atomicMax(a.stats + o.D * WG_COLS + wg_col(n), c);
    }
}

// n == 0: the table's clearing alone (in front of the first n)
__global__ __launch_bounds__(RW_THREADS) void td_wg_cover(const WgArgs a) {
    if (wg_stopped(a)) return;
    const int64_t n_words = (int64_t)a.lhead[WG_L_WORDS], n_long = (int64_t)a.lhead[WG_L_DOCS];
    if (!n_words) return;
    const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    const int n = a.n;
    for (int64_t i = gid; i <= (int64_t)a.head[RP_H_MASK]; i += step) a.table[i] = a.cnt[i] = 0;  // (nobody reads the table here)
    if (!n) return;
    for (int64_t q0 = gid - threadIdx.x % 64; q0 < n_words; q0 += step) {  // (a wavefront stays together)
        const int64_t q = q0 + threadIdx.x % 64;
        const bool in = q < n_words;
        WgOcc o = WgOcc{-1, 0, 0, 0};
        if (in) o = wg_locate(a, q, n_long);
        const int64_t r = o.f + o.j;
        if (n <= WG_TOP_HI) {
            if (in && o.j + n <= o.W && a.occ[r] == a.stats[o.D * WG_COLS + wg_col(n)])
                atomicMax(a.stats + o.D * WG_COLS + wg_col(n) + 1, a.cum[r + n] - a.cum[r]);
            continue;
        }
        long long v = 0;
        if (in) {
            bool covered = false;
            for (int64_t k = o.j - n + 1 < 0 ? 0 : o.j - n + 1; k <= o.j; ++k) covered |= a.flag[o.f + k] != 0;
            if (covered) v = (long long)(a.cum[r + 1] - a.cum[r]);
        }
        // a wavefront whose words lie in one document adds once
        const bool one = __all(in && (long long)o.D == __shfl((long long)o.D, 0));
        if (one)
            for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
        if (v && (!one || threadIdx.x % 64 == 0))
            __hip_atomic_fetch_add(a.stats + o.D * WG_COLS + wg_col(n), (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(RW_THREADS) void td_wg_totals(const WgArgs a) {
    __shared__ long long s_red[RP_WAVES];
    if (wg_stopped(a) || !a.totals) return;
    long long v[WG_COLS];
    for (int c = 0; c < WG_COLS; ++c) v[c] = 0;
    for (int64_t d = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; d < a.n_docs; d += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long* row = a.stats + d * WG_COLS;
#pragma unroll
        for (int c = 0; c < WG_COLS; ++c) v[c] = wg_col_is_max(c) ? max(v[c], (long long)row[c]) : v[c] + (long long)row[c];
    }
#pragma unroll
    for (int c = 0; c < WG_COLS; ++c) {
        const long long r = wg_col_is_max(c) ? block_max(v[c], s_red) : block_sum(v[c], s_red);
        if (threadIdx.x != 0 || !r) continue;
        if (wg_col_is_max(c)) atomicMax(a.totals + c, (unsigned long long)r);
        else __hip_atomic_fetch_add(a.totals + c, (unsigned long long)r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace

hipError_t launch_word_ngrams(const WgArgs& a, hipStream_t stream) {
    hipError_t e;
    if ((e = rewrite_launch(td_wg_docs, rewrite_grid(a.n_docs + 1, RW_THREADS, 4096), a, stream)) != hipSuccess) return e;
    const unsigned tiles = rewrite_grid(a.n_bytes + 16, RW_TILE, RW_MAX_GRID);
    if ((e = rewrite_launch(td_wg_summary, tiles, a, stream)) != hipSuccess) return e;
    if ((e = rewrite_launch(td_rp_prefix, 1, static_cast<const RpArgs&>(a), stream)) != hipSuccess) return e;
    if ((e = rewrite_launch(td_wg_reset, rewrite_grid(a.n_docs * WG_COLS + WG_COLS, 4 * RW_THREADS, 4096), a, stream)) != hipSuccess) return e;
    if ((e = rewrite_launch(td_wg_tiles, tiles, a, stream)) != hipSuccess) return e;
    if ((e = rewrite_launch(td_wg_long, 1, a, stream)) != hipSuccess) return e;
    if ((e = rewrite_launch(td_wg_short, rewrite_grid(a.n_docs, WG_DOC_BLOCK, RW_MAX_GRID), a, stream)) != hipSuccess) return e;
    const unsigned lanes = rewrite_grid(a.max_units, RW_THREADS, WG_MAX_GRID);
    WgArgs b = a;
    b.n = 0;
    if ((e = rewrite_launch(td_wg_cover, lanes, b, stream)) != hipSuccess) return e;
    for (b.n = WG_TOP_LO; b.n <= WG_DUP_HI; ++b.n) {
        if (!wg_asked(a.groups, b.n)) continue;
        if ((e = rewrite_launch(td_wg_insert, lanes, b, stream)) != hipSuccess) return e;
        if ((e = rewrite_launch(td_wg_count, lanes, b, stream)) != hipSuccess) return e;
        if ((e = rewrite_launch(td_wg_cover, lanes, b, stream)) != hipSuccess) return e;
    }
    return rewrite_launch(td_wg_totals, rewrite_grid(a.n_docs, RW_THREADS, 1024), a, stream);
}

}  // namespace td
