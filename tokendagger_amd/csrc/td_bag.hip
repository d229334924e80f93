// Bag models (td_bag_classify_device and what ends in it): text + document offsets + a model -> each document's best label, its
// probability, optionally all probabilities and the hidden vector, and stats[n_docs][BAG_COLS].  The rule is the contract in
// include/tokendagger_hip.h; td_bag_args.h has the delimiters, the hash, the n-gram walks and the dictionary's table, which the model's
// builder and the host statement (td_bag_classify_host) compile too.
//
// The windows, the tiles, the offsets check and the tile's table of documents are the text passes' frame (td_rewrite_common.h).  A token
// is at most 1024 bytes, so a tile decides every token that STARTS in it from its own bytes, one byte in front and 1024 behind; nothing
// is carried from tile to tile.  A call is
//   td_bag_docs      the frame's offsets check
//   td_bag_tiles<0>  a workgroup a tile.  The lanes put their windows, the halo and every window's 16-bit delimiter mask (dword tests:
//                    ma_in, ma_eq, ma_pack) into LDS.  A token starts at a non-delimiter behind a delimiter or a document's start; its end
//                    is the first set bit of the masks behind it, read 64 bytes a step, or the document's end.  COUNT: the kept tokens
//                    (at most 1024 bytes) of the tile go to tile_base[t].
//   td_bag_scan      ONE workgroup: tile_base to its exclusive prefixes; the call's records
//   td_bag_reset     stats and totals 0; first[] of the documents at the text's end
//   td_bag_tiles<1>  WRITE: the same, then a workgroup scan places the kept tokens; a lane walks each of its tokens once in LDS for the
//                    hash, probes the dictionary (a table word's tag first, then the bytes) and writes one 16-byte record {start, length,
//                    hash, word or -1} at the token's rank.  The lane that holds a document's first byte writes first[] of it and of the
//                    empty documents in front of it; skipped tokens are added to LONG.
//   td_bag_features  A UNIT is a token's record or, behind a document's last one under TD_BAG_EOS, its "</s>" (never stored: its place
//                    follows from first[]).  A wavefront takes a CHUNK of BAG_CHUNK consecutive units, whatever the grid.  It works in
//                    ROUNDS: every lane puts up to eight row ids into LDS, a wavefront scan packs them into a queue in the lanes'
//                    order, and the wavefront drains the queue with the lanes across the columns: a lane holds one float4 (two above
//                    256 columns) and 64 / lanes-a-row rows are loaded a step with 16-byte loads; queue entry q goes to lane group
//                    q mod groups.  Without character n-grams a round is 64 units, a lane a unit (the word row and the word n-grams
//                    from the next N - 1 records of the document); with them a round is 64 positions of one token, a lane a position
//                    of '<' + token + '>' with one incremental walk of up to maxn characters (position 0 in front of them: the word row
//                    and the word n-grams).  Where a document ends, or the chunk, the groups are folded by a fixed tree of shuffles: a
//                    document inside one chunk is finished there (hsum), one that reaches beyond leaves a partial (part[chunk][0]: it
//                    began at or before the chunk's first unit, [1]: later).  FEATURES and IN_VOCAB go to stats by integer adds.
//   td_bag_output    a workgroup a document: the partials of a document that spans chunks are added in chunk order; hidden = sum / n;
//                    a lane a label: the logits by plain FMAs over the transposed output layer (coalesced), then softmax (maximum,
//                    sum), a sigmoid a label, or the tree's paths from a table; the best label by a fixed reduction (ties: the lowest
//                    index).  d_probs is written only where it is asked for.
//   td_bag_totals    a lane a document: the columns' sums
// No floating-point atomics: every sum's order is fixed by the text and the model.  Nothing outside text[0, doc_off[n_docs]) and
// doc_off[0, n_docs] is read.  No kernel waits for another workgroup.
#include <hip/hip_runtime.h>

#include "td_bag.h"
#include "td_rewrite_common.h"

namespace td {

namespace {

constexpr int BAG_WAVES = RW_THREADS / 64;
constexpr int BAG_FRONT = 16;                         // s_txt[BAG_FRONT + r]: byte r of the tile; s_txt[BAG_FRONT - 1]: the byte in front
constexpr int BAG_HALO = BAG_TOKEN_BYTES;             // bytes behind the tile: a token of 1024 bytes that starts at the tile's last byte
constexpr int BAG_TXT = BAG_FRONT + RW_TILE + BAG_HALO;
constexpr int BAG_DM = (RW_TILE + BAG_HALO) / 16;     // the windows' delimiter masks
constexpr int BAG_ROWS = 8;                           // row ids a lane puts up in a round
constexpr int BAG_MAX_GRID = 2048;
static_assert(BAG_HALO % 64 == 0 && BAG_DM % 4 == 0 && BAG_HALO / 16 <= RW_THREADS, "the masks are read 64 bytes at a time; a lane a halo window");
static_assert(BAG_MAX_N <= BAG_ROWS && BAG_MAX_WORD_NGRAMS <= BAG_ROWS, "a position's character n-grams, a unit's word row and word n-grams");
static_assert(RC_LDS_DOCS * 4 + BAG_TXT + BAG_DM * 2 + 256 <= 160 * 1024 / 6, "six workgroups a CU");

__device__ __forceinline__ void bag_add(unsigned long long* p, unsigned long long v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool bag_stopped(const BagArgs& a) { return a.head[RW_H_BAD] != 0; }

__device__ __forceinline__ uint32_t bag_delim_mask(const uint32_t w[4]) {  // bit k: byte k of the window is a delimiter
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) m |= ma_pack(ma_in(w[j], 9, 13) | ma_eq(w[j], 0x20) | ma_eq(w[j], 0)) << 4 * j;
    return m;
}

// The length of the token at byte r of the tile, at most lim (1 <= lim <= 1025): the first delimiter behind r, 64 bytes a step.
__device__ __forceinline__ int bag_token_len(const uint16_t* s_dm, int r, int lim) {
    const uint64_t* m = reinterpret_cast<const uint64_t*>(s_dm);
    int wi = r >> 6;  // (r + lim <= RW_TILE + BAG_HALO: no word behind BAG_DM / 4 - 1 is read)
    uint64_t x = m[wi] >> (r & 63);
    int len = 64 - (r & 63);
    if (x) return min(__builtin_ctzll(x), lim);
    while (len < lim) {
        x = m[++wi];
        if (x) return min(len + __builtin_ctzll(x), lim);
        len += 64;
    }
    return lim;
}

__global__ __launch_bounds__(RW_THREADS) void td_bag_docs(const BagArgs a) {
    rewrite_docs(a, blockIdx.x * (int64_t)blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

template <int MODE>
__global__ __launch_bounds__(RW_THREADS) void td_bag_tiles(const BagArgs a) {
    __shared__ int32_t s_off[RC_LDS_DOCS];
    __shared__ __attribute__((aligned(16))) uint8_t s_txt[BAG_TXT];
    __shared__ __attribute__((aligned(8))) uint16_t s_dm[BAG_DM];
    __shared__ long long s_red[BAG_WAVES];
    if (rewrite_bad_offsets(a, MODE == 0)) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t total = a.doc_off[a.n_docs];
    const int shift = (int)(((uintptr_t)a.text) & 15);
    const int64_t ntiles = total > 0 ? (total + shift + RW_TILE - 1) / RW_TILE : 0;
    const auto off_of = [off = a.doc_off](int64_t d) { return off[d]; };
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const RwTile tl = rw_tile(t, shift, total);
        const int64_t b0 = tl.base + 16 * tid, b = b0 < 0 ? 0 : b0, we = b0 + 16 < total ? b0 + 16 : total;
        const bool owns = b < we;
        const int k0 = (int)(b - b0), k1 = (int)(we - b0);
        uint32_t w[4] = {0, 0, 0, 0};
        if (owns) rw_load(a.text, b0, b, we, w);
        const uint32_t dm = bag_delim_mask(w);  // (what lies outside the text is 0 here: a delimiter)
        __syncthreads();                        // (the tile before has read its bytes, masks and table)
        *reinterpret_cast<uint4*>(s_txt + BAG_FRONT + 16 * tid) = make_uint4(w[0], w[1], w[2], w[3]);
        s_dm[tid] = (uint16_t)dm;
        if (tid < BAG_HALO / 16) {
            const int64_t x0 = tl.base + RW_TILE + 16 * tid, xe = x0 + 16 < total ? x0 + 16 : total;
            uint32_t xw[4] = {0, 0, 0, 0};
            if (x0 < xe) rw_load(a.text, x0, x0, xe, xw);
            *reinterpret_cast<uint4*>(s_txt + BAG_FRONT + RW_TILE + 16 * tid) = make_uint4(xw[0], xw[1], xw[2], xw[3]);
            s_dm[RW_THREADS + tid] = (uint16_t)bag_delim_mask(xw);
        }
        if (tid == 72) s_txt[BAG_FRONT - 1] = tl.base > 0 ? a.text[tl.base - 1] : (uint8_t)0;
        const RwTable tb = rw_table(s_off, off_of, a.n_docs, tl);
        __syncthreads();
        const int64_t ds0 = a.doc_off[tb.kb], de0 = a.doc_off[tb.kb + 1];
        const bool uni = ds0 <= tl.t0 && de0 >= tl.s1;  // the common case: the whole tile lies in one document
        // ---- the START bits: no delimiter, behind a delimiter or at a document's start ----
        const uint32_t whole = owns ? ((1u << k1) - 1u) & ~((1u << k0) - 1u) : 0u;
        uint32_t pred = (__shfl(dm, (lane + 63) & 63) >> 15) & 1u;
        if (lane == 0) pred = bag_delim(s_txt[BAG_FRONT + 16 * tid - 1]);
        int64_t kf = 0;  // the first document that starts at or behind b (not uni)
        uint32_t dstart = 0;
        if (owns && uni) {
            if (b == ds0) dstart = 1u << k0;
        } else if (owns) {
            kf = rw_doc_of(a.doc_off, s_off, tb, tl.t0, b);
            while (kf > 0 && a.doc_off[kf - 1] >= b) --kf;  // (the empty documents at b in front of it)
            for (int64_t k = kf; k < a.n_docs; ++k) {
                const int64_t s = a.doc_off[k];
                if (s >= we) break;
                if (s >= b) dstart |= 1u << (int)(s - b0);
            }
        }
        const uint32_t starts = ~dm & ((dm << 1) | pred | dstart) & whole;
        // ---- the tokens' lengths: kept ones and skipped ones ----
        const auto doc_at = [&](int64_t p) { return uni ? tb.kb : rw_doc_of(a.doc_off, s_off, tb, tl.t0, p); };
        uint32_t kept = 0;
        for (uint32_t x = starts; x; x &= x - 1) {
            const int k = __builtin_ctz(x), r = 16 * tid + k;
            const int64_t p = tl.base + r, D = doc_at(p), room = a.doc_off[D + 1] - p;
            const int lim = room < BAG_TOKEN_BYTES + 1 ? (int)room : BAG_TOKEN_BYTES + 1;
            if (bag_token_len(s_dm, r, lim) <= BAG_TOKEN_BYTES) kept |= 1u << k;
            else if (MODE == 1) bag_add(a.stats + D * BAG_COLS + BAG_LONG, 1ull);
        }
        long long n_kept;
        const long long at = block_excl(__builtin_popcount(kept), s_red, n_kept);
        if (MODE == 0) {
            if (tid == 0) a.tile_base[t] = (unsigned long long)n_kept;
            continue;
        }
        // ---- WRITE: a record a kept token, first[] of the documents that start in the window ----
        long long rank = (long long)a.tile_base[t] + at;
        const long long rank0 = rank;
        for (uint32_t x = kept; x; x &= x - 1, ++rank) {
            const int k = __builtin_ctz(x), r = 16 * tid + k;
            const int64_t p = tl.base + r, room = a.doc_off[doc_at(p) + 1] - p;
            const int L = bag_token_len(s_dm, r, room < BAG_TOKEN_BYTES ? (int)room : BAG_TOKEN_BYTES);
            const uint8_t* tx = s_txt + BAG_FRONT + r;  // (r + L <= RW_TILE - 1 + BAG_HALO)
            uint32_t h = BAG_HASH_INIT;
#pragma unroll 1
            for (int j = 0; j < L; ++j) h = bag_step(h, tx[j]);
            const int32_t word = bag_lookup(a.m.dict, [tx](int j) { return tx[j]; }, L, h);
            if (rank < a.max_recs) a.rec[rank] = BagRec{(uint64_t)p << 11 | (uint64_t)L, h, word};
        }
        if (owns && uni) {
            if (b == ds0) a.first[tb.kb] = rank0;
        } else if (owns) {
            for (int64_t k = kf; k < a.n_docs; ++k) {
                const int64_t s = a.doc_off[k];
                if (s >= we) break;
                if (s >= b) a.first[k] = rank0 + __builtin_popcount(kept & ((1u << (int)(s - b0)) - 1u));
            }
        }
    }
}

__global__ __launch_bounds__(RW_THREADS) void td_bag_scan(const BagArgs a) {
    __shared__ long long s_wave[BAG_WAVES];
    if (bag_stopped(a)) return;
    const int64_t total = a.doc_off[a.n_docs];
    const int shift = (int)(((uintptr_t)a.text) & 15);
    const int64_t ntiles = total > 0 ? (total + shift + RW_TILE - 1) / RW_TILE : 0;
    long long carry[1];
    chunks_excl_scan<1>(a.tile_base, ntiles, s_wave, carry);
    if (threadIdx.x == 0) a.bhead[BAG_H_RECS] = (unsigned long long)carry[0];
}

__global__ __launch_bounds__(RW_THREADS) void td_bag_reset(const BagArgs a) {
    if (bag_stopped(a)) return;
    const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    if (a.totals && gid < BAG_COLS) a.totals[gid] = 0;
    for (int64_t i = gid; i < a.n_docs * BAG_COLS; i += step) a.stats[i] = 0;
    // the documents that start at the text's end (the entry behind the last one among them): no window holds them
    const int64_t total = a.doc_off[a.n_docs];
    const long long recs = (long long)a.bhead[BAG_H_RECS];
    for (int64_t d = gid; d <= a.n_docs; d += step)
        if (a.doc_off[d] == total) a.first[d] = recs;
}

// ---- the features ---------------------------------------------------------------------------------------------------------------------------
struct BagAcc {
    float4 lo, hi;  // columns 4 v .. 4 v + 3 and, above 256 columns, 4 (v + 64) ..
};
__device__ __forceinline__ void bag_add4(float4& x, const float4& y) {
    x.x += y.x; x.y += y.y; x.z += y.z; x.w += y.w;
}
__device__ __forceinline__ float4 bag_shfl4(const float4& x, int d) {
    return make_float4(__shfl_xor(x.x, d), __shfl_xor(x.y, d), __shfl_xor(x.z, d), __shfl_xor(x.w, d));
}
__device__ __forceinline__ void bag_lds_fence() {  // a wavefront's LDS writes are seen by its own lanes
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(RW_THREADS) void td_bag_features(const BagArgs a) {
    __shared__ uint32_t s_raw[BAG_WAVES][64 * BAG_ROWS];
    __shared__ uint32_t s_q[BAG_WAVES][64 * BAG_ROWS];
    if (bag_stopped(a)) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t* raw = s_raw[wv];
    uint32_t* q = s_q[wv];
    const BagModel& M = a.m;
    const int64_t eos = (a.call_flags & BAG_EOS) ? 1 : 0;
    const int64_t recs = (int64_t)a.bhead[BAG_H_RECS], units = recs + eos * a.n_docs, nchunks = (units + BAG_CHUNK - 1) / BAG_CHUNK;
    const auto ufirst = [&](int64_t d) { return (int64_t)a.first[d] + eos * d; };
    // the lanes across the columns
    const int nvec = M.dimp / 4;
    int per = 1;  // lanes a row (a power of two)
    while (per < nvec && per < 64) per <<= 1;
    const int groups = 64 / per, g = lane / per, v = lane % per;
    const bool lo_on = v < nvec, hi_on = v + 64 < nvec;
    const uint32_t eos_hash = bag_eos_hash();
    for (int64_t c = blockIdx.x * (int64_t)BAG_WAVES + wv; c < nchunks; c += (int64_t)gridDim.x * BAG_WAVES) {
        const int64_t u0 = c * BAG_CHUNK, u1 = u0 + BAG_CHUNK < units ? u0 + BAG_CHUNK : units;
        // the document of u0: the last one whose first unit is at or below it (so none without units)
        int64_t D = last_le_global(ufirst, 0, a.n_docs, u0);
        for (int64_t us = ufirst(D); us < u1; ++D, us = ufirst(D)) {  // (D < n_docs: ufirst(n_docs) = units >= u1)
            const int64_t ue = ufirst(D + 1);
            if (ue <= us) continue;
            const int64_t m = ue - us, f0 = (int64_t)a.first[D], s0 = us > u0 ? us : u0, s1 = ue < u1 ? ue : u1;
            BagAcc A = {make_float4(0, 0, 0, 0), make_float4(0, 0, 0, 0)};
            unsigned long long n_rows = 0, n_voc = 0;
            const auto hash_of = [&](int64_t k) { return eos && k == m - 1 ? eos_hash : a.rec[f0 + k].hash; };
            // unit j's own rows: its word, then the word n-grams that begin with it
            const auto unit_rows = [&](int64_t j, int32_t word, auto emit) {
                if (word >= 0) emit((uint32_t)word);
                if (M.word_ngrams > 1)
                    bag_wordgrams_at(hash_of, m, j, M.word_ngrams, [&](uint64_t h) { emit((uint32_t)(M.nwords + (int64_t)(h % (uint64_t)M.bucket))); });
            };
            // one round: fill(emit) in every lane, the queue in the lanes' order, the drain
            const auto round = [&](auto fill) {
                int cnt = 0;
                fill([&](uint32_t row) {
                    if (cnt < BAG_ROWS) raw[lane * BAG_ROWS + cnt++] = row;
                });
                const int incl = wave_incl_scan(cnt, lane, [](int x, int y) { return x + y; });
                const int T = __shfl(incl, 63);
                bag_lds_fence();  // (the round before has read the queue)
                for (int i = 0; i < cnt; ++i) q[incl - cnt + i] = raw[lane * BAG_ROWS + i];
                bag_lds_fence();
                for (int q0 = 0; q0 < T; q0 += groups) {
                    const int qi = q0 + g;
                    if (qi < T) {
                        const float4* src = reinterpret_cast<const float4*>(M.win + (int64_t)q[qi] * M.dimp);
                        if (lo_on) bag_add4(A.lo, src[v]);
                        if (hi_on) bag_add4(A.hi, src[v + 64]);
                    }
                }
                n_rows += (unsigned long long)T;
            };
            if (M.maxn == 0) {  // a lane a unit
                for (int64_t ub = s0; ub < s1; ub += 64) {
                    const int64_t j = ub + lane - us;
                    const bool on = ub + lane < s1;
                    int32_t word = -1;
                    if (on) word = eos && j == m - 1 ? M.eos_idx : a.rec[f0 + j].word;
                    n_voc += (unsigned long long)__builtin_popcountll(__ballot(word >= 0));
                    round([&](auto emit) {
                        if (on) unit_rows(j, word, emit);
                    });
                }
            } else {  // a lane a position of one unit
                for (int64_t u = s0; u < s1; ++u) {
                    const int64_t j = u - us;
                    const bool is_eos = eos && j == m - 1;
                    int32_t word = M.eos_idx;
                    int n_s = 0;
                    const uint8_t* tk = a.text;
                    if (!is_eos) {
                        const BagRec R = a.rec[f0 + j];
                        const int L = (int)(R.start_len & 2047u);
                        tk = a.text + (R.start_len >> 11);
                        word = R.word;
                        const bool lit = L == 4 && tk[0] == '<' && tk[1] == '/' && tk[2] == 's' && tk[3] == '>';
                        n_s = lit ? 0 : L + 2;
                    }
                    n_voc += word >= 0;
                    const auto s = [&](int k) -> uint32_t { return k == 0 ? '<' : k == n_s - 1 ? '>' : tk[k - 1]; };
                    for (int pb = 0; pb < n_s + 1; pb += 64) {  // position 0: the unit's own rows; position i + 1: s[i]
                        const int p = pb + lane;
                        round([&](auto emit) {
                            if (p == 0) unit_rows(j, word, emit);
                            else if (p <= n_s) bag_chargrams_at(s, n_s, p - 1, M.minn, M.maxn, [&](uint32_t h) { emit((uint32_t)(M.nwords + (int64_t)(h % (uint32_t)M.bucket))); });
                        });
                    }
                }
            }
            // the groups' sums by a fixed tree; to the document's sum, or to the chunk's partial of it
            for (int d = 32; d >= per; d >>= 1) {
                bag_add4(A.lo, bag_shfl4(A.lo, d));
                bag_add4(A.hi, bag_shfl4(A.hi, d));
            }
            float* dst = us >= u0 && ue <= u1 ? a.hsum + D * M.dimp : a.part + (c * 2 + (us <= u0 ? 0 : 1)) * M.dimp;
            if (g == 0 && lo_on) reinterpret_cast<float4*>(dst)[v] = A.lo;
            if (g == 0 && hi_on) reinterpret_cast<float4*>(dst)[v + 64] = A.hi;
            if (lane == 0) {
                if (n_rows) bag_add(a.stats + D * BAG_COLS + BAG_FEATURES, n_rows);
                if (n_voc) bag_add(a.stats + D * BAG_COLS + BAG_IN_VOCAB, n_voc);
            }
        }
    }
}

// ---- the output layer -------------------------------------------------------------------------------------------------------------------
struct BagBest {
    float v;
    int l;
};
__device__ __forceinline__ BagBest bag_better(const BagBest& x, const BagBest& y) {  // the larger value; a tie: the lower index
    return y.v > x.v || (y.v == x.v && y.l < x.l) ? y : x;
}
// the workgroup's maximum / sum / best, in a fixed order, in every lane
__device__ __forceinline__ float bag_block_max(float x, float* s_red) {
    for (int d = 32; d >= 1; d >>= 1) x = fmaxf(x, __shfl_xor(x, d));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = x;
    __syncthreads();
    float r = s_red[0];
    for (int w = 1; w < BAG_WAVES; ++w) r = fmaxf(r, s_red[w]);
    return r;
}
__device__ __forceinline__ float bag_block_sum(float x, float* s_red) {
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = x;
    __syncthreads();
    float r = s_red[0];
    for (int w = 1; w < BAG_WAVES; ++w) r += s_red[w];
    return r;
}
__device__ __forceinline__ BagBest bag_block_best(BagBest x, BagBest* s_best) {
    for (int d = 32; d >= 1; d >>= 1) x = bag_better(x, BagBest{__shfl_xor(x.v, d), __shfl_xor(x.l, d)});
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = x;
    __syncthreads();
    BagBest r = s_best[0];
    for (int w = 1; w < BAG_WAVES; ++w) r = bag_better(r, s_best[w]);
    return r;
}
__device__ __forceinline__ float bag_log_sigmoid(float x) { return x < 0.0f ? x - log1pf(expf(x)) : -log1pf(expf(-x)); }

__global__ __launch_bounds__(RW_THREADS) void td_bag_output(const BagArgs a) {
    __shared__ float s_h[BAG_MAX_DIM];
    __shared__ float s_f[BAG_MAX_LABELS];
    __shared__ float s_red[BAG_WAVES];
    __shared__ BagBest s_best[BAG_WAVES];
    if (bag_stopped(a)) return;
    const int tid = threadIdx.x;
    const BagModel& M = a.m;
    const int64_t eos = (a.call_flags & BAG_EOS) ? 1 : 0;
    const int L = M.n_labels;
    for (int64_t d = blockIdx.x; d < a.n_docs; d += gridDim.x) {
        const int64_t us = (int64_t)a.first[d] + eos * d, ue = (int64_t)a.first[d + 1] + eos * (d + 1), m = ue - us;
        const unsigned long long n = a.stats[d * BAG_COLS + BAG_FEATURES];
        __syncthreads();  // (the document before has read s_h and s_f)
        const int64_t c0 = us / BAG_CHUNK, c1 = m > 0 ? (ue - 1) / BAG_CHUNK : c0;
        for (int c = tid; c < M.dim; c += RW_THREADS) {
            float s = 0.0f;
            if (m > 0 && c0 == c1) s = a.hsum[d * M.dimp + c];
            else if (m > 0)
                for (int64_t ch = c0; ch <= c1; ++ch) s += a.part[(ch * 2 + (us <= ch * BAG_CHUNK ? 0 : 1)) * M.dimp + c];
            const float h = n ? s / (float)n : 0.0f;
            s_h[c] = h;
            if (a.hidden) a.hidden[d * M.dim + c] = h;
        }
        if (tid == 0) a.stats[d * BAG_COLS + BAG_TOKENS] = (unsigned long long)m;
        if (!n) {  // (the same in every lane)
            if (a.probs)
                for (int l = tid; l < L; l += RW_THREADS) a.probs[d * L + l] = 0.0f;
            if (tid == 0) {
                a.best[d] = -1;
                a.best_prob[d] = 0.0f;
            }
            continue;
        }
        __syncthreads();
        for (int l = tid; l < M.n_out; l += RW_THREADS) {
            float f = 0.0f;
            for (int k = 0; k < M.dim; ++k) f = fmaf(M.wo_t[(int64_t)k * M.lpad + l], s_h[k], f);
            s_f[l] = f;
        }
        __syncthreads();
        BagBest mine = {-INFINITY, 0x7FFFFFFF};
        float scale = 1.0f, mx = 0.0f;
        if (M.loss == BAG_SOFTMAX) {
            float x = -INFINITY, z = 0.0f;
            for (int l = tid; l < L; l += RW_THREADS) x = fmaxf(x, s_f[l]);
            mx = bag_block_max(x, s_red);
            for (int l = tid; l < L; l += RW_THREADS) z += expf(s_f[l] - mx);
            scale = bag_block_sum(z, s_red);
        }
        for (int l = tid; l < L; l += RW_THREADS) {
            float p;
            if (M.loss == BAG_SOFTMAX) {
                p = expf(s_f[l] - mx) / scale;
            } else if (M.loss == BAG_OVA) {
                p = 1.0f / (1.0f + expf(-s_f[l]));
            } else {
                float lp = 0.0f;
                for (uint32_t k = M.hs_off[l]; k < M.hs_off[l + 1]; ++k) {
                    const uint32_t e = M.hs_path[k];
                    lp += bag_log_sigmoid((e & 1u) ? s_f[e >> 1] : -s_f[e >> 1]);
                }
                p = expf(lp);
            }
            if (a.probs) a.probs[d * L + l] = p;
            mine = bag_better(mine, BagBest{p, l});
        }
        const BagBest top = bag_block_best(mine, s_best);
        if (tid == 0) {
            a.best[d] = top.l;
            a.best_prob[d] = top.v;
        }
    }
}

__global__ __launch_bounds__(RW_THREADS) void td_bag_totals(const BagArgs a) {
    if (bag_stopped(a) || !a.totals) return;
    unsigned long long v[BAG_COLS] = {0, 0, 0, 0};
    for (int64_t d = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; d < a.n_docs; d += (int64_t)gridDim.x * blockDim.x)
        for (int c = 0; c < BAG_COLS; ++c) v[c] += a.stats[d * BAG_COLS + c];
    for (int c = 0; c < BAG_COLS; ++c) {
        for (int d = 32; d >= 1; d >>= 1) v[c] += (unsigned long long)__shfl_xor((long long)v[c], d);
        if ((threadIdx.x & 63) == 0 && v[c]) bag_add(a.totals + c, v[c]);
    }
}

}  // namespace

hipError_t launch_bag(const BagArgs& a, hipStream_t stream) {
    hipError_t e;
    if ((e = rewrite_launch(td_bag_docs, rewrite_grid(a.n_docs + 1, RW_THREADS, 4096), a, stream)) != hipSuccess) return e;
    const unsigned tiles = rewrite_grid(a.n_bytes + 16, RW_TILE, RW_MAX_GRID);
    if ((e = rewrite_launch(td_bag_tiles<0>, tiles, a, stream)) != hipSuccess) return e;
    if ((e = rewrite_launch(td_bag_scan, 1, a, stream)) != hipSuccess) return e;
    if ((e = rewrite_launch(td_bag_reset, rewrite_grid(a.n_docs * BAG_COLS + BAG_COLS, 4 * RW_THREADS, 4096), a, stream)) != hipSuccess) return e;
    if ((e = rewrite_launch(td_bag_tiles<1>, tiles, a, stream)) != hipSuccess) return e;
    if ((e = rewrite_launch(td_bag_features, rewrite_grid(bag_max_chunks(a.n_bytes, a.n_docs), BAG_WAVES, 16 * BAG_MAX_GRID), a, stream)) != hipSuccess) return e;
    if ((e = rewrite_launch(td_bag_output, rewrite_grid(a.n_docs, 1, 16 * BAG_MAX_GRID), a, stream)) != hipSuccess) return e;
    return rewrite_launch(td_bag_totals, rewrite_grid(a.n_docs, RW_THREADS, 1024), a, stream);
}

}  // namespace td
