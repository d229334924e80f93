// Address masking (td_mask_addresses_device and what ends in it): text + document offsets + rules -> the text with every e-mail and IPv4
// address replaced by a placeholder, its document offsets, stats[n_docs][MA_COLS] and totals.  The rule is the contract in
// include/tokendagger_hip.h; td_mask_args.h has the byte classes, the decision on an '@', the decision on a digit and the hash that picks
// the placeholder, which the host statement (td_mask_addresses_host) compiles too.  No table: everything is compares on bytes.
//
// The windows, the tiles, the offsets check, the tile's table of documents, the scan of the tiles' sizes and the cooperative copy are the
// text passes' frame (td_rewrite_common.h).  What is this pass's own: bytes are INSERTED at places that have to be found, and a match can
// begin in the tile in front and end in the tile behind.  A call is
//   td_ma_docs      the frame's offsets check
//   td_ma_reset     stats, totals and counts 0
//   td_ma_tiles<0>  MEASURE, a workgroup a tile.  A lane loads its window once and makes 16-bit masks of '@', digits, '.' and L by
//                   bit-wise tests on the four dwords.  ANCHORS: an '@'; a digit whose predecessor (the neighbouring lane's mask, one byte
//                   load at a wavefront's first lane) is not in L or lies in another document, and that has ". digit" one to three bytes
//                   behind it (the next lane's masks; at a wavefront's last lane whatever may be).  The halo, 256 bytes in front of the
//                   tile and 80 behind it, is screened the same way by 21 lanes of the first wavefront.  The lane that finds an anchor
//                   decides it from global memory (ma_email, ma_ipv4: bounded by the rule's reach and the document's edges), the halo's
//                   anchors too: nothing is exchanged between tiles and nothing is carried.  A match that touches the tile marks its
//                   bytes dead in the windows' words of LDS (atomic OR); the tile that holds its first byte also hashes it, leaves its
//                   kind and literal at that byte's slot of s_lit, a start bit and the literal's length at the window, and the
//                   per-document sums (LDS over the tile's first MA_SLOTS documents, 64-bit adds for the rest).  One __syncthreads_or:
//                   a tile with no match stores its own length and is done; any other sums live bytes + literal bytes.
//   td_ma_scan      the frame's: tile_base to its prefixes, counts[0], TD_E_CAPACITY
//   td_ma_sums      a lane a document: OUT_BYTES = length - BYTES_OUT_OF + BYTES_IN, and the columns' sums into totals
//   td_ma_tiles<1>  WRITE: a tile MEASURE found clean is one cooperative copy (and its documents' offsets); any other is decided once
//                   more, a workgroup scan places the lanes, and a lane copies its live bytes and emits the literal (from the rules in
//                   LDS) of every match that starts in its window.  The lane that has a document's first byte writes its output offset.
// There is no list of matches, so there is no bound to overflow: s_lit has a slot for every byte a match can start at.  Nothing outside
// text[0, doc_off[n_docs]) and doc_off[0, n_docs] is read.  Only stores of values that do not depend on the lanes' order and integer adds
// touch the outputs.
#include <hip/hip_runtime.h>

#include "td_mask.h"
#include "td_rewrite_common.h"

namespace td {

namespace {

constexpr int MA_WAVES = RW_THREADS / 64;
constexpr int MA_SLOTS = 32;                // documents of a tile whose sums meet in LDS
constexpr int MA_FRONT = 16, MA_BACK = 5;   // the halo's windows
static_assert(MA_FRONT * 16 >= MA_MATCH_MAX, "a match that reaches the tile has its anchor at most 253 bytes in front of it");
static_assert(MA_BACK * 16 >= MA_LOCAL_MAX + 1, "an '@' whose LOCAL begins in the tile lies at most 64 bytes behind it");
static_assert(MA_FRONT + MA_BACK <= 64, "the halo is the first wavefront's");
// the worst case a tile can hold, matches of MA_MATCH_MIN bytes back to back and one astride either seam, against the slots of s_lit
static_assert((RW_TILE + 2 * (MA_MATCH_MIN - 1)) / MA_MATCH_MIN + 1 <= RW_TILE, "a slot a start byte holds every match of a tile");
static_assert(TD_MA_MAX_LITERALS <= 8 && 16 / MA_MATCH_MIN + 1 <= 3, "s_lit: kind << 3 | literal; three starts a window at the most");

struct MaLds {  // the rules as the lanes read them: [0] e-mail, [1] IPv4
    uint8_t n[2];
    uint8_t len[2][TD_MA_MAX_LITERALS];
    uint8_t bytes[2][TD_MA_MAX_LITERALS][TD_MA_LITERAL_BYTES];
};

// by the whole workgroup; the caller's next barrier publishes it
__device__ __forceinline__ void ma_load_rules(const MaArgs& a, MaLds& s) {
    const int tid = threadIdx.x;
    for (int i = tid; i < 2 * TD_MA_MAX_LITERALS * TD_MA_LITERAL_BYTES; i += RW_THREADS) {
        const int k = i / (TD_MA_MAX_LITERALS * TD_MA_LITERAL_BYTES), j = i / TD_MA_LITERAL_BYTES % TD_MA_MAX_LITERALS, x = i % TD_MA_LITERAL_BYTES;
        s.bytes[k][j][x] = k ? a.rules.ips[j].bytes[x] : a.rules.emails[j].bytes[x];
    }
    if (tid < 2 * TD_MA_MAX_LITERALS) {
        const int k = tid / TD_MA_MAX_LITERALS, j = tid % TD_MA_MAX_LITERALS;
        s.len[k][j] = k ? a.rules.ips[j].len : a.rules.emails[j].len;
    }
    if (tid < 2) s.n[tid] = (uint8_t)(tid ? a.rules.n_ips : a.rules.n_emails);
}

// ---- a window's classes: ma_eq, ma_in and ma_pack of td_rewrite_common.h, four bits a dword ------------------------------------------------

struct MaCls {  // bit k: byte k of the window
    uint32_t at, dig, dot, L;
};
__device__ __forceinline__ MaCls ma_classes(const uint32_t w[4]) {
    MaCls c = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t x = w[j];
        const uint32_t at = ma_eq(x, '@'), dig = ma_in(x, '0', '9'), dot = ma_eq(x, '.');
        const uint32_t L = dig | dot | ma_in(x | 0x20202020u, 'a', 'z') | ma_eq(x, '-') | ma_eq(x, '_') | ma_eq(x, '%') | ma_eq(x, '+');
        c.at |= ma_pack(at) << 4 * j;
        c.dig |= ma_pack(dig) << 4 * j;
        c.dot |= ma_pack(dot) << 4 * j;
        c.L |= ma_pack(L) << 4 * j;
    }
    return c;
}
// the digits of a window that have ". digit" one to three bytes behind them; next: the masks of the window behind
__device__ __forceinline__ uint32_t ma_quad_screen(uint32_t dig, uint32_t dot, uint32_t next_dig, uint32_t next_dot) {
    const uint32_t dd = (dot | next_dot << 16) & ((dig | next_dig << 16) >> 1);
    return dig & (dd >> 1 | dd >> 2 | dd >> 3);
}

__device__ __forceinline__ void ma_add(unsigned long long* p, unsigned long long v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int64_t ma_tiles_of(const MaArgs& a, int64_t& total, int& shift) {
    total = a.doc_off[a.n_docs];
    shift = (int)(((uintptr_t)a.text) & 15);
    return total > 0 ? (total + shift + RW_TILE - 1) / RW_TILE : 0;
}

__global__ __launch_bounds__(RW_THREADS) void td_ma_docs(const MaArgs a) {
    rewrite_docs(a, blockIdx.x * (int64_t)blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

__global__ __launch_bounds__(RW_THREADS) void td_ma_reset(const MaArgs a) {
    if (a.head[RW_H_BAD]) return;
    const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    if (gid < RW_C_WORDS) a.counts[gid] = 0;
    if (a.totals && gid < MA_COLS) a.totals[gid] = 0;
    for (int64_t i = gid; i < a.n_docs * MA_COLS; i += step) a.stats[i] = 0;
}

// the output offsets of the documents that start in the window [b, we): place(k) is what the window leaves in front of its byte k
template <class Place>
__device__ __forceinline__ void ma_doc_offsets(const MaArgs& a, const int32_t* s_off, const RwTable& tb, const RwTile& tl, int64_t b0, int64_t b,
                                               int64_t we, Place place) {
    for (int64_t k = b > 0 ? rw_doc_of(a.doc_off, s_off, tb, tl.t0, b - 1) + 1 : 0; k <= a.n_docs; ++k) {
        const int64_t s = a.doc_off[k];
        if (s >= we) break;
        a.out_doc_off[k] = place((int)(s - b0));
    }
}

template <int WRITE>
__global__ __launch_bounds__(RW_THREADS) void td_ma_tiles(const MaArgs a) {
    __shared__ int32_t s_off[RC_LDS_DOCS];
    __shared__ long long s_red[MA_WAVES];
    __shared__ unsigned long long s_acc[MA_SLOTS * MA_COLS];
    __shared__ MaLds s_rules;
    __shared__ uint32_t s_mark[RW_THREADS];  // a window's bytes inside matches (bits 0 - 15) and its bytes a match starts at (bits 16 - 31)
    __shared__ uint32_t s_add[RW_THREADS];   // the literals' bytes of the matches that start in the window
    __shared__ uint8_t s_lit[RW_TILE];       // at a match's first byte: kind << 3 | literal; read only where a start bit is set
    if (rewrite_bad_offsets(a, !WRITE)) return;
    if (WRITE && a.head[RW_H_FULL]) return;
    const int tid = threadIdx.x, lane = tid & 63;
    ma_load_rules(a, s_rules);
    s_mark[tid] = 0;  // (zero again behind every tile that used them)
    s_add[tid] = 0;
    if constexpr (!WRITE)
        for (int i = tid; i < MA_SLOTS * MA_COLS; i += RW_THREADS) s_acc[i] = 0;
    int64_t total;
    int shift;
    const int64_t ntiles = ma_tiles_of(a, total, shift);
    const int flags = a.rules.flags;
    const auto off_of = [off = a.doc_off](int64_t d) { return off[d]; };
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const RwTile tl = rw_tile(t, shift, total);
        const int64_t b0 = tl.base + 16 * tid, b = b0 < 0 ? 0 : b0, we = b0 + 16 < total ? b0 + 16 : total;
        const bool owns = b < we;
        const int k0 = (int)(b - b0), k1 = (int)(we - b0);
        if constexpr (WRITE) {
            if (!a.dirty[t]) {  // (the same in every lane) no match touches the tile: its bytes as they are
                const int64_t obase = (int64_t)a.tile_base[t];
                if (a.out_doc_off) {
                    __syncthreads();  // (the tile before has read its table)
                    const RwTable tb = rw_table(s_off, off_of, a.n_docs, tl);
                    __syncthreads();
                    if (owns) ma_doc_offsets(a, s_off, tb, tl, b0, b, we, [&](int k) { return obase + (b0 + k - tl.t0); });
                }
                if (a.out) rewrite_group_copy(a.out + obase, a.text + tl.t0, tl.s1 - tl.t0);
                continue;
            }
        }
        uint32_t w[4] = {0, 0, 0, 0};
        if (owns) rw_load(a.text, b0, b, we, w);
        __syncthreads();  // (the tile before has read its table, s_lit and s_acc; s_rules, s_mark, s_add and s_acc are written)
        const RwTable tb = rw_table(s_off, off_of, a.n_docs, tl);
        __syncthreads();
        // ---- the anchors: bits 0 - 15 an '@', bits 16 - 31 a digit that may begin a quad ----
        const MaCls c = ma_classes(w);
        uint32_t pred = __shfl(c.L, (lane + 63) & 63) >> 15;
        if (lane == 0) pred = owns && b0 > 0 && ma_L(a.text[b0 - 1]);
        uint32_t nd = __shfl(c.dig, (lane + 1) & 63), ndot = __shfl(c.dot, (lane + 1) & 63);
        if (lane == 63) nd = ndot = 0xFFFFu;  // (not known here: whatever may be)
        uint32_t quad = flags & TD_MA_IPS ? ma_quad_screen(c.dig, c.dot, nd, ndot) : 0u;
        const uint32_t behind_L = (c.L << 1 | pred) & 0xFFFFu;
        if (quad & behind_L) {  // behind an L byte a quad begins at a document's start only
            uint32_t starts = 0;
            for (int64_t k = rw_doc_of(a.doc_off, s_off, tb, tl.t0, b); k <= a.n_docs; ++k) {
                const int64_t s = a.doc_off[k];
                if (s >= we) break;
                if (s >= b) starts |= 1u << (int)(s - b0);
            }
            quad &= ~behind_L | starts;
        }
        uint32_t anchors[2] = {(flags & TD_MA_EMAILS ? c.at : 0u) | quad << 16, 0u};
        int64_t from[2] = {b0, 0};
        const uint32_t dig0 = __shfl(c.dig, 0), dot0 = __shfl(c.dot, 0);
        if (tid < MA_FRONT + MA_BACK) {  // the halo: 16 windows in front of the tile, 5 behind it
            const int64_t x0 = tid < MA_FRONT ? tl.base - 16 * (MA_FRONT - tid) : tl.base + RW_TILE + 16 * (tid - MA_FRONT);
            const int64_t xb = x0 < 0 ? 0 : x0, xe = x0 + 16 < total ? x0 + 16 : total;
            if (xb < xe) {
                uint32_t xw[4];
                rw_load(a.text, x0, xb, xe, xw);
                const MaCls x = ma_classes(xw);
                from[1] = x0;
                if (flags & TD_MA_EMAILS) anchors[1] = x.at;
                if (tid == MA_FRONT - 1 && (flags & TD_MA_IPS)) {  // a quad that reaches the tile begins at most 14 bytes in front of it
                    const uint32_t xp = x0 > 0 && ma_L(a.text[x0 - 1]);
                    const int64_t r = a.doc_off[tb.kb] - x0;  // the start of the document that holds the byte in front of the tile
                    const uint32_t start = r >= 0 && r < 16 ? 1u << (int)r : 0u;
                    anchors[1] |= (ma_quad_screen(x.dig, x.dot, dig0, dot0) & (~((x.L << 1 | xp) & 0xFFFFu) | start)) << 16;
                }
            }
        }
        // ---- a lane an anchor decides it ----
        bool found = false;
        const auto put = [&](int64_t D, int col, unsigned long long v) {
            if (D - tb.kb < MA_SLOTS) atomicAdd(&s_acc[(D - tb.kb) * MA_COLS + col], v);
            else ma_add(a.stats + D * MA_COLS + col, v);
        };
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll 1
            for (uint32_t m = anchors[h]; m; m &= m - 1) {
                const int bit = __builtin_ctz(m);
                const int64_t p = from[h] + (bit & 15);
                // the one document in which a match around p can touch the tile
                const int64_t D = p < tl.t0 ? tb.kb : rw_doc_of(a.doc_off, s_off, tb, tl.t0, p < tl.s1 ? p : tl.s1 - 1);
                const int64_t ds = a.doc_off[D], de = a.doc_off[D + 1];
                if (p < ds || p >= de) continue;
                int64_t ms = p, me = p;
                int kind;
                if (bit < 16) kind = ma_email(a.text, ds, de, p, ms, me) ? MA_EMAIL : MA_NONE;
                else kind = ma_ipv4(a.text, ds, de, p, flags, me);
                if (kind == MA_NONE || me <= tl.t0 || ms >= tl.s1) continue;
                const bool mine = ms >= tl.t0;  // the tile that holds a match's first byte counts, sizes and hashes it
                if (kind == MA_IP_KEPT) {
                    if (!WRITE && mine) {
                        put(D, MA_IPS_KEPT, 1);
                        found = true;
                    }
                    continue;
                }
                found = true;
                const int r0 = (int)((mine ? ms : tl.t0) - tl.base), r1 = (int)((me < tl.s1 ? me : tl.s1) - tl.base);
                for (int win = r0 >> 4; win <= (r1 - 1) >> 4; ++win) {
                    const int lo = r0 - 16 * win > 0 ? r0 - 16 * win : 0, hi = r1 - 16 * win < 16 ? r1 - 16 * win : 16;
                    atomicOr(&s_mark[win], ((1u << hi) - 1u) & ~((1u << lo) - 1u));
                }
                if (!mine) continue;
                const int kd = kind == MA_EMAIL ? 0 : 1, li = ma_pick(a.text, ms, me, s_rules.n[kd]);
                const uint32_t ll = s_rules.len[kd][li];
                s_lit[r0] = (uint8_t)(kd << 3 | li);
                atomicOr(&s_mark[r0 >> 4], 0x10000u << (r0 & 15));
                atomicAdd(&s_add[r0 >> 4], ll);
                if constexpr (!WRITE) {
                    put(D, kd ? MA_IPS : MA_EMAILS, 1);
                    put(D, MA_BYTES_OUT_OF, (unsigned long long)(me - ms));
                    put(D, MA_BYTES_IN, ll);
                }
            }
        }
        [[maybe_unused]] const bool any = __syncthreads_or(found);
        if constexpr (!WRITE) {
            if (!any) {  // the common case: the tile is its own bytes
                if (tid == 0) {
                    a.tile_base[t] = (unsigned long long)(tl.s1 - tl.t0);
                    a.dirty[t] = 0;
                }
                continue;
            }
        }
        const uint32_t whole = owns ? ((1u << k1) - 1u) & ~((1u << k0) - 1u) : 0u;
        const uint32_t mark = s_mark[tid], add = s_add[tid];
        s_mark[tid] = 0;
        s_add[tid] = 0;
        const uint32_t live = whole & ~mark, starts = mark >> 16;
        if constexpr (!WRITE) {
            const long long sum = block_sum(__builtin_popcount(live) + add, s_red);
            if (tid == 0) {
                a.tile_base[t] = (unsigned long long)sum;
                a.dirty[t] = 1;
            }
            for (int i = tid; i < MA_SLOTS * MA_COLS; i += RW_THREADS) {
                const unsigned long long v = s_acc[i];
                if (!v) continue;
                ma_add(a.stats + (tb.kb + i / MA_COLS) * MA_COLS + i % MA_COLS, v);
                s_acc[i] = 0;
            }
        } else {
            long long sum;
            const int64_t opos = (int64_t)a.tile_base[t] + block_excl(__builtin_popcount(live) + add, s_red, sum);
            const auto lit_len = [&](int k) {
                const uint32_t code = s_lit[16 * tid + k];
                return (int)s_rules.len[code >> 3][code & 7];
            };
            if (owns && a.out_doc_off) {
                ma_doc_offsets(a, s_off, tb, tl, b0, b, we, [&](int k) {
                    int64_t o = opos + __builtin_popcount(live & ((1u << k) - 1u));
                    for (uint32_t m = starts & ((1u << k) - 1u); m; m &= m - 1) o += lit_len(__builtin_ctz(m));
                    return o;
                });
            }
            if (a.out && (live | starts)) {  // lane by lane: the live bytes, and in front of a match's first byte its literal
                uint64_t lo = w[0] | (uint64_t)w[1] << 32, hi = w[2] | (uint64_t)w[3] << 32;
                uint8_t* o = a.out + opos;
#pragma unroll 1
                for (int k = 0; k < 16; ++k) {
                    if ((starts >> k) & 1u) {
                        const uint32_t code = s_lit[16 * tid + k];
                        const uint8_t* src = s_rules.bytes[code >> 3][code & 7];
                        const int n = s_rules.len[code >> 3][code & 7];
                        for (int j = 0; j < n; ++j) *o++ = src[j];
                    }
                    if ((live >> k) & 1u) *o++ = (uint8_t)lo;
                    lo = lo >> 8 | hi << 56;
                    hi >>= 8;
                }
            }
        }
    }
}

__global__ __launch_bounds__(RW_THREADS) void td_ma_scan(const MaArgs a) { rewrite_scan(a); }

__global__ __launch_bounds__(RW_THREADS) void td_ma_sums(const MaArgs a) {
    __shared__ long long s_red[MA_WAVES];
    if (a.head[RW_H_BAD]) return;
    long long v[MA_COLS] = {0, 0, 0, 0, 0, 0};
    for (int64_t d = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; d < a.n_docs; d += (int64_t)gridDim.x * blockDim.x) {
        unsigned long long* row = a.stats + d * MA_COLS;
        row[MA_OUT_BYTES] = (unsigned long long)(a.doc_off[d + 1] - a.doc_off[d]) - row[MA_BYTES_OUT_OF] + row[MA_BYTES_IN];
#pragma unroll
        for (int c = 0; c < MA_COLS; ++c) v[c] += (long long)row[c];
    }
    if (!a.totals) return;
#pragma unroll
    for (int c = 0; c < MA_COLS; ++c) {
        const long long r = block_sum(v[c], s_red);
        if (threadIdx.x == 0 && r) ma_add(a.totals + c, (unsigned long long)r);
    }
}

}  // namespace

hipError_t launch_mask(const MaArgs& a, hipStream_t stream, int phases) {
    hipError_t e;
    const unsigned tiles = rewrite_grid(a.n_bytes + 16, RW_TILE, RW_MAX_GRID);
    if (phases & RW_RUN_MEASURE) {
        if ((e = rewrite_launch(td_ma_docs, rewrite_grid(a.n_docs + 1, RW_THREADS, 4096), a, stream)) != hipSuccess) return e;
        if ((e = rewrite_launch(td_ma_reset, rewrite_grid(a.n_docs * MA_COLS + MA_COLS, RW_THREADS, 4096), a, stream)) != hipSuccess) return e;
        if ((e = rewrite_launch(td_ma_tiles<0>, tiles, a, stream)) != hipSuccess) return e;
        if ((e = rewrite_launch(td_ma_scan, 1, a, stream)) != hipSuccess) return e;
        if ((e = rewrite_launch(td_ma_sums, rewrite_grid(a.n_docs, RW_THREADS, 1024), a, stream)) != hipSuccess) return e;
    }
    return phases & RW_RUN_WRITE ? rewrite_launch(td_ma_tiles<1>, tiles, a, stream) : hipGetLastError();
}

}  // namespace td
