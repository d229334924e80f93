// Training rows (td_make_rows*, td_encode_batch_rows): ids + per-document token offsets -> rows of S slots.
//
// CONCAT places document d's slots at base_d = tok_off[d] + d * (b + e), a closed form, so the rows need no scan: the slot
// kernel owns contiguous tiles of OUTPUT slots, finds the tile's first document by group_last_le over base_d and keeps the
// bases of the documents that overlap the tile in LDS (tile_table, td_rows_common.h; more than fit: every slot searches global
// memory, last_le_global).  PAD places
// slot j in document j / S.  Either way the ids are read at a per-document shift, as four dwords (or two aligned int4 and a
// funnel, funnel_src), and written as int4: nearly a copy.  A one-id document costs what its slots cost, and a PAD row of a
// truncated giant document reads S ids of it, not its body.
//
// cu_seqlens (CONCAT, requested): document d contributes c_d = [its start] + [the row starts strictly inside it], clamped to
// R; an exclusive scan of c_d places its entries.  One pass: chunks of documents take tickets in launch order, publish their
// total, look back over their predecessors' 64 at a time (decoupled look-back; a predecessor that has not published in time is
// summed by the waiting lane itself, so the spin is bounded and the result does not depend on scheduling), and write their entries
// load-balanced across the workgroup, so a document with many rows inside it is written by all lanes.
//
//   td_rows_concat / td_rows_pad   slots, positions, lengths, counts; <RowsLabArgs>: the label stream lab.src -> lab.dst beside
//                                  the ids (td_rows_common.h), <RowsArgs>: one stream, what the kernels were before the pair form
//   td_rows_cu                     cu_seqlens
#include <hip/hip_runtime.h>

#include "td_rows.h"
#include "td_rows_common.h"

namespace td {

namespace {

constexpr unsigned long long RS_AGG = 1ull << 62, RS_PRE = 2ull << 62, RS_VAL = (1ull << 62) - 1;
constexpr int ROWS_SPIN = 1 << 14;  // polls of a predecessor's status before the waiting wave sums that chunk itself
constexpr int ROWS_THREADS = RC_THREADS, ROWS_TILE = RC_TILE, ROWS_MAX_GRID = RC_MAX_GRID;

struct Plan {
    int64_t rows, total, R;  // rows, slots written (rows * S), real slots (CONCAT)
    bool ok;
};

// Every workgroup reads tok_off[n_docs] itself: the capacity check needs no launch of its own.  An error writes nothing.
__device__ Plan rows_plan(const RowsArgs& a, bool report) {
    Plan p{0, 0, 0, false};
    const int64_t ntok = a.tok_off[a.n_docs];
    if (ntok < 0 || ntok > a.n_tokens) {
        if (report) rows_raise(a, TD_E_INVALID, ntok);
        return p;
    }
    const int64_t k = a.b + a.e;
    if (a.layout == TD_ROWS_CONCAT) {
        const int64_t T = ntok + a.n_docs * k;
        p.rows = a.drop_last ? T / a.S : (T + a.S - 1) / a.S;
        p.R = T < p.rows * a.S ? T : p.rows * a.S;
    } else {
        p.rows = a.n_docs;
    }
    p.total = p.rows * a.S;
    if (p.rows > a.rows_cap) {
        if (report) {
            rows_raise(a, TD_E_CAPACITY, p.rows);
            a.counts[0] = p.rows;
        }
        return p;
    }
    p.ok = true;
    return p;
}

__device__ __forceinline__ int64_t doc_base(const RowsArgs& a, int64_t d, int64_t k) { return a.tok_off[d] + d * k; }

// ids[src .. src + 3] (L: lab.src[src .. src + 3]; the funnel is chosen per stream), 0 <= src and src + 4 <= n_tokens
template <bool L, class A>
__device__ __forceinline__ int4 rows_load4(const A& a, int64_t src) {
    const int32_t* p;
    if constexpr (L) p = a.lab.src;
    else p = a.ids;
    if (a.funnel_src && (((uintptr_t)p) & 15) == 0) {
        const int64_t al = src & ~(int64_t)3;
        const int sh = (int)(src & 3);
        const int4 q0 = *reinterpret_cast<const int4*>(p + al);
        if (sh == 0) return q0;
        if (al + 8 <= a.n_tokens) {  // (the second block may not lie behind the buffer)
            const int4 q1 = *reinterpret_cast<const int4*>(p + al + 4);
            if (sh == 1) return make_int4(q0.y, q0.z, q0.w, q1.x);
            if (sh == 2) return make_int4(q0.z, q0.w, q1.x, q1.y);
            return make_int4(q0.w, q1.x, q1.y, q1.z);
        }
    }
    return make_int4(p[src], p[src + 1], p[src + 2], p[src + 3]);
}

template <class A>
__global__ __launch_bounds__(ROWS_THREADS) void td_rows_concat(const A a) {
    constexpr bool LAB = has_lab<A>;
    __shared__ int32_t s_lb[RC_LDS_DOCS];  // bases of the tile's documents - s0, clamped to [-1, ROWS_TILE + 1]
    __shared__ long long s_red[ROWS_THREADS / 64];
    const int tid = threadIdx.x;
    const Plan p = rows_plan(a, blockIdx.x == 0 && tid == 0);
    if (!p.ok) return;
    const int64_t k = a.b + a.e, S = a.S, R = p.R;
    const int64_t ntiles = (p.total + ROWS_TILE - 1) / ROWS_TILE;
    const auto base_of = [off = a.tok_off, k](int64_t d) { return off[d] + d * k; };  // doc_base
    long long segs = 0;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t s0 = tile * ROWS_TILE;
        const int64_t s1 = s0 + ROWS_TILE < p.total ? s0 + ROWS_TILE : p.total;
        const int64_t r1 = s1 < R ? s1 : R;  // real slots of the tile end here
        __syncthreads();  // (the previous tile's readers of s_lb are done)
        int64_t d0 = 0, base0 = 0;
        int nl = 0;  // documents that overlap [s0, r1): s_lb[0, nl), and s_lb[nl] the base of the next
        bool over = false;
        if (s0 < r1) {
            d0 = group_last_le(base_of, 0, a.n_docs, s0);  // (base_0 = 0 <= s0)
            base0 = doc_base(a, d0, k);
            bool fits;
            nl = tile_table(s_lb, base_of, d0, a.n_docs, s0, -1, ROWS_TILE + 1, (int32_t)(r1 - s0), fits);
            over = !fits;
            // segments: the row starts in [s0, r1), and the starts of non-empty documents there that are not row starts
            {  // (lane 0 counts the row starts; in vector registers, the scalar ones are taken by the tile's bounds)
                const int64_t x0 = tid == 0 ? s0 + S - 1 : 0, x1 = tid == 0 ? r1 + S - 1 : 0;
                segs += div_magic(x1, a.S, a.s_magic) - div_magic(x0, a.S, a.s_magic);
            }
            if (!over) {
                for (int i = tid; i < nl; i += ROWS_THREADS) {
                    const int32_t r = s_lb[i];
                    if (r >= 0 && s_lb[i + 1] > r && s0 + r != div_magic(s0 + r, a.S, a.s_magic) * S) ++segs;
                }
            } else {
                for (int64_t c0 = 0;; c0 += ROWS_THREADS) {
                    const int64_t d = d0 + c0 + tid;
                    bool in = false;
                    if (d < a.n_docs) {
                        const int64_t bs = doc_base(a, d, k);
                        in = bs < r1;
                        if (in && bs >= s0 && doc_base(a, d + 1, k) > bs && bs != div_magic(bs, a.S, a.s_magic) * S) ++segs;
                    }
                    if (__syncthreads_count(in) < ROWS_THREADS) break;
                }
            }
        }
        for (int it = 0; it < ROWS_TILE / (4 * ROWS_THREADS); ++it) {
            const int64_t j0 = s0 + (int64_t)it * 4 * ROWS_THREADS + 4 * tid;
            if (j0 >= s1) break;
            int i = -1;               // the current document: d, [base, end) (end clamped to s0 + ROWS_TILE + 1 in LDS)
            int64_t d = -1, base = 0, end = 0;
            auto seek = [&](int64_t j) {  // j < r1
                if (!over) {
                    const int32_t x = (int32_t)(j - s0);
                    if (i < 0) i = last_le(s_lb, nl, x);
                    while (i + 1 < nl && s_lb[i + 1] <= x) ++i;
                    d = d0 + i;
                    base = i == 0 ? base0 : s0 + s_lb[i];
                    end = s0 + s_lb[i + 1];
                } else if (d < 0 || j >= end) {
                    d = last_le_global(base_of, d < 0 ? d0 : d, a.n_docs, j);
                    base = doc_base(a, d, k);
                    end = doc_base(a, d + 1, k);
                }
            };
            int32_t v[4], ps[4];
            [[maybe_unused]] int32_t lv[4];
            bool fast = false;
            if (j0 + 4 <= r1) {
                seek(j0);
                const int64_t src = j0 - d * k - a.b;
                if (j0 - base >= a.b && j0 + 3 < end - a.e && src >= 0 && src + 4 <= a.n_tokens) {
                    const int4 q = rows_load4<false>(a, src);
                    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
                    if constexpr (LAB) {
                        const int4 l = rows_load4<true>(a, src);
                        lv[0] = l.x; lv[1] = l.y; lv[2] = l.z; lv[3] = l.w;
                    }
                    fast = true;
                }
            }
            int64_t rs = div_magic(j0, a.S, a.s_magic) * S;  // row start
            for (int q = 0; q < 4; ++q) {
                const int64_t j = j0 + q;
                while (j >= rs + S) rs += S;
                if (j >= r1) {
                    v[q] = a.pad;
                    if constexpr (LAB) lv[q] = a.lab.pad;
                    ps[q] = 0;
                    continue;
                }
                seek(j);
                if (!fast) {
                    if constexpr (LAB) {
                        if (a.b && j == base) { v[q] = a.bos; lv[q] = a.lab.bos; }
                        else if (a.e && j == end - 1) { v[q] = a.eos; lv[q] = a.lab.eos; }
                        else v[q] = rows_load1_pair(a, j - d * k - a.b, lv[q]);
                    } else {
                        if (a.b && j == base) v[q] = a.bos;
                        else if (a.e && j == end - 1) v[q] = a.eos;
                        else v[q] = rows_load1(a, j - d * k - a.b);
                    }
                }
                ps[q] = (int32_t)(j - (base > rs ? base : rs));
            }
            rows_put4(a.out, j0, s1, v);
            lab_put4(a, j0, s1, lv);
            if (a.pos) rows_put4(a.pos, j0, s1, ps);
        }
    }
    const long long tot = block_sum(segs, s_red);
    if (tid == 0) {
        if (tot) atomicAdd(reinterpret_cast<unsigned long long*>(&a.counts[2]), (unsigned long long)tot);
        if (blockIdx.x == 0) {
            a.counts[0] = p.rows;
            a.counts[1] = R;
        }
    }
}

template <class A>
__global__ __launch_bounds__(ROWS_THREADS) void td_rows_pad(const A a) {
    constexpr bool LAB = has_lab<A>;
    __shared__ long long s_red[ROWS_THREADS / 64];
    const int tid = threadIdx.x;
    const Plan p = rows_plan(a, blockIdx.x == 0 && tid == 0);
    if (!p.ok) return;
    const int64_t k = a.b + a.e, S = a.S, room = S - k;
    const int64_t ntiles = (p.total + ROWS_TILE - 1) / ROWS_TILE;
    long long real = 0, segs = 0, trunc = 0;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t s0 = tile * ROWS_TILE;
        const int64_t s1 = s0 + ROWS_TILE < p.total ? s0 + ROWS_TILE : p.total;
        for (int it = 0; it < ROWS_TILE / (4 * ROWS_THREADS); ++it) {
            const int64_t j0 = s0 + (int64_t)it * 4 * ROWS_THREADS + 4 * tid;
            if (j0 >= s1) break;
            int64_t d = div_magic(j0, a.S, a.s_magic), o = j0 - d * S, lo = 0, L = 0, body = 0, len = 0;
            auto load_doc = [&] {
                lo = a.tok_off[d];
                L = a.tok_off[d + 1] - lo;
                body = L < 0 ? 0 : L < room ? L : room;
                len = a.b + body + a.e;
            };
            load_doc();
            int32_t v[4], ps[4];
            [[maybe_unused]] int32_t lv[4];
            bool fast = false;
            const int64_t src = lo + o - a.b;
            if (o + 4 <= S && j0 + 4 <= s1 && o >= a.b && o + 4 <= a.b + body && src >= 0 && src + 4 <= a.n_tokens) {
                const int4 q = rows_load4<false>(a, src);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
                if constexpr (LAB) {
                    const int4 l = rows_load4<true>(a, src);
                    lv[0] = l.x; lv[1] = l.y; lv[2] = l.z; lv[3] = l.w;
                }
                fast = true;
            }
            for (int q = 0; q < 4; ++q) {
                if (j0 + q >= s1) break;
                if (q > 0 && ++o == S) {
                    o = 0;
                    ++d;
                    load_doc();
                }
                if (!fast) {
                    if constexpr (LAB) {
                        if (o < a.b) { v[q] = a.bos; lv[q] = a.lab.bos; }
                        else if (o < a.b + body) v[q] = rows_load1_pair(a, lo + o - a.b, lv[q]);
                        else if (a.e && o == a.b + body) { v[q] = a.eos; lv[q] = a.lab.eos; }
                        else { v[q] = a.pad; lv[q] = a.lab.pad; }
                    } else {
                        if (o < a.b) v[q] = a.bos;
                        else if (o < a.b + body) v[q] = rows_load1(a, lo + o - a.b);
                        else if (a.e && o == a.b + body) v[q] = a.eos;
                        else v[q] = a.pad;
                    }
                }
                ps[q] = o < len ? (int32_t)o : 0;
                if (o == 0) {
                    if (a.aux) a.aux[d] = (int32_t)len;
                    real += len;
                    segs += len > 0;
                    trunc += L > room;
                }
            }
            rows_put4(a.out, j0, s1, v);
            lab_put4(a, j0, s1, lv);
            if (a.pos) rows_put4(a.pos, j0, s1, ps);
        }
    }
    const long long r = block_sum(real, s_red), s = block_sum(segs, s_red), t = block_sum(trunc, s_red);
    if (tid == 0) {
        if (r) atomicAdd(reinterpret_cast<unsigned long long*>(&a.counts[1]), (unsigned long long)r);
        if (s) atomicAdd(reinterpret_cast<unsigned long long*>(&a.counts[2]), (unsigned long long)s);
        if (t) atomicAdd(reinterpret_cast<unsigned long long*>(&a.counts[3]), (unsigned long long)t);
        if (blockIdx.x == 0) a.counts[0] = p.rows;
    }
}

// c_d: the document's start and the row starts strictly inside it, below R
__device__ __forceinline__ long long doc_cuts(const RowsArgs& a, int64_t d, int64_t k, int64_t R, int64_t& base) {
    base = doc_base(a, d, k);
    const int64_t n = a.tok_off[d + 1] - a.tok_off[d] + k;
    if (n <= 0 || base >= R) return 0;
    const int64_t end = base + n < R ? base + n : R;
    return 1 + div_magic(end - 1, a.S, a.s_magic) - div_magic(base, a.S, a.s_magic);
}

__device__ __forceinline__ unsigned long long wave_u64(unsigned long long w) {  // (the same word in every lane: wave-uniform branches)
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)w), hi = __builtin_amdgcn_readfirstlane((uint32_t)(w >> 32));
    return (unsigned long long)hi << 32 | lo;
}

__global__ __launch_bounds__(ROWS_THREADS) void td_rows_cu(const RowsArgs a) {
    __shared__ long long s_w[RC_SCAN_CHUNK + 1];  // the chunk's exclusive scan of c_d, then its total
    __shared__ long long s_base[RC_SCAN_CHUNK];
    __shared__ long long s_wave[ROWS_THREADS / 64];
    __shared__ long long s_excl;
    __shared__ unsigned long long s_chunk;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const Plan p = rows_plan(a, false);
    if (!p.ok) return;
    if (tid == 0) s_chunk = atomicAdd(&a.scan[0], 1ull);  // (tickets in launch order: every predecessor has started)
    __syncthreads();
    const int64_t c = (int64_t)s_chunk;
    const int64_t nch = a.n_docs > 0 ? (a.n_docs + RC_SCAN_CHUNK - 1) / RC_SCAN_CHUNK : 1;
    const int64_t k = a.b + a.e, R = p.R;
    long long v[4], sum = 0;
    for (int q = 0; q < 4; ++q) {
        const int64_t d = c * RC_SCAN_CHUNK + tid * 4 + q;
        int64_t base = 0;
        v[q] = d < a.n_docs ? doc_cuts(a, d, k, R, base) : 0;
        s_base[tid * 4 + q] = base;
        sum += v[q];
    }
    const long long incl = wave_incl_scan(sum, lane, [](long long x, long long y) { return x + y; });
    if (lane == 63) s_wave[wv] = incl;
    __syncthreads();
    long long before = 0, agg = 0;
    for (int w = 0; w < ROWS_THREADS / 64; ++w) {
        if (w < wv) before += s_wave[w];
        agg += s_wave[w];
    }
    long long run = before + incl - sum;
    for (int q = 0; q < 4; ++q) {
        s_w[tid * 4 + q] = run;
        run += v[q];
    }
    if (tid == 0) s_w[RC_SCAN_CHUNK] = agg;
    if (wv == 0) {  // look back 64 predecessors at a time: lane i reads chunk top - i
        unsigned long long* st = a.scan + 1;
        long long pre = 0;
        if (c > 0) {
            if (lane == 0) __hip_atomic_store(&st[c], RS_AGG | (unsigned long long)agg, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            for (int64_t top = c - 1;; top -= 64) {
                const int64_t q = top - lane;
                unsigned long long w = RS_PRE;  // (in front of chunk 0: an inclusive prefix of 0)
                if (q >= 0) {
                    w = 0;
                    for (int spin = 0; spin < ROWS_SPIN && (w >> 62) == 0; ++spin) {
                        w = __hip_atomic_load(&st[q], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
                        if ((w >> 62) == 0) __builtin_amdgcn_s_sleep(1);
                    }
                    if ((w >> 62) == 0) {  // not published in time: this lane sums chunk q itself
                        long long part = 0;
                        for (int r = 0; r < RC_SCAN_CHUNK; ++r) {
                            const int64_t d = q * RC_SCAN_CHUNK + r;
                            int64_t base;
                            if (d < a.n_docs) part += doc_cuts(a, d, k, R, base);
                        }
                        w = RS_AGG | (unsigned long long)part;
                    }
                }
                const unsigned long long prefix = __ballot((w >> 62) == 2);  // (the nearest inclusive prefix ends the walk)
                const int stop = prefix ? __ffsll((long long)prefix) - 1 : 63;
                long long part = lane <= stop ? (long long)(w & RS_VAL) : 0;
                for (int dd = 32; dd >= 1; dd >>= 1) part += __shfl_xor(part, dd);
                pre += part;
                if (prefix) break;
            }
        }
        if (lane == 0) {
            __hip_atomic_store(&st[c], RS_PRE | (unsigned long long)(pre + agg), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            s_excl = pre;
        }
    }
    __syncthreads();
    const long long ex = s_excl;
    for (long long q = tid; q < agg; q += ROWS_THREADS) {  // entry q of the chunk: in the last document whose scan is <= q
        const int lo = last_le(s_w, RC_SCAN_CHUNK, q);
        const long long m = q - s_w[lo], base = s_base[lo];
        const long long val = m == 0 ? base : (div_magic(base, a.S, a.s_magic) + m) * a.S;
        if (ex + q < a.aux_cap) a.aux[ex + q] = (int32_t)val;
        else rows_raise(a, TD_E_INVALID, ex + q);
    }
    if (c == nch - 1 && tid == 0) {
        if (ex + agg < a.aux_cap) a.aux[ex + agg] = (int32_t)R;
        else rows_raise(a, TD_E_INVALID, ex + agg);
    }
}

}  // namespace

int64_t rows_scan_words(int64_t n_docs) { return 1 + (n_docs > 0 ? (n_docs + RC_SCAN_CHUNK - 1) / RC_SCAN_CHUNK : 1); }

hipError_t launch_rows(const RowsLabArgs& a, hipStream_t stream) {
    const int64_t tiles = (a.rows_cap * a.S + ROWS_TILE - 1) / ROWS_TILE;  // (the host keeps rows_cap * S far from overflow)
    const int grid = (int)(tiles < 1 ? 1 : tiles < ROWS_MAX_GRID ? tiles : ROWS_MAX_GRID);
    const RowsArgs& one = a;
    if (a.lab.src) {  // the pair form: ids and labels by one resolution of every slot
        if (a.layout == TD_ROWS_PAD) hipLaunchKernelGGL(td_rows_pad<RowsLabArgs>, dim3(grid), dim3(ROWS_THREADS), 0, stream, a);
        else hipLaunchKernelGGL(td_rows_concat<RowsLabArgs>, dim3(grid), dim3(ROWS_THREADS), 0, stream, a);
    } else {
        if (a.layout == TD_ROWS_PAD) hipLaunchKernelGGL(td_rows_pad<RowsArgs>, dim3(grid), dim3(ROWS_THREADS), 0, stream, one);
        else hipLaunchKernelGGL(td_rows_concat<RowsArgs>, dim3(grid), dim3(ROWS_THREADS), 0, stream, one);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (a.layout == TD_ROWS_CONCAT && a.aux) {
        hipLaunchKernelGGL(td_rows_cu, dim3((unsigned)(rows_scan_words(a.n_docs) - 1)), dim3(ROWS_THREADS), 0, stream, one);
        e = hipGetLastError();
    }
    return e;
}

}  // namespace td
