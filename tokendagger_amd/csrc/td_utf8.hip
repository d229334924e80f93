// UTF-8 validation and repair (td_utf8_check_device, td_utf8_device and what ends in them): text + document offsets -> flags[d] (0:
// well-formed), first_bad[d], n_bad[d], and the repaired text + its document offsets.  The rule is the contract in
// include/tokendagger_hip.h; td_utf8_args.h has the unit rule, the window screen and the lane walk, which the host statement
// (td_utf8_host) and the CPU model compile too.  No table: everything is compares on bytes.
//
// The text is cut into WINDOWS of 16 bytes at 16-byte aligned ADDRESSES (the base pointer need not be aligned: the first window is short),
// a lane a window, 256 windows a tile.  Two facts keep the documents off the fast path:
//   - a unit is fixed by three bytes in front of it and three behind it, so a unit at least three bytes away from both ends of its
//     document is what it would be were the whole text one document;
//   - the window screen (u8_window_suspect: SWAR over the window's four dwords, the dword in front and the dword behind, in registers)
//     is never set on well-formed text and always set where a byte of the window belongs to an ill-formed subpart of the text.
// So a lane a document looks at its document's first byte and at the byte behind its last: only where one of them is a continuation
// byte can the document's rule differ from the text's, and then the units within three bytes of the document's ends are taken by the
// document's rule (at most six).  A window finds its documents only when the screen is set.  A window with no byte >= 0x80 is skipped
// after four ORs.
//
//   td_utf8_docs     a lane a document: the offsets checks.  The lowest bad document is kept in head; every later kernel returns when
//                    there is one, the next one raises it: nothing is written then.
//   td_utf8_prepare  a lane a document: flags 0, first_bad -1, n_bad 0, counts 0, then the document's edges.  The check reports them at
//                    once (flags, first_bad: its own document's entries); the repair marks the windows that hold their bytes in `dirty`.
//   td_utf8_check    grid-stride over windows, four loads in flight a lane; a window the screen sets is walked by the document's rule
//                    (its documents by bisection): flags (a store) and first_bad (a minimum) are idempotent, so both paths may report.
//   td_utf8_tiles<0> MEASURE: a lane has the BYTES of its window: a byte of a well-formed unit is a byte of output, the first byte of a
//                    subpart three bytes or none.  A window that is neither suspect nor dirty is a copy and is not walked.  flags,
//                    first_bad, n_bad, counts[2] and counts[3] are made here alone, by the lane that has the subpart's first byte.
//   td_utf8_scan     one workgroup: tile_base to its exclusive prefixes, counts[0], TD_E_CAPACITY, the offsets of the documents that start
//                    at the text's end.
//   td_utf8_tiles<1> WRITE: sizes once more, a workgroup scan places the lanes, then they write: a tile of copied windows is one
//                    cooperative copy with 16-byte stores, any other tile is written lane by lane.  A document's output offset is written
//                    by the lane that has its first byte.
//   td_utf8_sums     a lane a document: counts[1] from flags; for the repair counts[4] and counts[5] from the documents' first and last units
// Nothing outside text[0, doc_off[n_docs]) and doc_off[0, n_docs] is read, nothing outside the outputs is written.  Sums, minima and
// stores of 1 only: the results do not depend on the order of the lanes.
#include <hip/hip_runtime.h>

#include "td_rows_common.h"
#include "td_utf8.h"

namespace td {

namespace {

static_assert(U8_THREADS == RC_THREADS && U8_TILE == RC_TILE, "the row kernels' launch shape");
constexpr int U8_MAX_GRID = 1 << 20;
constexpr int32_t U8_OFF_LO = -8, U8_OFF_HI = U8_TILE + 8;
constexpr long long U8_BAD_TOP = 1ll << 62;

struct U8Add {
    __device__ __forceinline__ void operator()(unsigned long long* p, unsigned long long n) const {
        __hip_atomic_fetch_add(p, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};
struct U8Lower {
    __device__ __forceinline__ void operator()(unsigned long long* p, unsigned long long v) const {
        __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

__device__ __forceinline__ bool u8_ascii(uint4 v) { return ((v.x | v.y | v.z | v.w) & U8_H) == 0; }

// the screen of the window v at text + b, which has four bytes of the text in front of it and four behind it
__device__ __forceinline__ bool u8_suspect_at(const uint8_t* text, int64_t b, uint4 v) {
    const uint32_t s[6] = {*reinterpret_cast<const uint32_t*>(text + b - 4), v.x, v.y, v.z, v.w, *reinterpret_cast<const uint32_t*>(text + b + 16)};
    return u8_window_suspect(s);
}

__global__ __launch_bounds__(U8_THREADS) void td_utf8_docs(const U8Args a) {
    const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (gid == 0 && a.doc_off[0] != 0) atomicMax(&a.head[U8_H_BAD], (unsigned long long)U8_BAD_TOP);
    for (int64_t d = gid; d < a.n_docs; d += (int64_t)gridDim.x * blockDim.x) {
        const int64_t lo = a.doc_off[d], hi = a.doc_off[d + 1];
        if (lo < 0 || hi < lo || hi > a.n_bytes) atomicMax(&a.head[U8_H_BAD], (unsigned long long)(U8_BAD_TOP - d));
    }
}

__global__ __launch_bounds__(U8_THREADS) void td_utf8_prepare(const U8Args a) {
    if (a.head[U8_H_BAD]) return;
    const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    const int shift = (int)(((uintptr_t)a.text) & 15);
    const int64_t total = a.doc_off[a.n_docs];
    if (gid < U8_C_WORDS) a.counts[gid] = 0;
    for (int64_t d = gid; d < a.n_docs; d += step) {
        const int64_t ds = a.doc_off[d], de = a.doc_off[d + 1];
        unsigned long long first = ~0ull;
        bool ill = false;
        u8_doc_edges(a.text, ds, de, total, [&](int64_t p, int len) {
            if (a.dirty) {  // (the repair: the measure pass reports, each subpart by the one lane that has its first byte)
                a.dirty[u8_window_of(p, shift)] = 1;
                a.dirty[u8_window_of(p + len - 1, shift)] = 1;
            } else {
                ill = true;
                first = first < (unsigned long long)(p - ds) ? first : (unsigned long long)(p - ds);
            }
        });
        a.flags[d] = ill;
        if (a.first_bad) a.first_bad[d] = first;
        if (a.n_bad) a.n_bad[d] = 0;
    }
}

// (shared by the kernels that come first behind td_utf8_prepare in a call)
__device__ __forceinline__ bool u8_bad_offsets(const U8Args& a, bool raise) {
    const unsigned long long bad = a.head[U8_H_BAD];
    if (!bad) return false;
    if (raise && blockIdx.x == 0 && threadIdx.x == 0) rows_raise(a, TD_E_INVALID, (int64_t)(U8_BAD_TOP - (long long)bad));
    return true;
}

// ---- the check ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(U8_THREADS) void td_utf8_check(const U8Args a) {
    if (u8_bad_offsets(a, true)) return;
    const int64_t total = a.doc_off[a.n_docs];
    const int shift = (int)(((uintptr_t)a.text) & 15);
    const int64_t nwin = u8_windows(total, shift), step = (int64_t)gridDim.x * blockDim.x;
    int64_t D = -1, ds = 0, de = 0;
    const auto slow = [&](int64_t g) {
        const int64_t b = g * 16 - shift;
        u8_check_window(a, b < 0 ? 0 : b, b + 16 < total ? b + 16 : total, D, ds, de,
                        [&](int64_t p) { return last_le_global([off = a.doc_off](int64_t d) { return off[d]; }, 0, a.n_docs, p); }, U8Lower{});
    };
    int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    // four windows a step while all four have four bytes of the text in front of them and four behind them
    for (; g * 16 - shift >= 4 && (g + 3 * step) * 16 - shift + 20 <= total; g += 4 * step) {
        uint4 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = *reinterpret_cast<const uint4*>(a.text + ((g + q * step) * 16 - shift));
        if (((v[0].x | v[0].y | v[0].z | v[0].w | v[1].x | v[1].y | v[1].z | v[1].w | v[2].x | v[2].y | v[2].z | v[2].w | v[3].x | v[3].y | v[3].z |
              v[3].w) & U8_H) == 0)
            continue;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (!u8_ascii(v[q]) && u8_suspect_at(a.text, (g + q * step) * 16 - shift, v[q])) slow(g + q * step);
    }
    for (; g < nwin; g += step) {
        const int64_t b = g * 16 - shift;
        if (b >= 4 && b + 20 <= total) {
            const uint4 v = *reinterpret_cast<const uint4*>(a.text + b);
            if (u8_ascii(v) || !u8_suspect_at(a.text, b, v)) continue;
        }
        slow(g);
    }
}

__global__ __launch_bounds__(U8_THREADS) void td_utf8_sums(const U8Args a) {
    __shared__ long long s_red[U8_THREADS / 64];
    if (a.head[U8_H_BAD]) return;
    const bool repair = a.dirty != nullptr;
    long long ill = 0, begins = 0, ends = 0;
    for (int64_t d = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; d < a.n_docs; d += (int64_t)gridDim.x * blockDim.x) {
        ill += a.flags[d] != 0;
        const int64_t ds = a.doc_off[d], de = a.doc_off[d + 1];
        if (repair && ds < de) {
            begins += u8_is_cont(a.text[ds]);
            ends += u8_ends_cut(a.text, ds, de);
        }
    }
    ill = block_sum(ill, s_red);
    begins = block_sum(begins, s_red);
    ends = block_sum(ends, s_red);
    if (threadIdx.x == 0) {
        if (ill) U8Add{}(a.counts + U8_C_DOCS, (unsigned long long)ill);
        if (begins) U8Add{}(a.counts + U8_C_BEGIN_CONT, (unsigned long long)begins);
        if (ends) U8Add{}(a.counts + U8_C_END_LEAD, (unsigned long long)ends);
    }
}

// ---- the repair -----------------------------------------------------------------------------------------------------------------------
// dst[0, len) = src[0, len) by the whole workgroup: 16-byte stores at 16-byte aligned addresses of dst, the source as it lies
__device__ __forceinline__ void u8_group_copy(uint8_t* dst, const uint8_t* src, int64_t len) {
    const int tid = threadIdx.x;
    int64_t head = (int64_t)((16 - (((uintptr_t)dst) & 15)) & 15);
    head = head < len ? head : len;
    const int64_t n16 = (len - head) >> 4;
    if (tid < head) dst[tid] = src[tid];
    for (int64_t k = tid; k < n16; k += U8_THREADS) {
        uint4 v;
        __builtin_memcpy(&v, src + head + 16 * k, 16);
        *reinterpret_cast<uint4*>(dst + head + 16 * k) = v;
    }
    const int64_t tail = head + 16 * n16;
    if (tail + tid < len) dst[tail + tid] = src[tail + tid];
}

template <int WRITE>
__global__ __launch_bounds__(U8_THREADS) void td_utf8_tiles(const U8Args a) {
    __shared__ int32_t s_off[RC_LDS_DOCS];  // doc_off[kb + i] - t0, clamped to [U8_OFF_LO, U8_OFF_HI]
    __shared__ long long s_red[U8_THREADS / 64];
    const int tid = threadIdx.x;
    if (u8_bad_offsets(a, !WRITE)) return;
    if (WRITE && a.head[U8_H_FULL]) return;
    const int64_t total = a.doc_off[a.n_docs];
    const int shift = (int)(((uintptr_t)a.text) & 15);
    const int64_t ntiles = total > 0 ? (total + shift + U8_TILE - 1) / U8_TILE : 0;
    const auto off_of = [off = a.doc_off](int64_t d) { return off[d]; };
    U8LaneStats st = {0, 0};
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t t0 = t * U8_TILE - shift < 0 ? 0 : t * U8_TILE - shift;
        const int64_t s1 = (t + 1) * U8_TILE - shift < total ? (t + 1) * U8_TILE - shift : total;
        const int64_t b0 = t * U8_TILE + 16 * tid - shift, b = b0 < 0 ? 0 : b0, we = b0 + 16 < total ? b0 + 16 : total;
        const bool owns = b < we;
        // a window none of whose bytes belongs to an ill-formed subpart: a copy.  Windows at the text's ends are walked.
        bool fast = !owns;
        if (owns && b0 >= 4 && b0 + 20 <= total) {
            const uint4 v = *reinterpret_cast<const uint4*>(a.text + b);
            fast = u8_ascii(v) || (!u8_suspect_at(a.text, b, v) && !a.dirty[t * U8_THREADS + tid]);
        }
        // the tile's documents: kb the last that starts in front of t0 (t0 == 0: the first), its table, where a lane needs one
        const bool need = WRITE || !fast;
        int64_t kb = 0, nk = 0;
        bool lds = true;
        __syncthreads();  // (the tile before has read its table)
        if (__syncthreads_or(need)) {
            kb = t0 > 0 ? group_last_le(off_of, 0, a.n_docs, t0 - 1) : 0;
            nk = tile_table(s_off, off_of, kb, a.n_docs, t0, U8_OFF_LO, U8_OFF_HI, (int32_t)(s1 - t0), lds);
            if (!lds) nk = group_last_le(off_of, kb, a.n_docs, s1 - 1) - kb + 1;
            __syncthreads();
        }
        // ub(x), t0 - 1 <= x < s1: kb + the first entry of [0, nk] behind x (entry nk is at or behind s1)
        const auto ub_of = [&](auto rel) {
            return [=](int64_t x) {
                int64_t lo = 0, hi = nk;  // the answer lies in [lo, hi]
                const int64_t r = x - t0;
                while (lo < hi) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (rel(mid) > r) hi = mid;
                    else lo = mid + 1;
                }
                return kb + lo;
            };
        };
        const auto rel_lds = [&](int64_t i) { return (int64_t)s_off[i]; };
        const auto rel_glb = [&](int64_t i) { return a.doc_off[kb + i] - t0; };
        const auto lane = [&](auto mode, int64_t opos) {
            constexpr int MODE = decltype(mode)::value;
            if (!owns) return (int64_t)0;
            if (lds) return u8_lane<MODE>(a, b, we, ub_of(rel_lds), opos, st, U8Add{}, U8Lower{});
            return u8_lane<MODE>(a, b, we, ub_of(rel_glb), opos, st, U8Add{}, U8Lower{});
        };
        // a copied window: the output offsets of the documents that start in it
        const auto put_starts = [&](int64_t opos) {
            for (int64_t k = lds ? ub_of(rel_lds)(b - 1) : ub_of(rel_glb)(b - 1); k <= a.n_docs; ++k) {
                const int64_t s = a.doc_off[k];
                if (s >= we) break;
                a.out_doc_off[k] = opos + (s - b);
            }
        };
        if (!WRITE) {
            const int64_t n = !owns ? 0 : fast ? we - b : lane(std::integral_constant<int, U8_MEASURE>{}, 0);
            const long long sum = block_sum(n, s_red);
            if (tid == 0) a.tile_base[t] = (unsigned long long)sum;
        } else {
            const int64_t n = !owns ? 0 : fast ? we - b : lane(std::integral_constant<int, U8_SIZE>{}, 0);
            long long sum;
            const int64_t opos = (int64_t)a.tile_base[t] + block_excl(n, s_red, sum);
            if (__syncthreads_and(fast)) {
                u8_group_copy(a.out + a.tile_base[t], a.text + t0, s1 - t0);
                if (owns) put_starts(opos);
            } else if (fast && owns) {
                for (int64_t q = b; q < we; ++q) a.out[opos + (q - b)] = a.text[q];
                put_starts(opos);
            } else {
                lane(std::integral_constant<int, U8_WRITE>{}, opos);
            }
        }
    }
    if (!WRITE) {
        const long long sub = block_sum(st.subparts, s_red), byt = block_sum(st.sub_bytes, s_red);
        if (tid == 0) {
            if (sub) U8Add{}(a.counts + U8_C_SUBPARTS, (unsigned long long)sub);
            if (byt) U8Add{}(a.counts + U8_C_SUB_BYTES, (unsigned long long)byt);
        }
    }
}

__global__ __launch_bounds__(U8_THREADS) void td_utf8_scan(const U8Args a) {
    __shared__ long long s_wave[U8_THREADS / 64];
    if (a.head[U8_H_BAD]) return;
    const int64_t total = a.doc_off[a.n_docs];
    const int shift = (int)(((uintptr_t)a.text) & 15);
    const int64_t ntiles = total > 0 ? (total + shift + U8_TILE - 1) / U8_TILE : 0;
    long long carry[1];
    chunks_excl_scan<1>(a.tile_base, ntiles, s_wave, carry);
    const int64_t need = carry[0];
    if (threadIdx.x == 0) {
        a.counts[U8_C_BYTES] = (unsigned long long)need;
        if (need > a.out_capacity) {
            a.head[U8_H_FULL] = 1;
            rows_raise(a, TD_E_CAPACITY, need);
        }
    }
    if (need > a.out_capacity) return;
    // the documents that start at the text's end (the entry behind the last one among them): no window holds them
    for (int64_t d = a.n_docs - threadIdx.x; d >= 0 && a.doc_off[d] == total; d -= U8_THREADS) a.out_doc_off[d] = need;
}

unsigned u8_grid(int64_t n, int64_t per, int64_t most) {
    const int64_t g = (n + per - 1) / per;
    return (unsigned)(g < 1 ? 1 : g < most ? g : most);
}

}  // namespace

hipError_t launch_utf8_check(const U8Args& a, hipStream_t stream) {
    hipError_t e;
    hipLaunchKernelGGL(td_utf8_docs, dim3(u8_grid(a.n_docs + 1, U8_THREADS, 4096)), dim3(U8_THREADS), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(td_utf8_prepare, dim3(u8_grid(a.n_docs + U8_C_WORDS, U8_THREADS, 4096)), dim3(U8_THREADS), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // four windows a lane, and at most 2048 workgroups (eight a CU) that stride over the rest
    hipLaunchKernelGGL(td_utf8_check, dim3(u8_grid(a.n_bytes + 16, 4 * U8_TILE, 2048)), dim3(U8_THREADS), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(td_utf8_sums, dim3(u8_grid(a.n_docs, U8_THREADS, 4096)), dim3(U8_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_utf8(const U8Args& a, hipStream_t stream, int phases) {
    hipError_t e;
    const unsigned tiles = u8_grid(a.n_bytes + 16, U8_TILE, U8_MAX_GRID);
    if (phases & U8_RUN_MEASURE) {
        hipLaunchKernelGGL(td_utf8_docs, dim3(u8_grid(a.n_docs + 1, U8_THREADS, 4096)), dim3(U8_THREADS), 0, stream, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(td_utf8_prepare, dim3(u8_grid(a.n_docs + U8_C_WORDS, U8_THREADS, 4096)), dim3(U8_THREADS), 0, stream, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(td_utf8_tiles<0>, dim3(tiles), dim3(U8_THREADS), 0, stream, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(td_utf8_scan, dim3(1), dim3(U8_THREADS), 0, stream, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(td_utf8_sums, dim3(u8_grid(a.n_docs, U8_THREADS, 4096)), dim3(U8_THREADS), 0, stream, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (phases & U8_RUN_WRITE) hipLaunchKernelGGL(td_utf8_tiles<1>, dim3(tiles), dim3(U8_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace td
