// Unicode NFC normalisation (td_nfc_check_device, td_nfc_device and what ends in them): text + document offsets -> flags[d] (0: proven
// NFC) at read speed, and the normalised text + its document offsets.  The rule is the contract in include/tokendagger_hip.h;
// td_nfc_args.h has the lookup, the decoder, the quick check, the segment scan and the segment normaliser, which the host statement
// (td_nfc_host) and the CPU model compile too.  The tables (generated/unicode_nfc.inc, 55 KiB) are __device__ constants here: they are
// touched only behind a lead byte >= 0xCC and are left to L2, LDS holds none of them.
//
// The text is cut into WINDOWS of 16 bytes at 16-byte aligned ADDRESSES (the base pointer need not be aligned: the first window is short),
// a lane a window, 256 windows a tile.  A window inside the text is one 16-byte load; a window none of whose bytes reaches 0xCC holds
// boundaries only and is proven by four integer operations a dword.
//
//   td_nfc_docs     a lane a document: the offsets checks.  The lowest bad document is kept in head; every later kernel returns when there
//                   is one, the next one raises it: nothing is written then.
//   td_nfc_clear    flags, changed and counts to zero
//   td_nfc_check    grid-stride over windows, four loads in flight a lane.  A byte >= 0xCC is decoded inside its document (found by
//                   bisection); a code point that is not Quick_Check Yes, or a non-starter below the ccc of the unit in front
//                   of it (decoded backwards: a unit is fixed by three bytes of context, so lane, step and workgroup seams do not matter),
//                   flags its document.
//   td_nfc_tiles<0> MEASURE: a lane OWNS the segments that start in its window and walks each to its end, beyond the window too; a lane
//                   whose window holds no boundary owns nothing and looks no further than its window.  Proven segments count their
//                   length, the others go through the normaliser with a sink that only counts and compares.  A window of ASCII is not
//                   walked (sixteen segments of one code point); one of bytes below 0xCC is, for its opaque bytes.  The tile's bytes go to tile_base[t]; flags, changed and the counts are made here.
//   td_nfc_scan     one workgroup: tile_base to its exclusive prefixes, counts[0], TD_E_CAPACITY, the offsets of the documents that start
//                   at the text's end.
//   td_nfc_tiles<1> WRITE: the lanes measure once more (sizes only), a workgroup scan places them, then they write: a tile of proven
//                   windows is one cooperative copy with 16-byte stores, any other tile is written lane by lane.  A document's output offset
//                   is written by the lane that owns its first segment.
//   td_nfc_sums     a lane a document: counts[1] and counts[2] from flags and changed
// Measure and write are two walks, not one with staging in LDS: an output tile is up to three times its input, the proven case (all of
// real text but a few places) walks nothing twice but sixteen bytes' worth of compares, and nothing is carried from tile to tile.
//
// Nothing outside text[0, doc_off[n_docs]) and doc_off[0, n_docs] is read, nothing outside the outputs is written.
#include <hip/hip_runtime.h>

#include "td_nfc.h"
#include "td_rows_common.h"

namespace td {

namespace {

#define TD_NFC_TABLE(type, name, n) __device__ const type name[n]
#include "generated/unicode_nfc.inc"
#undef TD_NFC_TABLE

static_assert(NFC_THREADS == RC_THREADS && NFC_TILE == RC_TILE, "the row kernels' launch shape");
constexpr int NFC_MAX_GRID = 1 << 20;
constexpr int32_t NFC_OFF_LO = -8, NFC_OFF_HI = NFC_TILE + 8;
constexpr long long NFC_BAD_TOP = 1ll << 62;

__device__ __forceinline__ NfcTables nfc_tables() {
    return NfcTables{td_nfc_stage1, td_nfc_stage2, td_nfc_dec_key, td_nfc_dec_off, td_nfc_dec_cps, td_nfc_pair_a, td_nfc_pair_b, td_nfc_pair_c};
}

__device__ __forceinline__ void nfc_add(unsigned long long* p, unsigned long long n) {
    __hip_atomic_fetch_add(p, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the bytes of a dword at or above 0xCC, as their top bits
__device__ __forceinline__ uint32_t nfc_hits(uint32_t w) { return ((w & 0x7F7F7F7Fu) + 0x34343434u) & w & 0x80808080u; }
__device__ __forceinline__ uint32_t nfc_hits(uint4 v) { return nfc_hits(v.x) | nfc_hits(v.y) | nfc_hits(v.z) | nfc_hits(v.w); }

__global__ __launch_bounds__(NFC_THREADS) void td_nfc_docs(const NfcArgs a) {
    const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (gid == 0 && a.doc_off[0] != 0) atomicMax(&a.head[NFC_H_BAD], (unsigned long long)NFC_BAD_TOP);
    for (int64_t d = gid; d < a.n_docs; d += (int64_t)gridDim.x * blockDim.x) {
        const int64_t lo = a.doc_off[d], hi = a.doc_off[d + 1];
        if (lo < 0 || hi < lo || hi > a.n_bytes) atomicMax(&a.head[NFC_H_BAD], (unsigned long long)(NFC_BAD_TOP - d));
    }
}

__global__ __launch_bounds__(NFC_THREADS) void td_nfc_clear(const NfcArgs a) {
    if (a.head[NFC_H_BAD]) return;
    const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    if (gid < NFC_C_WORDS) a.counts[gid] = 0;
    for (int64_t d = gid; d < a.n_docs; d += step) {
        a.flags[d] = 0;
        if (a.changed) a.changed[d] = 0;
    }
}

// (shared by the kernels that come first behind td_nfc_docs in a call)
__device__ __forceinline__ bool nfc_bad_offsets(const NfcArgs& a, bool raise) {
    const unsigned long long bad = a.head[NFC_H_BAD];
    if (!bad) return false;
    if (raise && blockIdx.x == 0 && threadIdx.x == 0) rows_raise(a, TD_E_INVALID, (int64_t)(NFC_BAD_TOP - (long long)bad));
    return true;
}

// ---- the check ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NFC_THREADS) void td_nfc_check(const NfcArgs a) {
    if (nfc_bad_offsets(a, true)) return;
    const NfcTables T = nfc_tables();
    const int64_t total = a.doc_off[a.n_docs];
    const int shift = (int)(((uintptr_t)a.text) & 15);
    const int64_t nwin = (total + shift + 15) >> 4, step = (int64_t)gridDim.x * blockDim.x;
    int64_t D = -1, ds = 0, de = 0;
    const auto slow = [&](int64_t g) {
        const int64_t b = g * 16 - shift;
        nfc_check_window(a, T, b < 0 ? 0 : b, b + 16 < total ? b + 16 : total, D, ds, de,
                         [&](int64_t p) { return last_le_global([off = a.doc_off](int64_t d) { return off[d]; }, 0, a.n_docs, p); });
    };
    int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    // four windows a step while all four lie inside the text (g >= 1: the first window may begin in front of it)
    for (; g >= 1 && (g + 3 * step) * 16 - shift + 16 <= total; g += 4 * step) {
        uint4 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = *reinterpret_cast<const uint4*>(a.text + ((g + q * step) * 16 - shift));
        if ((nfc_hits(v[0]) | nfc_hits(v[1]) | nfc_hits(v[2]) | nfc_hits(v[3])) == 0) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (nfc_hits(v[q])) slow(g + q * step);
    }
    for (; g < nwin; g += step) {
        const int64_t b = g * 16 - shift;
        if (b >= 0 && b + 16 <= total && nfc_hits(*reinterpret_cast<const uint4*>(a.text + b)) == 0) continue;
        slow(g);
    }
}

__global__ __launch_bounds__(NFC_THREADS) void td_nfc_sums(const NfcArgs a) {
    __shared__ long long s_red[NFC_THREADS / 64];
    if (a.head[NFC_H_BAD]) return;
    long long unproven = 0, changed = 0;
    for (int64_t d = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; d < a.n_docs; d += (int64_t)gridDim.x * blockDim.x) {
        unproven += a.flags[d] != 0;
        if (a.changed) changed += a.changed[d] != 0;
    }
    unproven = block_sum(unproven, s_red);
    changed = block_sum(changed, s_red);
    if (threadIdx.x == 0) {
        if (unproven) nfc_add(a.counts + NFC_C_UNPROVEN, (unsigned long long)unproven);
        if (changed) nfc_add(a.counts + NFC_C_CHANGED, (unsigned long long)changed);
    }
}

// ---- the normaliser -------------------------------------------------------------------------------------------------------------------
// dst[0, len) = src[0, len) by the whole workgroup: 16-byte stores at 16-byte aligned addresses of dst, the source as it lies
__device__ __forceinline__ void nfc_group_copy(uint8_t* dst, const uint8_t* src, int64_t len) {
    const int tid = threadIdx.x;
    int64_t head = (int64_t)((16 - (((uintptr_t)dst) & 15)) & 15);
    head = head < len ? head : len;
    const int64_t n16 = (len - head) >> 4;
    if (tid < head) dst[tid] = src[tid];
    for (int64_t k = tid; k < n16; k += NFC_THREADS) {
        uint4 v;
        __builtin_memcpy(&v, src + head + 16 * k, 16);
        *reinterpret_cast<uint4*>(dst + head + 16 * k) = v;
    }
    const int64_t tail = head + 16 * n16;
    if (tail + tid < len) dst[tail + tid] = src[tail + tid];
}

template <int WRITE>
__global__ __launch_bounds__(NFC_THREADS) void td_nfc_tiles(const NfcArgs a) {
    __shared__ int32_t s_off[RC_LDS_DOCS];  // doc_off[kb + i] - t0, clamped to [NFC_OFF_LO, NFC_OFF_HI]
    __shared__ long long s_red[NFC_THREADS / 64];
    const int tid = threadIdx.x;
    if (nfc_bad_offsets(a, !WRITE)) return;
    if (WRITE && a.head[NFC_H_FULL]) return;
    const NfcTables T = nfc_tables();
    const int64_t total = a.doc_off[a.n_docs];
    const int shift = (int)(((uintptr_t)a.text) & 15);
    const int64_t ntiles = total > 0 ? (total + shift + NFC_TILE - 1) / NFC_TILE : 0;
    const auto off_of = [off = a.doc_off](int64_t d) { return off[d]; };
    NfcLaneStats st = {0, 0, 0, 0};
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t t0 = t * NFC_TILE - shift < 0 ? 0 : t * NFC_TILE - shift;
        const int64_t s1 = (t + 1) * NFC_TILE - shift < total ? (t + 1) * NFC_TILE - shift : total;
        const int64_t b0 = t * NFC_TILE + 16 * tid - shift, b = b0 < 0 ? 0 : b0, we = b0 + 16 < total ? b0 + 16 : total;
        const bool owns = b < we;
        // a window of bytes below 0xCC, begun and followed by a byte that is no continuation byte: boundaries only, a copy
        // (PLAIN: ASCII alone, sixteen code points and no opaque byte; a fast window with a byte from 0x80 on is still a copy, but MEASURE
        // walks it for counts[5] and counts[6]: which of its bytes are opaque depends on the documents' ends too)
        bool fast = !owns, plain = !owns;
        if (owns && b0 >= 0 && b0 + 16 <= total) {
            const uint4 v = *reinterpret_cast<const uint4*>(a.text + b);
            if (nfc_hits(v) == 0 && (a.text[b] & 0xC0) != 0x80) {
                fast = we == total || ((a.text[we] & 0xC0) != 0x80 && a.text[we] < NFC_LEAD_MIN);
                plain = fast && ((v.x | v.y | v.z | v.w) & 0x80808080u) == 0;
            }
        }
        // the tile's documents: kb the last that starts in front of t0 (t0 == 0: the first), its table, where a lane needs one
        const bool need = WRITE || !plain;
        int64_t kb = 0, nk = 0;
        bool lds = true;
        __syncthreads();  // (the tile before has read its table)
        if (__syncthreads_or(need)) {
            kb = t0 > 0 ? group_last_le(off_of, 0, a.n_docs, t0 - 1) : 0;
            nk = tile_table(s_off, off_of, kb, a.n_docs, t0, NFC_OFF_LO, NFC_OFF_HI, (int32_t)(s1 - t0), lds);
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
            if (lds) return nfc_lane<MODE>(a, T, b, we, total, ub_of(rel_lds), opos, st);
            return nfc_lane<MODE>(a, T, b, we, total, ub_of(rel_glb), opos, st);
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
            const int64_t n = !owns ? 0 : plain ? we - b : lane(std::integral_constant<int, NFC_MEASURE>{}, 0);
            if (owns && plain) st.longest = st.longest > 1 ? st.longest : 1;
            const long long sum = block_sum(n, s_red);
            if (tid == 0) a.tile_base[t] = (unsigned long long)sum;
        } else {
            const int64_t n = !owns ? 0 : fast ? we - b : lane(std::integral_constant<int, NFC_SIZE>{}, 0);
            long long sum;
            const int64_t opos = (int64_t)a.tile_base[t] + block_excl(n, s_red, sum);
            if (__syncthreads_and(fast)) {
                nfc_group_copy(a.out + a.tile_base[t], a.text + t0, s1 - t0);
                if (owns) put_starts(opos);
            } else if (fast && owns) {
                for (int64_t q = b; q < we; ++q) a.out[opos + (q - b)] = a.text[q];
                put_starts(opos);
            } else {
                lane(std::integral_constant<int, NFC_WRITE>{}, opos);
            }
        }
    }
    if (!WRITE) {
        const long long seg = block_sum(st.segments, s_red), cps = block_sum(st.cps, s_red), opq = block_sum(st.opaque, s_red);
        const long long lng = block_max(st.longest, s_red);
        if (tid == 0) {
            if (seg) nfc_add(a.counts + NFC_C_SEGMENTS, (unsigned long long)seg);
            if (cps) nfc_add(a.counts + NFC_C_CPS, (unsigned long long)cps);
            if (opq) nfc_add(a.counts + NFC_C_OPAQUE, (unsigned long long)opq);
            if (lng) atomicMax(a.counts + NFC_C_LONGEST, (unsigned long long)lng);
        }
    }
}

__global__ __launch_bounds__(NFC_THREADS) void td_nfc_scan(const NfcArgs a) {
    __shared__ long long s_wave[NFC_THREADS / 64];
    if (a.head[NFC_H_BAD]) return;
    const int64_t total = a.doc_off[a.n_docs];
    const int shift = (int)(((uintptr_t)a.text) & 15);
    const int64_t ntiles = total > 0 ? (total + shift + NFC_TILE - 1) / NFC_TILE : 0;
    long long carry[1];
    chunks_excl_scan<1>(a.tile_base, ntiles, s_wave, carry);
    const int64_t need = carry[0];
    if (threadIdx.x == 0) {
        a.counts[NFC_C_BYTES] = (unsigned long long)need;
        if (need > a.out_capacity) {
            a.head[NFC_H_FULL] = 1;
            rows_raise(a, TD_E_CAPACITY, need);
        }
    }
    if (need > a.out_capacity) return;
    // the documents that start at the text's end (the entry behind the last one among them): no window holds them
    for (int64_t d = a.n_docs - threadIdx.x; d >= 0 && a.doc_off[d] == total; d -= NFC_THREADS) a.out_doc_off[d] = need;
}

unsigned nfc_grid(int64_t n, int64_t per, int64_t most) {
    const int64_t g = (n + per - 1) / per;
    return (unsigned)(g < 1 ? 1 : g < most ? g : most);
}

}  // namespace

hipError_t launch_nfc_check(const NfcArgs& a, hipStream_t stream) {
    hipError_t e;
    hipLaunchKernelGGL(td_nfc_docs, dim3(nfc_grid(a.n_docs + 1, NFC_THREADS, 4096)), dim3(NFC_THREADS), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(td_nfc_clear, dim3(nfc_grid(a.n_docs + NFC_C_WORDS, NFC_THREADS, 4096)), dim3(NFC_THREADS), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // four windows a lane, and at most 2048 workgroups (eight a CU) that stride over the rest
    hipLaunchKernelGGL(td_nfc_check, dim3(nfc_grid(a.n_bytes + 16, 4 * NFC_TILE, 2048)), dim3(NFC_THREADS), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(td_nfc_sums, dim3(nfc_grid(a.n_docs, NFC_THREADS, 4096)), dim3(NFC_THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_nfc(const NfcArgs& a, hipStream_t stream, int phases) {
    hipError_t e;
    const unsigned tiles = nfc_grid(a.n_bytes + 16, NFC_TILE, NFC_MAX_GRID);
    if (phases & NFC_RUN_MEASURE) {
        hipLaunchKernelGGL(td_nfc_docs, dim3(nfc_grid(a.n_docs + 1, NFC_THREADS, 4096)), dim3(NFC_THREADS), 0, stream, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(td_nfc_clear, dim3(nfc_grid(a.n_docs + NFC_C_WORDS, NFC_THREADS, 4096)), dim3(NFC_THREADS), 0, stream, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(td_nfc_tiles<0>, dim3(tiles), dim3(NFC_THREADS), 0, stream, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(td_nfc_scan, dim3(1), dim3(NFC_THREADS), 0, stream, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(td_nfc_sums, dim3(nfc_grid(a.n_docs, NFC_THREADS, 4096)), dim3(NFC_THREADS), 0, stream, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (phases & NFC_RUN_WRITE) hipLaunchKernelGGL(td_nfc_tiles<1>, dim3(tiles), dim3(NFC_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace td
