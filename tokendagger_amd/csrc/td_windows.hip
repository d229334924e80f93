// Overlapping window rows (td_window_rows*, td_encode_batch_window_rows): ids + per-document token offsets -> rows of S slots,
// one document per row; a document longer than the body room C = S - b - e continues in further rows of its own, each starting
// step = C - overlap ids after the one before.
//
// Document d has w_d = max(1, ceil((L_d - overlap) / step)) rows, and its first row is the exclusive prefix sum of w: unlike
// CONCAT and PAD no closed form, unlike BESTFIT nothing sequential.  Three small launches make first_row[n_docs + 1]; no lane
// waits for another workgroup in any of them, so there is nothing to bound:
//
//   td_win_count    w_d of 1024 documents a workgroup (the division by a host-computed multiplier), the offsets checks, the
//                   chunk's rows into the scan words, the counts by one atomic a workgroup
//   td_win_chunks   one workgroup: the chunks' rows -> their exclusive prefixes (chunks_excl_scan<1>, td_rows_common.h),
//                   first_row[n_docs] = rows (-1: bad offsets), the capacity check, counts
//   td_win_first    first_row[d] = the chunk's prefix + the scan inside the chunk
//   td_win_slots    the slots.  td_rows_pad's shape: tiles of 4096 OUTPUT slots, four a lane stored as one int4, so a document of
//                   a quarter of a million ids is written by as many lanes as its rows have slots.  The rows of a tile are
//                   consecutive and their documents ascend: group_last_le over first_row finds the document of the tile's
//                   first row (inside [r - (rows - n_docs), r]: first_row[d] - d never decreases, so without a split document
//                   the search is no step at all), tile_table puts the first rows of the tile's documents into LDS, and a lane
//                   finds its row's document there (last_le; all three in td_rows_common.h).  The tile in which a row starts
//                   writes the row's length, document and start.  <WindowLabArgs>: the pair form, lab.src -> lab.dst beside the
//                   ids and the overlap mask (td_rows_common.h); <WindowArgs>: one stream.
//
// td_win_slots reads first_row[n_docs] itself (a kernel boundary lies behind td_win_chunks): above the capacity, or -1, it
// leaves without a store.
#include <hip/hip_runtime.h>

#include "td_rows_common.h"
#include "td_windows.h"

namespace td {

namespace {

constexpr int WIN_THREADS = RC_THREADS, WIN_TILE = RC_TILE, WIN_MAX_GRID = RC_MAX_GRID;

// L_d; 0 with `bad` set unless 0 <= tok_off[d] <= tok_off[d + 1] <= n_tokens
__device__ __forceinline__ int64_t win_len(const WindowArgs& a, int64_t d, bool& bad) {
    const int64_t lo = a.tok_off[d], hi = a.tok_off[d + 1];
    if (lo < 0 || hi < lo || hi > a.n_tokens) {
        bad = true;
        return 0;
    }
    return hi - lo;
}

// w_d = max(1, ceil((L - overlap) / step)): L <= C is one window, more is at least two
__device__ __forceinline__ int64_t win_count(const WindowArgs& a, int64_t L) {
    return L <= a.C ? 1 : div_magic(L - a.overlap + a.step - 1, a.step, a.step_magic);
}

__global__ __launch_bounds__(WIN_THREADS) void td_win_count(const WindowArgs a) {
    __shared__ long long s_red[WIN_THREADS / 64];
    const int tid = threadIdx.x;
    long long rows = 0, real = 0, multi = 0, mx = 0;
    bool bad = false;
    int64_t bad_at = 0;
    for (int q = 0; q < 4; ++q) {
        const int64_t d = (int64_t)blockIdx.x * RC_SCAN_CHUNK + tid * 4 + q;
        if (d >= a.n_docs) break;
        bool bd = false;
        const int64_t L = win_len(a, d, bd), w = win_count(a, L);
        if (bd && !bad) bad_at = d;
        bad |= bd;
        rows += w;
        real += w * (a.b + a.e) + L + (w - 1) * a.overlap;
        multi += w > 1;
        mx = w > mx ? w : mx;
    }
    if (a.n_docs == 0 && blockIdx.x == 0 && tid == 0) {
        const int64_t o = a.tok_off[0];
        bad = o < 0 || o > a.n_tokens;
    }
    if (bad) rows_raise(a, TD_E_INVALID, bad_at);
    rows = block_sum(rows, s_red);
    real = block_sum(real, s_red);
    multi = block_sum(multi, s_red);
    mx = block_max(mx, s_red);
    const long long any_bad = block_max(bad, s_red);
    if (tid == 0) {
        a.scan[WIN_SCAN_HEAD + blockIdx.x] = (unsigned long long)rows;
        if (real) atomicAdd(&a.scan[0], (unsigned long long)real);
        if (multi) atomicAdd(&a.scan[1], (unsigned long long)multi);
        if (mx) atomicMax(&a.scan[2], (unsigned long long)mx);
        if (any_bad) atomicAdd(&a.scan[3], 1ull);
    }
}

__global__ __launch_bounds__(WIN_THREADS) void td_win_chunks(const WindowArgs a, int64_t nch) {
    __shared__ long long s_wave[WIN_THREADS / 64];
    const int tid = threadIdx.x;
    long long carry[1];
    chunks_excl_scan<1>(a.scan + WIN_SCAN_HEAD, nch, s_wave, carry);
    if (tid == 0) {
        const bool bad = a.scan[3] != 0;
        const int64_t rows = a.n_docs > 0 ? carry[0] : 0;
        a.first_row[a.n_docs] = bad ? -1 : rows;
        const bool fits = !bad && rows <= a.rows_cap;
        if (!bad && !fits) rows_raise(a, TD_E_CAPACITY, rows);
        a.counts[0] = bad ? 0 : rows;
        a.counts[1] = fits ? (long long)a.scan[0] : 0;
        a.counts[2] = fits ? (long long)a.scan[1] : 0;
        a.counts[3] = fits ? (long long)a.scan[2] : 0;
    }
}

__global__ __launch_bounds__(WIN_THREADS) void td_win_first(const WindowArgs a) {
    __shared__ long long s_wave[WIN_THREADS / 64];
    const int tid = threadIdx.x;
    long long v[4], sum = 0;
    for (int q = 0; q < 4; ++q) {
        const int64_t d = (int64_t)blockIdx.x * RC_SCAN_CHUNK + tid * 4 + q;
        bool bd = false;
        v[q] = d < a.n_docs ? win_count(a, win_len(a, d, bd)) : 0;
        sum += v[q];
    }
    long long total;
    long long run = (long long)a.scan[WIN_SCAN_HEAD + blockIdx.x] + block_excl(sum, s_wave, total);
    for (int q = 0; q < 4; ++q) {
        const int64_t d = (int64_t)blockIdx.x * RC_SCAN_CHUNK + tid * 4 + q;
        if (d < a.n_docs) a.first_row[d] = run;
        run += v[q];
    }
}

template <class A>
__global__ __launch_bounds__(WIN_THREADS) void td_win_slots(const A a) {
    constexpr bool LAB = has_lab<A>;
    // (rows ascend by one and a document has at least one: at most WIN_TILE + 1 documents have a row in the tile, and the step of
    // the table that holds the one behind them ends below RC_LDS_DOCS; tile_table always fits)
    static_assert(RC_LDS_DOCS >= WIN_TILE + 1 + WIN_THREADS - 1, "td_win_slots has no path for a table that does not fit");
    __shared__ int32_t s_fr[RC_LDS_DOCS];  // first rows of the tile's documents - r0, clamped to [-1, WIN_TILE + 2]
    const int tid = threadIdx.x;
    const int64_t rows = a.first_row[a.n_docs];
    if (rows < 0 || rows > a.rows_cap) return;
    const int64_t S = a.S, total = rows * S, extra = rows - a.n_docs;
    const int64_t ntiles = (total + WIN_TILE - 1) / WIN_TILE;
    const auto first_of = [fr = a.first_row](int64_t d) { return fr[d]; };
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t s0 = tile * WIN_TILE;
        const int64_t s1 = s0 + WIN_TILE < total ? s0 + WIN_TILE : total;
        const int64_t r0 = div_magic(s0, S, a.s_magic);
        const int nr = (int)(div_magic(s1 - 1, S, a.s_magic) - r0) + 1;  // rows [r0, r0 + nr) have slots in the tile
        __syncthreads();  // (the previous tile's readers of s_fr are done)
        // d0: the last document with first_row[d] <= r0.  d <= first_row[d] <= d + extra bounds it
        const int64_t d0 = group_last_le(first_of, r0 > extra ? r0 - extra : 0, (r0 < a.n_docs - 1 ? r0 : a.n_docs - 1) + 1, r0);
        const int64_t fr0 = a.first_row[d0];
        // documents with rows in the tile: s_fr[0, nl), and s_fr[nl] the first row of the next (>= nr)
        const int nl = tile_table(s_fr, first_of, d0, a.n_docs, r0, -1, WIN_TILE + 2, nr);
        for (int it = 0; it < WIN_TILE / (4 * WIN_THREADS); ++it) {
            const int64_t j0 = s0 + (int64_t)it * 4 * WIN_THREADS + 4 * tid;
            if (j0 >= s1) break;
            int64_t r = div_magic(j0, S, a.s_magic), o = j0 - r * S;
            int i = last_le(s_fr, nl, (int32_t)(r - r0));  // the row's document: the last of the tile's with first row <= r
            int64_t d = 0, tlo = 0, start = 0, body = 0, len = 0;
            auto load_row = [&] {
                d = d0 + i;
                tlo = a.tok_off[d];
                const int64_t L = a.tok_off[d + 1] - tlo;
                start = (r - (i == 0 ? fr0 : r0 + s_fr[i])) * a.step;
                body = L - start;
                body = body < 0 ? 0 : body > a.C ? a.C : body;
                len = a.b + body + a.e;
            };
            load_row();
            int32_t v[4], ps[4];
            [[maybe_unused]] int32_t lv[4];
            bool fast = false;
            const int64_t src = tlo + start + o - a.b;
            if (o + 4 <= S && j0 + 4 <= s1 && o >= a.b && o + 4 <= a.b + body && src >= 0 && src + 4 <= a.n_tokens) {
                const int32_t* p = a.ids + src;  // (four dwords: the sources are misaligned three times out of four)
                v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
                if constexpr (LAB) rows_get4(a.lab.src, src, lv);
                fast = true;
            }
            for (int q = 0; q < 4; ++q) {
                if (j0 + q >= s1) break;
                if (q > 0 && ++o == S) {
                    o = 0;
                    ++r;
                    if (i + 1 < nl && s_fr[i + 1] <= (int32_t)(r - r0)) ++i;
                    load_row();
                }
                if constexpr (LAB) {
                    if (!fast) {
                        if (o < a.b) { v[q] = a.bos; lv[q] = a.lab.bos; }
                        else if (o < a.b + body) v[q] = rows_load1_pair(a, tlo + start + o - a.b, lv[q]);
                        else if (a.e && o == a.b + body) { v[q] = a.eos; lv[q] = a.lab.eos; }
                        else { v[q] = a.pad; lv[q] = a.lab.pad; }
                    }
                    // the ids a window k > 0 repeats: body slots [0, overlap), all below its body (body > overlap there)
                    if (a.lab.mask_overlap && start > 0 && o >= a.b && o < a.b + a.overlap && o < a.b + body) lv[q] = a.lab.pad;
                } else if (!fast) {
                    if (o < a.b) v[q] = a.bos;
                    else if (o < a.b + body) v[q] = rows_load1(a, tlo + start + o - a.b);
                    else if (a.e && o == a.b + body) v[q] = a.eos;
                    else v[q] = a.pad;
                }
                ps[q] = o < len ? (int32_t)o : 0;
                if (o == 0) {
                    if (a.row_len) a.row_len[r] = (int32_t)len;
                    if (a.row_doc) a.row_doc[r] = d;
                    if (a.row_start) a.row_start[r] = start;
                }
            }
            rows_put4(a.out, j0, s1, v);
            lab_put4(a, j0, s1, lv);
            if (a.pos) rows_put4(a.pos, j0, s1, ps);
        }
    }
}

}  // namespace

int64_t windows_scan_words(int64_t n_docs) { return WIN_SCAN_HEAD + (n_docs > 0 ? (n_docs + RC_SCAN_CHUNK - 1) / RC_SCAN_CHUNK : 1); }

hipError_t launch_windows(const WindowLabArgs& al, hipStream_t stream) {
    const WindowArgs& a = al;
    const int64_t nch = windows_scan_words(a.n_docs) - WIN_SCAN_HEAD;
    hipLaunchKernelGGL(td_win_count, dim3((unsigned)nch), dim3(WIN_THREADS), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(td_win_chunks, dim3(1), dim3(WIN_THREADS), 0, stream, a, nch);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(td_win_first, dim3((unsigned)nch), dim3(WIN_THREADS), 0, stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const int64_t tiles = (a.rows_cap * a.S + WIN_TILE - 1) / WIN_TILE;  // (the host keeps rows_cap * S far from overflow)
    const int grid = (int)(tiles < 1 ? 1 : tiles < WIN_MAX_GRID ? tiles : WIN_MAX_GRID);
    if (al.lab.src) hipLaunchKernelGGL(td_win_slots<WindowLabArgs>, dim3(grid), dim3(WIN_THREADS), 0, stream, al);
    else hipLaunchKernelGGL(td_win_slots<WindowArgs>, dim3(grid), dim3(WIN_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace td
