// CPU model of td_counts.hip's decomposition, over the shared header (tokendagger_amd/csrc/td_counts_args.h: the constants, the
// grid and the seat hash).  The seats, the flush interval, the grid and the capacity of the tile's document table are parameters.
// What it follows from the kernel:
//
//   range    the visited positions [lo, hi) clamped into the buffer, offsets that leave it raised
//   grid     workgroup b takes the tiles lo / CNT_TILE + b, + grid, ...: absolute multiples of the tile
//   docs     (groups) the tile's first document by bisection, the documents that begin inside the tile by the table when they fit
//            and by bisection of tok_offsets when they do not; a tile inside one document resolves its group once
//   step     a wavefront's 64 lanes bring one position each (lane l of wave w, load `it`, element q: t0 + it * 1024 + 4 * (64 w + l) + q);
//            64 equal keys are one add by lane 0; otherwise every key tries cnt_seat(key) and that ^ 1, first come first seated
//   conflict keys without a seat go to the counts at once, the equal ones of the step as ONE add
//   flush    behind every flush_tiles tiles of a workgroup and behind its last: occupied seats only, one add each, seats cleared
// The lanes of a step are seated in lane order and the wavefronts of a tile one after the other: the kernel's order is another,
// the sums are the same.  stats: adds to the counts from conflicts, from flushes, adds to seats, tiles.
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../tokendagger_amd/csrc/td_counts_args.h"

using namespace td;

namespace {

static_assert(CNT_TILE == 4096 && CNT_THREADS == 256, "the model's lane arithmetic");
constexpr int TD_E_INVALID_ = 1;

template <class Key>
int64_t last_le(Key key, int64_t lo, int64_t hi, long long x) {
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (key(mid) <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

struct Model {
    const int32_t* ids; int64_t n_tokens; const int64_t* tok_off; int64_t n_docs; const int32_t* doc_group; int64_t n_bins, n_groups;
    int seat_bits, flush_tiles; int64_t table_cap;
    int64_t* counts; int64_t info[4] = {}; int64_t stats[4] = {};
    int err = 0; int64_t err_pos = -1;
    std::vector<int32_t> s_key; std::vector<uint32_t> s_cnt;

    void raise(int code, int64_t pos) { if (!err) { err = code; err_pos = pos; } }

    bool take(uint32_t s, int32_t key) {
        if (s_key[s] == CNT_EMPTY) { s_key[s] = key; return true; }
        return s_key[s] == key;
    }

    void flush() {
        for (size_t s = 0; s < s_key.size(); ++s)
            if (s_key[s] != CNT_EMPTY) {
                counts[s_key[s]] += s_cnt[s];
                ++stats[1];
                s_key[s] = CNT_EMPTY;
                s_cnt[s] = 0;
            }
    }

    void step(const int32_t key[64]) {
        bool uniform = true;
        for (int l = 1; l < 64; ++l) uniform &= key[l] == key[0];
        if (uniform) {
            if (key[0] == CNT_EMPTY) return;
            uint32_t s = cnt_seat(key[0], seat_bits);
            bool seated = take(s, key[0]);
            if (!seated) seated = take(s ^= 1u, key[0]);
            if (seated) { s_cnt[s] += 64; ++stats[2]; }
            else { counts[key[0]] += 64; ++stats[0]; }
            return;
        }
        int32_t pend[64];
        for (int l = 0; l < 64; ++l) {
            pend[l] = CNT_EMPTY;
            if (key[l] == CNT_EMPTY) continue;
            uint32_t s = cnt_seat(key[l], seat_bits);
            bool seated = take(s, key[l]);
            if (!seated) seated = take(s ^= 1u, key[l]);
            if (seated) { ++s_cnt[s]; ++stats[2]; }
            else pend[l] = key[l];
        }
        for (int l = 0; l < 64; ++l) {
            if (pend[l] == CNT_EMPTY) continue;
            const int32_t k = pend[l];
            int64_t n = 0;
            for (int m = l; m < 64; ++m)
                if (pend[m] == k) { ++n; pend[m] = CNT_EMPTY; }
            counts[k] += n;
            ++stats[0];
        }
    }

    void run(int grid) {
        int64_t lo = 0, hi = n_tokens;
        if (tok_off) {
            lo = tok_off[0];
            hi = tok_off[n_docs];
            if (lo < 0 || hi < lo || hi > n_tokens) {
                raise(TD_E_INVALID_, lo < 0 ? 0 : n_docs);
                lo = std::max<int64_t>(lo, 0);
                hi = std::min(hi, n_tokens);
                hi = std::max(hi, lo);
            }
        }
        const int64_t stop = lo < hi ? hi : 0;
        const bool groups = doc_group != nullptr;
        const auto off = [this](int64_t k) { return tok_off[k]; };
        if (groups)  // (the grid's slices of the offsets, as one loop)
            for (int64_t d = 0; d < n_docs; ++d)
                if (off(d + 1) < off(d)) raise(TD_E_INVALID_, d);
        for (int b = 0; b < grid; ++b) {
            s_key.assign((size_t)1 << seat_bits, CNT_EMPTY);
            s_cnt.assign((size_t)1 << seat_bits, 0);
            int since = 0;
            for (int64_t tile = lo / CNT_TILE + b; tile * CNT_TILE < stop; tile += grid) {
                ++stats[3];
                const int64_t t0 = tile * CNT_TILE, s0 = std::max(t0, lo), s1 = std::min<int64_t>(t0 + CNT_TILE, hi);
                int64_t k0 = 0, nk = 1;
                bool lds = true;
                if (groups) {
                    k0 = last_le(off, 0, n_docs, s0);
                    // the table: documents behind k0 in steps of CNT_THREADS until one begins at or behind the tile's end
                    nk = 0;
                    lds = false;
                    for (int64_t c0 = 0; c0 < table_cap && !lds; c0 += CNT_THREADS) {
                        int c = 0;
                        for (int64_t i = c0; i < c0 + CNT_THREADS; ++i) c += (k0 + i <= n_docs ? std::max<int64_t>(off(k0 + i) - s0, 0) : CNT_TILE + 1) < s1 - s0;
                        nk += c;
                        lds = c < CNT_THREADS;
                    }
                    if (!lds) nk = last_le(off, k0, n_docs, s1 - 1) - k0 + 1;
                }
                const bool one = nk <= 1;
                for (int w = 0; w < CNT_THREADS / 64; ++w)
                    for (int it = 0; it < 4; ++it)
                        for (int q = 0; q < 4; ++q) {
                            int32_t key[64];
                            for (int l = 0; l < 64; ++l) {
                                key[l] = CNT_EMPTY;
                                const int64_t j = t0 + (int64_t)it * 4 * CNT_THREADS + 4 * (64 * w + l) + q;
                                if (j < s0 || j >= s1) continue;
                                int64_t g = 0;
                                bool bad = false;
                                if (groups) {
                                    const int64_t d = one ? k0 : k0 + last_le([&](int64_t i) { return off(k0 + i); }, 0, nk, j);
                                    g = doc_group[d];
                                    bad = g < 0 || g >= n_groups;
                                    if (bad) raise(TD_E_INVALID_, d);
                                }
                                const int32_t x = ids[j];
                                if (bad) ++info[CNT_I_BAD_GROUP];
                                else if (x < 0) ++info[CNT_I_NEGATIVE];
                                else if (x >= n_bins) ++info[CNT_I_TOO_LARGE];
                                else {
                                    ++info[CNT_I_COUNTED];
                                    key[l] = (int32_t)(g * n_bins + x);
                                }
                            }
                            step(key);
                        }
                if (++since >= flush_tiles) { flush(); since = 0; }
            }
            if (since) flush();
        }
    }
};

}  // namespace

extern "C" {

// counts: the caller's (zeroed, or accumulated into).  seat_bits 0, flush_tiles 0, grid 0, table_cap 0: the kernel's.  -> the
// error code (0: none), *err_pos its position; info[4], stats[4].
int counts_model(const int32_t* ids, int64_t n_tokens, const int64_t* tok_off, int64_t n_docs, const int32_t* doc_group, int64_t n_bins,
                 int64_t n_groups, int seat_bits, int flush_tiles, int grid, int64_t table_cap, int64_t* counts, int64_t* info, int64_t* stats,
                 int64_t* err_pos) {
    Model m;
    m.ids = ids; m.n_tokens = n_tokens; m.tok_off = tok_off; m.n_docs = n_docs; m.doc_group = doc_group; m.n_bins = n_bins; m.n_groups = n_groups;
    int bits = 0;
    while ((1 << bits) < CNT_SEATS) ++bits;
    m.seat_bits = seat_bits ? seat_bits : bits;
    m.flush_tiles = flush_tiles ? flush_tiles : CNT_FLUSH_TILES;
    m.table_cap = table_cap ? table_cap : 4352;  // td::RC_LDS_DOCS, which lives in a device header; tests/test_counts_model.py compares the two
    m.counts = counts;
    m.run(grid ? grid : cnt_grid(n_tokens));
    for (int k = 0; k < 4; ++k) { info[k] = m.info[k]; stats[k] = m.stats[k]; }
    *err_pos = m.err_pos;
    return m.err;
}

// the header's constants, for the test: seats, flush interval, tile, grid of n_tokens
int64_t counts_model_const(int what, int64_t n_tokens) {
    switch (what) {
        case 0: return CNT_SEATS;
        case 1: return CNT_FLUSH_TILES;
        case 2: return CNT_TILE;
        case 3: return cnt_grid(n_tokens);
        case 4: return CNT_MAX_GRID;
    }
    return -1;
}

}  // extern "C"
