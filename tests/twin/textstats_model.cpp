// CPU model of td_textstats.hip's decomposition over tokendagger_amd/csrc/td_textstats_args.h (the rule of one byte, a window's classes
// and its walk are the kernels' own): windows of 16 bytes at 16 g - shift (shift: the base pointer's misalignment), a lane a window,
// tile / 16 windows a tile; under TS_RUNS the tiles' four last positions, their inclusive prefix maxima in sweeps of a tile a lane with
// the carry across sweeps, and the exclusive maximum scan across a tile's lanes behind the tile in front; the walk, a lane's sums
// flushed when its document changes and at its window's end; the totals by a pass over the documents.  The tile size is an argument.
// textstats_host is the host statement itself (ts_host), for the tests that run without the product's library.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../tokendagger_amd/csrc/td_tables.h"
#include "../../tokendagger_amd/csrc/td_textstats_args.h"

using namespace td;

namespace {

struct Window {
    int64_t b0, b, we;
    uint32_t w[4], c[4];
    TsCursor cur;
    TsLane S;
};

int64_t doc_of(const int64_t* off, int64_t n_docs, int64_t p) { return (int64_t)(std::upper_bound(off, off + n_docs, p) - off) - 1; }

}  // namespace

extern "C" int textstats_host(const uint8_t* text, const int64_t* off, int64_t n_docs, int groups, int64_t* stats, int64_t* totals) {
    return ts_host(class_tables(), text, off, n_docs, groups, stats, totals);
}

// info[4]: tiles, sweeps of the prefix maximum, windows without a byte >= 0x80, flushes in the middle of a window.
// Returns 0, or 1 for bad arguments.
extern "C" int textstats_model(const uint8_t* text, const int64_t* off, int64_t n_docs, int groups, int tile, int shift, int64_t* stats,
                               int64_t* totals, int64_t* info) {
    if (tile < 64 || tile % 16 || shift < 0 || shift > 15 || n_docs < 0 || !ts_groups_ok(groups) || !rewrite_offsets_ok(off, n_docs)) return 1;
    const Tables T = class_tables();
    const int64_t total = off[n_docs];
    const int lanes = tile / 16;
    const int64_t ntiles = total > 0 ? (total + shift + tile - 1) / tile : 0;
    memset(info, 0, 4 * sizeof(int64_t));
    info[0] = ntiles;
    // ---- reset ----------------------------------------------------------------------------------------------------------------------
    for (int64_t i = 0; i < n_docs * TS_COLS; ++i) stats[i] = (groups & TS_LOCAL) && i % TS_COLS == TS_BYTES ? off[i / TS_COLS + 1] - off[i / TS_COLS] : 0;
    const auto window = [&](int64_t t, int l) {
        Window W;
        W.b0 = t * tile + 16 * l - shift;
        W.b = std::max<int64_t>(W.b0, 0);
        W.we = std::min(W.b0 + 16, total);
        W.S = {-1, -1, -1, -1, false};
        W.cur = {-1, 0, 0};
        if (W.b >= W.we) return W;
        ts_load_bytes(text, W.b0, W.b, W.we, W.w);
        W.cur.D = doc_of(off, n_docs, W.b);
        W.cur.ds = off[W.cur.D];
        W.cur.de = off[W.cur.D + 1];
        ts_window_classes(T, T.ascii_cls, text, off, W.b0, W.b, W.we, W.w, W.cur, W.c, W.S);
        return W;
    };
    // ---- carry and prefix (TS_RUNS) ---------------------------------------------------------------------------------------------------
    std::vector<long long> carry((size_t)ntiles * 4 + 4, -1);
    if (groups & TS_RUNS) {
        for (int64_t t = 0; t < ntiles; ++t) {
            long long m[4] = {-1, -1, -1, -1};
            for (int l = 0; l < lanes; ++l) {
                const Window W = window(t, l);
                const long long v[4] = {W.S.lf, W.S.sp, W.S.vis, W.S.let};
                for (int k = 0; k < 4; ++k) m[k] = std::max(m[k], v[k]);
            }
            for (int k = 0; k < 4; ++k) carry[(size_t)(4 * t + k)] = m[k];
        }
        long long run[4] = {-1, -1, -1, -1};
        for (int64_t base = 0; base < ntiles; base += lanes) {  // a sweep: a tile a lane
            ++info[1];
            long long all[4] = {-1, -1, -1, -1};
            std::vector<long long> before((size_t)lanes * 4, -1);
            for (int l = 0; l < lanes && base + l < ntiles; ++l)
                for (int k = 0; k < 4; ++k) {
                    before[(size_t)(4 * l + k)] = all[k];
                    all[k] = std::max(all[k], carry[(size_t)(4 * (base + l) + k)]);
                }
            for (int l = 0; l < lanes && base + l < ntiles; ++l)
                for (int k = 0; k < 4; ++k) {
                    long long& v = carry[(size_t)(4 * (base + l) + k)];
                    v = std::max(std::max(before[(size_t)(4 * l + k)], run[k]), v);
                }
            for (int k = 0; k < 4; ++k) run[k] = std::max(run[k], all[k]);
        }
    }
    // ---- the walk -----------------------------------------------------------------------------------------------------------------
    const auto put = [&](int64_t D, const TsAcc& A) {
        for (int c = 1; c < TS_COLS; ++c) {
            int64_t& s = stats[D * TS_COLS + c];
            s = ts_is_max(c) ? std::max(s, ts_acc_col(A, c)) : s + ts_acc_col(A, c);
        }
    };
    for (int64_t t = 0; t < ntiles; ++t) {
        long long in[4] = {-1, -1, -1, -1};
        if ((groups & TS_RUNS) && t > 0)
            for (int k = 0; k < 4; ++k) in[k] = carry[(size_t)(4 * (t - 1) + k)];
        for (int l = 0; l < lanes; ++l) {
            Window W = window(t, l);
            if (W.b < W.we) {
                info[2] += ts_window_ascii(W.w);
                TsLane L = {-1, -1, -1, -1, false};
                if (groups & TS_RUNS) L = {in[0], in[1], in[2], in[3], false};
                L.prev_space = ts_space_before(T, T.ascii_cls, text, W.b, W.cur.ds, W.cur.de);
                TsAcc A;
                memset(&A, 0, sizeof A);
                const auto flush = [&](int64_t D, const TsAcc& X) { ++info[3]; put(D, X); };
                if (groups == TS_LOCAL) ts_window_walk<TS_LOCAL>(text, off, W.b0, W.b, W.we, W.w, W.c, W.cur, L, A, flush);
                else if (groups == TS_RUNS) ts_window_walk<TS_RUNS>(text, off, W.b0, W.b, W.we, W.w, W.c, W.cur, L, A, flush);
                else ts_window_walk<TS_LOCAL | TS_RUNS>(text, off, W.b0, W.b, W.we, W.w, W.c, W.cur, L, A, flush);
                put(W.cur.D, A);
            }
            const long long v[4] = {W.S.lf, W.S.sp, W.S.vis, W.S.let};  // (the exclusive scan across the lanes)
            for (int k = 0; k < 4; ++k) in[k] = std::max(in[k], v[k]);
        }
    }
    // ---- totals -------------------------------------------------------------------------------------------------------------------
    if (totals) {
        for (int c = 0; c < TS_COLS; ++c) totals[c] = 0;
        for (int64_t d = 0; d < n_docs; ++d)
            for (int c = 0; c < TS_COLS; ++c) totals[c] = ts_is_max(c) ? std::max(totals[c], stats[d * TS_COLS + c]) : totals[c] + stats[d * TS_COLS + c];
    }
    return 0;
}
