// CPU model of td_ranges.hip's decomposition, over the shared header (tokendagger_amd/csrc/td_ranges_args.h: the head-word layout
// and the default sizes).  The tile, the window capacity, the table capacity and its step, the range chunk, the chunks a pass of
// the chunk scan covers and the ids a lane walks are parameters, and the tiles are resolved in the order the caller gives (the
// workgroups of a launch are independent of each other).  What it follows from the kernels, phase by phase:
//
//   docs    both offset arrays checked; the starts of the non-empty documents as a bitmap over the ids, every document's first range
//           as a bitmap over the ranges; covered form: a document without ids may have no range that ends above 0
//   check   a chunk of ranges at a time: the first-range bit in place of the end before it (which is fetched across lane and chunk
//           borders), the lowest bad index as the maximum of 2^63 - 1 - index, cum inside the chunk, the chunk's total
//   cum     the chunk totals to their exclusive prefixes, a pass at a time with the carry between passes; raises the bad range
//   carry   covered form: the bytes of every tile's first document in front of the tile, by the segmented scan's operator
//   apply   per tile: the lanes' starts from the carry, the tile's documents by the table when it fits and by bisection of
//           tok_offsets when it does not, the window [w0, w1) and the staged copy with cum + the chunk's prefix, the walk with
//           the clamp lo0 = max(range_off[d], w0), hi = min(range_off[d + 1], w1), the cursor k (k + 1 first, else bisect), G(e) of
//           the id before reused when s == prev_e, m = G(e) - G(s), the three rules, the covered form's check at a document's
//           last id
//   status  covered form: raises the lowest range beyond its document
//   finish  counts, trained_offsets from the tiles' counts and the positions' prefixes
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../tokendagger_amd/csrc/td_ranges_args.h"

using namespace td;

namespace {

constexpr int64_t MODEL_TABLE = 4352;  // td::RC_LDS_DOCS, which lives in a device header; tests/test_ranges_model.py compares the two
constexpr int64_t MODEL_TABLE_STEP = 256;
static_assert(RNG_TILE == 4096 && RNG_WIN == 512 && RNG_CHUNK == 1024, "ranges_model_defaults");
static_assert(RNG_H_RANGE == 5 && RNG_H_BEYOND == 6 && RNG_H_GAP == 7 && LAB_H_BAD == 0 && LAB_H_TRAINED == 1 && LAB_H_SPANS == 2 &&
                  LAB_H_UNTERM == 3 && LAB_HEAD_WORDS == 8,
              "RangeArgs::head as the model uses it");

constexpr unsigned long long TOP = 0x7FFFFFFFFFFFFFFFull;

struct Seg { uint32_t f; unsigned long long s; };
Seg seg_op(Seg x, Seg y) { return Seg{x.f | y.f, y.f ? y.s : x.s + y.s}; }

// the last index in [lo, hi) whose key is <= x, given key(lo) <= x (it is lo when the given does not hold, or the interval is empty)
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
    const int32_t* ids; const int64_t* tok_off; int64_t n_docs; const int64_t* starts; const int64_t* range_off; const int64_t* ranges;
    int64_t n_ranges; int32_t rule, ignore; const int64_t* lengths; int64_t n_lengths;
    int64_t tile, win, tab, tab_step, chunk, pass, per;
    unsigned long long head[LAB_HEAD_WORDS] = {};
    int err = 0; int64_t err_pos = -1;
    std::vector<uint8_t> bits, rbits;
    std::vector<long long> cum;
    std::vector<unsigned long long> rchunks, chunk_sum;

    void raise(int code, int64_t pos) { if (!err) { err = code; err_pos = pos; } }
    void lowest(int word, int64_t idx) { head[word] = std::max(head[word], TOP - (unsigned long long)idx); }
    void bad_doc(int64_t d) { raise(1, d); head[LAB_H_BAD] |= 1ull; }
    long long len_of(int32_t id) const { return id >= 0 && id < n_lengths ? lengths[id] : 0; }
    int64_t first_beyond(int64_t r0, int64_t r1, long long x) const {
        if (ranges[2 * r0 + 1] > x) return r0;
        return last_le([&](int64_t r) { return ranges[2 * r + 1]; }, r0, r1, x) + 1;
    }
};

}  // namespace

extern "C" void ranges_model_defaults(int64_t* out) {
    out[0] = RNG_TILE; out[1] = RNG_WIN; out[2] = MODEL_TABLE; out[3] = MODEL_TABLE_STEP; out[4] = RNG_CHUNK; out[5] = 4 * 256; out[6] = 16;
}

// sizes: tile, window, table, table step, range chunk, chunks a pass, ids a lane.  order: the tiles, every one once.  lengths[id]: the
// vocabulary's byte lengths (0: no token).  kinds[0 .. 3]: tiles by 2 * fits + staged; kinds[4]: staged windows that cross a chunk border;
// kinds[5]: passes of the chunk scan behind the first.  Returns 0, or 1 (TD_E_INVALID) / 2 (an id that is no token) with *err_pos.
extern "C" int ranges_model(const int32_t* ids, int64_t n_tokens, const int64_t* tok_off, int64_t n_docs, const int64_t* starts,
                            const int64_t* range_off, const int64_t* ranges, int64_t n_ranges, int32_t rule, int32_t ignore,
                            const int64_t* lengths, int64_t n_lengths, const int64_t* sizes, const int64_t* order, int32_t* labels,
                            uint8_t* mask, int64_t* trained_off, int64_t* counts, int64_t* err_pos, int64_t* kinds) {
    Model a;
    a.ids = ids; a.tok_off = tok_off; a.n_docs = n_docs; a.starts = starts; a.range_off = range_off; a.ranges = ranges;
    a.n_ranges = n_ranges; a.rule = rule; a.ignore = ignore; a.lengths = lengths; a.n_lengths = n_lengths;
    a.tile = sizes[0]; a.win = sizes[1]; a.tab = sizes[2]; a.tab_step = sizes[3]; a.chunk = sizes[4]; a.pass = sizes[5]; a.per = sizes[6];
    if (a.tile < 1 || a.win < 1 || a.tab_step < 1 || a.tab < a.tab_step || a.tab % a.tab_step || a.chunk < 1 || a.pass < 1 || a.per < 1) return -1;
    for (int i = 0; i < 6; ++i) kinds[i] = 0;
    *err_pos = -1;
    const auto done = [&]() { *err_pos = a.err_pos; return a.err; };

    // ---- docs ------------------------------------------------------------------------------------------------------------------------
    a.bits.assign((size_t)n_tokens + 2, 0);
    a.rbits.assign((size_t)n_ranges + 2, 0);
    if (tok_off[0] != 0 || range_off[0] != 0) a.bad_doc(0);
    if (range_off[n_docs] != n_ranges) a.bad_doc(n_docs > 0 ? n_docs - 1 : 0);
    for (int64_t d = 0; d < n_docs; ++d) {
        const int64_t lo = tok_off[d], hi = tok_off[d + 1], r0 = range_off[d], r1 = range_off[d + 1];
        if (lo < 0 || hi < lo || hi > n_tokens || r0 < 0 || r1 < r0 || r1 > n_ranges) { a.bad_doc(d); continue; }
        if (hi > lo) a.bits[(size_t)lo] = 1;
        if (r1 > r0) a.rbits[(size_t)r0] = 1;
        if (hi == lo && !starts && r1 > r0 && ranges[2 * (r1 - 1) + 1] > 0) a.lowest(RNG_H_BEYOND, a.first_beyond(r0, r1, 0));
    }
    if (a.head[LAB_H_BAD]) return done();

    // ---- check -----------------------------------------------------------------------------------------------------------------------
    const int64_t nch = (n_ranges + a.chunk - 1) / a.chunk;
    a.cum.assign((size_t)n_ranges + 1, 0);
    a.rchunks.assign((size_t)nch + 2, 0);
    for (int64_t c = nch - 1; c >= 0; --c) {  // (any order)
        long long run = 0;
        for (int64_t r = c * a.chunk; r < std::min(n_ranges, (c + 1) * a.chunk); ++r) {
            const long long prev_end = r > 0 ? ranges[2 * r - 1] : 0, b = ranges[2 * r], e = ranges[2 * r + 1];
            long long len = 0;
            if (b < 0 || e < b || (!a.rbits[(size_t)r] && b < prev_end)) a.lowest(RNG_H_RANGE, r);
            else len = e - b;
            a.cum[(size_t)r] = run;
            run += len;
        }
        a.rchunks[(size_t)c] = (unsigned long long)run;
    }
    // ---- cum -------------------------------------------------------------------------------------------------------------------------
    long long carry = 0;
    for (int64_t base = 0; base < nch; base += a.pass) {
        long long run = 0;  // the pass's own exclusive scan, the carry added on top
        for (int64_t c = base; c < std::min(nch, base + a.pass); ++c) {
            const long long v = (long long)a.rchunks[(size_t)c];
            a.rchunks[(size_t)c] = (unsigned long long)(carry + run);
            run += v;
        }
        carry += run;
        if (base > 0) ++kinds[5];
    }
    a.head[LAB_H_UNTERM] = (unsigned long long)carry;
    if (a.head[RNG_H_RANGE]) {
        a.raise(1, (int64_t)(TOP - a.head[RNG_H_RANGE]));
        return done();
    }

    // ---- carry (covered form) ---------------------------------------------------------------------------------------------------------
    const int64_t total = tok_off[n_docs], ntiles = (total + a.tile - 1) / a.tile;
    for (int64_t p = 0; p < total; ++p)
        if (a.len_of(ids[p]) == 0) { a.raise(2, p); return done(); }  // (the lowest index)
    a.chunk_sum.assign((size_t)ntiles + 1, 0);
    if (!starts) {
        std::vector<Seg> runs((size_t)ntiles + 1, Seg{0u, 0ull});
        for (int64_t k = 0; k < ntiles; ++k) {
            const int64_t t = order[k];
            Seg s{0u, 0ull};
            for (int64_t p = t * a.tile; p < std::min(total, (t + 1) * a.tile); ++p) s = seg_op(s, Seg{a.bits[(size_t)p], (unsigned long long)a.len_of(ids[p])});
            runs[(size_t)t] = s;
        }
        Seg before{0u, 0ull};
        for (int64_t t = 0; t < ntiles; ++t) {
            a.chunk_sum[(size_t)t] = before.s;
            before = seg_op(before, runs[(size_t)t]);
        }
    }

    // ---- apply ------------------------------------------------------------------------------------------------------------------------
    std::vector<uint64_t> tile_cnt((size_t)ntiles + 1, 0);
    std::vector<uint32_t> local((size_t)total + 1, 0);
    std::vector<int64_t> s_tab((size_t)a.tab);
    std::vector<long long> s_wb((size_t)a.win), s_we((size_t)a.win), s_wc((size_t)a.win);
    const auto tok_key = [&](int64_t d) { return tok_off[d]; };
    const auto beg_key = [&](int64_t r) { return ranges[2 * r]; };
    for (int64_t kk = 0; kk < ntiles; ++kk) {
        const int64_t t = order[kk], t0 = t * a.tile, tlen = std::min(a.tile, total - t0);
        const int64_t nlanes = (tlen + a.per - 1) / a.per;
        // the lanes' first starts and last ends: the covered form scans the lanes' runs behind the tile's carry
        std::vector<unsigned long long> cur0((size_t)nlanes);
        long long edge0 = 0, edge1 = 0;
        if (!starts) {
            Seg before{0u, a.chunk_sum[(size_t)t]};
            for (int64_t l = 0; l < nlanes; ++l) {
                cur0[(size_t)l] = before.s;
                Seg mine{0u, 0ull};
                for (int64_t p = t0 + l * a.per; p < t0 + std::min(tlen, (l + 1) * a.per); ++p) mine = seg_op(mine, Seg{a.bits[(size_t)p], (unsigned long long)a.len_of(ids[p])});
                if (l == 0) edge0 = a.bits[(size_t)t0] ? 0ll : (long long)before.s;
                before = seg_op(before, mine);
                edge1 = (long long)before.s;
            }
        } else {
            edge0 = starts[t0];
            edge1 = starts[t0 + tlen - 1] + a.len_of(ids[t0 + tlen - 1]);
        }
        // the tile's documents
        const int64_t d0 = last_le(tok_key, 0, n_docs, t0);
        int64_t nd = 0;
        bool fits = false;
        for (int64_t c0 = 0; c0 < a.tab; c0 += a.tab_step) {
            int64_t c = 0;
            for (int64_t i = 0; i < a.tab_step; ++i) {
                const int64_t d = d0 + c0 + i;
                int64_t v = a.tile;
                if (d <= n_docs) v = std::min(a.tile, std::max<int64_t>(0, tok_off[d] - t0));
                s_tab[(size_t)(c0 + i)] = v;
                c += v < tlen;
            }
            nd += c;
            if (c < a.tab_step) { fits = true; break; }
        }
        const auto tab_key = [&](int64_t i) { return s_tab[(size_t)i]; };
        const int64_t d_last = fits ? d0 + last_le(tab_key, 0, nd, tlen - 1) : last_le(tok_key, d0, n_docs, t0 + tlen - 1);
        // the window
        const int64_t f0 = range_off[d0], f1 = range_off[d0 + 1], l0 = range_off[d_last], l1 = range_off[d_last + 1];
        const int64_t w0 = last_le(beg_key, f0, f1, edge0);
        const int64_t w1 = l1 > l0 ? last_le(beg_key, l0, l1, edge1) + 1 : l0;
        const bool staged = w1 - w0 <= a.win;
        ++kinds[2 * (fits ? 1 : 0) + (staged ? 1 : 0)];
        if (staged) {
            for (int64_t i = 0; i < w1 - w0; ++i) {
                const int64_t r = w0 + i;
                s_wb[(size_t)i] = ranges[2 * r];
                s_we[(size_t)i] = ranges[2 * r + 1];
                s_wc[(size_t)i] = a.cum[(size_t)r] + (long long)a.rchunks[(size_t)(r / a.chunk)];
            }
            if (w1 > w0 && w0 / a.chunk != (w1 - 1) / a.chunk) ++kinds[4];
        }
        // the walk, a lane at a time
        uint32_t tile_tr = 0;
        std::vector<uint8_t> tr_of((size_t)tlen, 0);
        uint64_t n_pa = 0;
        for (int64_t l = 0; l < nlanes; ++l) {
            const int64_t jb = l * a.per, nv = std::min(a.per, tlen - jb), p0 = t0 + jb;
            int64_t it = -1, d = -1, lo0 = 0, hi = 0, k = -1;
            long long kb = 0, ke = 0, kc = 0, base = 0, prev_e = 0, prev_g = 0;
            bool prev_in = false, have_prev = false;
            unsigned long long cur = starts ? 0ull : cur0[(size_t)l];
            const auto beg_at = [&](int64_t r) { return staged ? s_wb[(size_t)(r - w0)] : ranges[2 * r]; };
            const auto eval = [&](long long x, long long& g, bool& in) {
                if (k + 1 < hi && beg_at(k + 1) <= x) {
                    k = last_le(beg_at, k + 1, hi, x);
                    if (staged) { kb = s_wb[(size_t)(k - w0)]; ke = s_we[(size_t)(k - w0)]; kc = s_wc[(size_t)(k - w0)]; }
                    else { kb = ranges[2 * k]; ke = ranges[2 * k + 1]; kc = a.cum[(size_t)k] + (long long)a.rchunks[(size_t)(k / a.chunk)]; }
                }
                if (k < lo0) { g = base; in = false; return; }
                const long long off = x - kb, len = ke - kb;
                g = kc + (off < 0 ? 0 : off > len ? len : off);
                in = x >= kb && x < ke;
            };
            for (int64_t i = 0; i < nv; ++i) {
                const int64_t p = p0 + i;
                const bool head = a.bits[(size_t)p] != 0;
                if (i == 0 || head) {
                    if (fits) {
                        const int64_t x = jb + i;
                        if (it < 0) it = last_le(tab_key, 0, nd, x);
                        while (it + 1 < nd && s_tab[(size_t)(it + 1)] <= x) ++it;
                        d = d0 + it;
                    } else {
                        d = last_le(tok_key, d < 0 ? d0 : d, n_docs, p);
                    }
                    lo0 = range_off[d];
                    hi = range_off[d + 1];
                    if (staged) { lo0 = std::max(lo0, w0); hi = std::min(hi, w1); }
                    k = lo0 - 1;
                    base = 0;
                    if (lo0 < hi) base = staged ? s_wc[(size_t)(lo0 - w0)] : a.cum[(size_t)lo0] + (long long)a.rchunks[(size_t)(lo0 / a.chunk)];
                    have_prev = false;
                }
                const long long len = a.len_of(ids[p]);
                const long long s = starts ? starts[p] : head ? 0ll : (long long)cur;
                const long long e = s + len;
                cur = (unsigned long long)e;
                long long gs = prev_g, ge;
                bool in_s = prev_in, in_e;
                if (!have_prev || s != prev_e) eval(s, gs, in_s);
                eval(e, ge, in_e);
                prev_e = e; prev_g = ge; prev_in = in_e; have_prev = true;
                const long long m = ge - gs;
                const bool tr = rule == 0 ? m > 0 : rule == 1 ? m == len : in_s;
                tr_of[(size_t)(jb + i)] = tr;
                n_pa += m > 0 && m < len;
                if (!starts && (p + 1 == total || a.bits[(size_t)(p + 1)])) {
                    const int64_t r0 = range_off[d], r1 = range_off[d + 1];
                    if (r1 > r0 && ranges[2 * (r1 - 1) + 1] > e) a.lowest(RNG_H_BEYOND, a.first_beyond(r0, r1, e));
                }
            }
        }
        for (int64_t j = 0; j < tlen; ++j) {
            local[(size_t)(t0 + j)] = tile_tr;
            tile_tr += tr_of[(size_t)j];
            labels[t0 + j] = tr_of[(size_t)j] ? ids[t0 + j] : ignore;
            if (mask) mask[t0 + j] = tr_of[(size_t)j];
        }
        tile_cnt[(size_t)t] = tile_tr;
        a.head[LAB_H_TRAINED] += tile_tr;
        a.head[LAB_H_SPANS] += n_pa;
    }
    // ---- status, finish -------------------------------------------------------------------------------------------------------------------
    if (!starts && a.head[RNG_H_BEYOND]) {
        a.raise(1, (int64_t)(TOP - a.head[RNG_H_BEYOND]));
        return done();
    }
    uint64_t run = 0;
    for (int64_t t = 0; t < ntiles; ++t) {
        const uint64_t c = tile_cnt[(size_t)t];
        tile_cnt[(size_t)t] = run;
        run += c;
    }
    if (trained_off)
        for (int64_t d = 0; d <= n_docs; ++d) {
            const int64_t p = tok_off[d];
            trained_off[d] = p < total ? (int64_t)tile_cnt[(size_t)(p / a.tile)] + (int64_t)local[(size_t)p] : (int64_t)a.head[LAB_H_TRAINED];
        }
    counts[0] = (int64_t)a.head[LAB_H_TRAINED];
    counts[1] = (int64_t)a.head[LAB_H_SPANS];
    counts[2] = (int64_t)a.head[LAB_H_UNTERM];
    counts[3] = 0;
    return done();
}
