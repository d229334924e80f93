// CPU model of td_utf8.hip's decomposition over tokendagger_amd/csrc/td_utf8_args.h (the unit rule, the window screen, the documents'
// edges, the check window and the lane walk are the kernels' own): windows of 16 bytes at 16 g - shift (shift: the base pointer's
// misalignment), a lane a window, tile / 16 windows a tile; the documents' edges by a lane a document (the check reports them, the repair
// marks their windows); the check by windows, the screen on the windows that have four bytes of the text on either side, the walk
// where it is set; the measure walk (a lane has the bytes of its window), the windows that are copies, the tile's table of documents
// from the last one that starts in front of the tile, clamped as the kernel clamps it, the scan over the tiles, the size walk and the
// write walk, a tile of copied windows as one copy.  The tile size is an argument.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../tokendagger_amd/csrc/td_utf8_args.h"

using namespace td;

namespace {

uint32_t dword(const uint8_t* p) {
    uint32_t w;
    memcpy(&w, p, 4);
    return w;
}

bool ascii(const uint8_t* p) {
    for (int i = 0; i < 16; ++i)
        if (p[i] & 0x80) return false;
    return true;
}

bool suspect_at(const uint8_t* text, int64_t b) {
    const uint32_t s[6] = {dword(text + b - 4), dword(text + b), dword(text + b + 4), dword(text + b + 8), dword(text + b + 12), dword(text + b + 16)};
    return u8_window_suspect(s);
}

struct Add {
    void operator()(unsigned long long* p, unsigned long long n) const { *p += n; }
};
struct Lower {
    void operator()(unsigned long long* p, unsigned long long v) const { *p = std::min(*p, v); }
};

}  // namespace

// The screen alone, for the test that compares it with the walker: s[24] = four bytes in front, the window, four bytes behind.
extern "C" int utf8_screen(const uint8_t* s) {
    const uint32_t w[6] = {dword(s), dword(s + 4), dword(s + 8), dword(s + 12), dword(s + 16), dword(s + 20)};
    return u8_window_suspect(w);
}

// stats[6]: tiles, windows copied without a walk, tiles that were one copy, windows the screen was asked about, windows the check
// walked, the most documents a tile's table held.
// Returns 0, 1 for bad arguments, 5 when the output does not fit (counts[0] is set, out and out_off are not written).
extern "C" int utf8_model(const uint8_t* text, const int64_t* off, int64_t n_docs, int policy, int tile, int shift, uint8_t* out, int64_t cap,
                          int64_t* out_off, uint8_t* check_flags, int64_t* check_first, uint8_t* flags, int64_t* first_bad, int64_t* n_bad,
                          int64_t* counts, int64_t* stats) {
    if (tile < 64 || tile % 16 || shift < 0 || shift > 15 || n_docs < 0) return 1;
    const int64_t total = off[n_docs];
    memset(stats, 0, 6 * sizeof(int64_t));
    const int64_t nwin = u8_windows(total, shift);
    std::vector<uint8_t> dirty((size_t)nwin + 1, 0);
    U8Args a;
    memset(&a, 0, sizeof a);
    a.text = text;
    a.n_bytes = total;
    a.doc_off = off;
    a.n_docs = n_docs;
    a.policy = policy;
    a.out = out;
    a.out_capacity = cap;
    a.out_doc_off = out_off;
    // ---- the check: prepare (the documents' edges), then the windows -----------------------------------------------------------------
    a.flags = check_flags;
    a.first_bad = (unsigned long long*)check_first;
    for (int64_t d = 0; d < n_docs; ++d) {
        unsigned long long first = ~0ull;
        bool ill = false;
        u8_doc_edges(text, off[d], off[d + 1], total, [&](int64_t p, int) {
            ill = true;
            first = std::min(first, (unsigned long long)(p - off[d]));
        });
        check_flags[d] = ill;
        check_first[d] = (int64_t)first;
    }
    for (int64_t g = 0; g < nwin; ++g) {
        const int64_t b0 = g * 16 - shift, b = std::max<int64_t>(b0, 0), we = std::min(b0 + 16, total);
        if (b0 >= 4 && b0 + 20 <= total) {
            if (ascii(text + b)) continue;
            ++stats[3];
            if (!suspect_at(text, b)) continue;
        }
        ++stats[4];
        int64_t D = -1, ds = 0, de = 0;
        u8_check_window(a, b, we, D, ds, de, [&](int64_t p) { return (int64_t)(std::upper_bound(off, off + n_docs, p) - off) - 1; }, Lower{});
    }
    // ---- the repair: prepare ----------------------------------------------------------------------------------------------------
    a.flags = flags;
    a.first_bad = (unsigned long long*)first_bad;
    a.n_bad = (unsigned long long*)n_bad;
    for (int64_t d = 0; d < n_docs; ++d) {
        flags[d] = 0;
        first_bad[d] = -1;
        n_bad[d] = 0;
        u8_doc_edges(text, off[d], off[d + 1], total, [&](int64_t p, int len) {
            dirty[(size_t)u8_window_of(p, shift)] = 1;
            dirty[(size_t)u8_window_of(p + len - 1, shift)] = 1;
        });
    }
    const int lanes = tile / 16;
    const int32_t off_lo = -8, off_hi = tile + 8;
    const int64_t ntiles = total > 0 ? (total + shift + tile - 1) / tile : 0;
    std::vector<unsigned long long> tile_base((size_t)ntiles + 1, 0);
    U8LaneStats st = {0, 0};
    const auto walk = [&](bool write) {
        for (int64_t t = 0; t < ntiles; ++t) {
            const int64_t t0 = std::max<int64_t>(t * tile - shift, 0), s1 = std::min<int64_t>((t + 1) * tile - shift, total);
            // the tile's table: from the last document that starts in front of t0
            const int64_t kb = t0 > 0 ? (int64_t)(std::upper_bound(off, off + n_docs, t0 - 1) - off) - 1 : 0;
            const int64_t nk = (int64_t)(std::upper_bound(off, off + n_docs, s1 - 1) - off) - kb;
            stats[5] = std::max(stats[5], nk);
            const auto rel = [&](int64_t i) { return (int64_t)std::min<int64_t>(std::max<int64_t>(off[kb + i] - t0, off_lo), off_hi); };
            const auto ub = [&](int64_t x) {
                int64_t lo = 0, hi = nk;
                while (lo < hi) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (rel(mid) > x - t0) hi = mid;
                    else lo = mid + 1;
                }
                return kb + lo;
            };
            std::vector<int64_t> n((size_t)lanes, 0);
            std::vector<char> fast((size_t)lanes, 1);
            bool all_fast = true;
            for (int l = 0; l < lanes; ++l) {
                const int64_t b0 = t * tile + 16 * l - shift, b = std::max<int64_t>(b0, 0), we = std::min(b0 + 16, total);
                if (b >= we) continue;
                fast[(size_t)l] = b0 >= 4 && b0 + 20 <= total && (ascii(text + b) || (!suspect_at(text, b) && !dirty[(size_t)(t * lanes + l)]));
                all_fast = all_fast && fast[(size_t)l];
                if (fast[(size_t)l]) {
                    n[(size_t)l] = we - b;
                    if (!write) ++stats[1];
                } else if (!write) {
                    n[(size_t)l] = u8_lane<U8_MEASURE>(a, b, we, ub, 0, st, Add{}, Lower{});
                } else {
                    n[(size_t)l] = u8_lane<U8_SIZE>(a, b, we, ub, 0, st, Add{}, Lower{});
                }
            }
            if (!write) {
                for (int l = 0; l < lanes; ++l) tile_base[(size_t)t] += (unsigned long long)n[(size_t)l];
                continue;
            }
            stats[2] += all_fast;
            if (all_fast) memcpy(out + tile_base[(size_t)t], text + t0, (size_t)(s1 - t0));
            int64_t opos = (int64_t)tile_base[(size_t)t];
            for (int l = 0; l < lanes; ++l) {
                const int64_t b0 = t * tile + 16 * l - shift, b = std::max<int64_t>(b0, 0), we = std::min(b0 + 16, total);
                if (b >= we) continue;
                if (fast[(size_t)l]) {
                    if (!all_fast) memcpy(out + opos, text + b, (size_t)(we - b));
                    for (int64_t k = ub(b - 1); k <= n_docs && off[k] < we; ++k) out_off[k] = opos + (off[k] - b);
                } else if (u8_lane<U8_WRITE>(a, b, we, ub, opos, st, Add{}, Lower{}) != n[(size_t)l]) {
                    return 2;
                }
                opos += n[(size_t)l];
            }
        }
        return 0;
    };
    walk(false);
    stats[0] = ntiles;
    // ---- scan and sums ----------------------------------------------------------------------------------------------------------
    unsigned long long run = 0;
    for (int64_t t = 0; t < ntiles; ++t) {
        const unsigned long long v = tile_base[(size_t)t];
        tile_base[(size_t)t] = run;
        run += v;
    }
    memset(counts, 0, U8_C_WORDS * sizeof(int64_t));
    counts[U8_C_BYTES] = (int64_t)run;
    counts[U8_C_SUBPARTS] = st.subparts;
    counts[U8_C_SUB_BYTES] = st.sub_bytes;
    for (int64_t d = 0; d < n_docs; ++d) {
        counts[U8_C_DOCS] += flags[d] != 0;
        if (off[d] < off[d + 1]) {
            counts[U8_C_BEGIN_CONT] += u8_is_cont(text[off[d]]);
            counts[U8_C_END_LEAD] += u8_ends_cut(text, off[d], off[d + 1]);
        }
    }
    if ((int64_t)run > cap) return 5;
    for (int64_t d = n_docs; d >= 0 && off[d] == total; --d) out_off[d] = (int64_t)run;
    // ---- write ------------------------------------------------------------------------------------------------------------------
    return walk(true);
}
