// CPU model of td_nfc.hip's decomposition over tokendagger_amd/csrc/td_nfc_args.h (the lookup, the decoder, the quick check, the segment
// scan, the normaliser, the check window and the lane walk are the kernels' own): windows of 16 bytes at 16 g - shift (shift: the base
// pointer's misalignment), a lane a window, tile / 16 windows a tile; the check by windows with its look-back; the measure walk (a lane
// owns the segments that start in its window), the windows that are proven by their bytes alone, the tile's table of documents from
// the last one that starts in front of the tile, clamped as the kernel clamps it, the scan over the tiles, the size walk and the write
// walk, a tile of proven windows as one copy.  The tile size is an argument.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../tokendagger_amd/csrc/td_nfc_args.h"

using namespace td;

namespace {

#define TD_NFC_TABLE(type, name, n) const type name[n]
#include "../../tokendagger_amd/csrc/generated/unicode_nfc.inc"
#undef TD_NFC_TABLE

const NfcTables T{td_nfc_stage1, td_nfc_stage2, td_nfc_dec_key, td_nfc_dec_off, td_nfc_dec_cps, td_nfc_pair_a, td_nfc_pair_b, td_nfc_pair_c};

bool hits(const uint8_t* p, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (p[i] >= NFC_LEAD_MIN) return true;
    return false;
}

}  // namespace

// stats[6]: tiles, windows proven by their bytes alone, tiles that were one copy, windows that own nothing, windows the check decoded
// in, the most documents a tile's table held.
// Returns 0, 1 for bad arguments, 5 when the output does not fit (counts is complete, out and out_off are not written).
extern "C" int nfc_model(const uint8_t* text, const int64_t* off, int64_t n_docs, int tile, int shift, uint8_t* out, int64_t cap,
                         int64_t* out_off, uint8_t* check_flags, uint8_t* flags, uint8_t* changed, int64_t* counts, int64_t* stats) {
    if (tile < 64 || tile % 16 || shift < 0 || shift > 15 || n_docs < 0) return 1;
    const int64_t total = off[n_docs];
    memset(stats, 0, 6 * sizeof(int64_t));
    NfcArgs a;
    memset(&a, 0, sizeof a);
    a.text = text;
    a.n_bytes = total;
    a.doc_off = off;
    a.n_docs = n_docs;
    a.out = out;
    a.out_capacity = cap;
    a.out_doc_off = out_off;
    unsigned long long c[NFC_C_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    // ---- the check -----------------------------------------------------------------------------------------------------------------
    a.flags = check_flags;
    for (int64_t d = 0; d < n_docs; ++d) check_flags[d] = 0;
    const int64_t nwin = (total + shift + 15) >> 4;
    for (int64_t g = 0; g < nwin; ++g) {
        const int64_t b0 = g * 16 - shift, b = std::max<int64_t>(b0, 0), we = std::min(b0 + 16, total);
        if (b >= we || !hits(text + b, we - b)) continue;
        ++stats[4];
        int64_t D = -1, ds = 0, de = 0;  // (a lane that meets a second window has its document of the first: any state must do)
        nfc_check_window(a, T, b, we, D, ds, de, [&](int64_t p) { return (int64_t)(std::upper_bound(off, off + n_docs, p) - off) - 1; });
    }
    // ---- measure ------------------------------------------------------------------------------------------------------------------
    a.flags = flags;
    a.changed = changed;
    for (int64_t d = 0; d < n_docs; ++d) flags[d] = changed[d] = 0;
    const int lanes = tile / 16;
    const int32_t off_lo = -8, off_hi = tile + 8;
    const int64_t ntiles = total > 0 ? (total + shift + tile - 1) / tile : 0;
    std::vector<unsigned long long> tile_base((size_t)ntiles + 1, 0);
    NfcLaneStats st = {0, 0, 0, 0};
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
                if (b >= we) {
                    if (!write) ++stats[3];
                    continue;
                }
                fast[(size_t)l] = b0 >= 0 && b0 + 16 <= total && !hits(text + b, 16) && (text[b] & 0xC0) != 0x80 &&
                                  (we == total || ((text[we] & 0xC0) != 0x80 && text[we] < NFC_LEAD_MIN));
                all_fast = all_fast && fast[(size_t)l];
                bool plain = fast[(size_t)l];  // ASCII alone: MEASURE walks every other window for counts[5] and counts[6]
                for (int64_t i = b; plain && i < we; ++i) plain = text[i] < 0x80;
                if (write ? (bool)fast[(size_t)l] : plain) {
                    n[(size_t)l] = we - b;
                    if (!write) {
                        ++stats[1];
                        st.longest = std::max<uint32_t>(st.longest, 1);
                    }
                } else if (!write) {
                    n[(size_t)l] = nfc_lane<NFC_MEASURE>(a, T, b, we, total, ub, 0, st);
                } else {
                    n[(size_t)l] = nfc_lane<NFC_SIZE>(a, T, b, we, total, ub, 0, st);
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
                } else if (nfc_lane<NFC_WRITE>(a, T, b, we, total, ub, opos, st) != n[(size_t)l]) {
                    return 2;
                }
                opos += n[(size_t)l];
            }
        }
        return 0;
    };
    walk(false);
    stats[0] = ntiles;
    // ---- scan -------------------------------------------------------------------------------------------------------------------
    unsigned long long run = 0;
    for (int64_t t = 0; t < ntiles; ++t) {
        const unsigned long long v = tile_base[(size_t)t];
        tile_base[(size_t)t] = run;
        run += v;
    }
    c[NFC_C_BYTES] = run;
    c[NFC_C_SEGMENTS] = st.segments;
    c[NFC_C_CPS] = st.cps;
    c[NFC_C_OPAQUE] = st.opaque;
    c[NFC_C_LONGEST] = st.longest;
    for (int64_t d = 0; d < n_docs; ++d) {
        c[NFC_C_UNPROVEN] += flags[d] != 0;
        c[NFC_C_CHANGED] += changed[d] != 0;
    }
    for (int i = 0; i < NFC_C_WORDS; ++i) counts[i] = (int64_t)c[i];
    if ((int64_t)run > cap) return 5;
    for (int64_t d = n_docs; d >= 0 && off[d] == total; --d) out_off[d] = (int64_t)run;
    // ---- write ------------------------------------------------------------------------------------------------------------------
    return walk(true);
}
