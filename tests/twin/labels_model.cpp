// CPU model of td_labels.hip's decomposition over the shared header (tokendagger_amd/csrc/td_labels.h): the same element
// classification, combine operator and walk step, with the tile size a parameter and the tiles resolved in the order the
// caller gives (every phase's tiles are independent of each other, as the workgroups of a launch are).
//
//   phase 0  the starts of the non-empty documents as a bitmap
//   phase 1  every tile's last event, looked for from the tile's end backwards
//   phase 2  the exclusive "rightmost non-NONE" scan over the tiles: the state in front of each, and at the very end
//   phase 3  every tile: events, the walk with the state known, labels / mask, the tile's counts and per-position prefixes
//   phase 4  the exclusive sum of the tiles' trained ids
//   phase 5  trained_offsets per document boundary, counts
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../tokendagger_amd/csrc/td_labels.h"

using namespace td;

namespace {

// ids of q's document that end at q, at most 8 (the kernel reads this off the bitmap words: the same eight bits)
int avail_at(const std::vector<uint8_t>& doc, int64_t q) {
    for (int j = 0; j < 8; ++j) {
        if (q - j < 0) return j;
        if (doc[(size_t)(q - j)]) return j + 1;
    }
    return 8;
}

struct Ev { bool doc, open, close; };

Ev classify(const LabSpec& s, const int32_t* ids, const std::vector<uint8_t>& doc, int64_t q) {
    Ev e{doc[(size_t)q] != 0, false, lab_is_close(s, ids[q])};
    const uint32_t cand = lab_last_mask(s, ids[q]);
    if (cand) e.open = lab_open_match(s, cand, [&](int64_t p) { return ids[p]; }, q, avail_at(doc, q));
    return e;
}

}  // namespace

extern "C" int labels_model(const int32_t* ids, const int64_t* tok_off, int64_t n_docs, const LabSpec* spec, int64_t tile,
                            const int64_t* order, int32_t* labels, uint8_t* mask, int64_t* trained_off, int64_t* counts) {
    const LabSpec& s = *spec;
    const int64_t total = tok_off[n_docs], ntiles = (total + tile - 1) / tile;
    std::vector<uint8_t> doc((size_t)total + 1, 0);
    for (int64_t d = 0; d < n_docs; ++d)
        if (tok_off[d + 1] > tok_off[d]) doc[(size_t)tok_off[d]] = 1;
    std::vector<uint32_t> tiles((size_t)ntiles + 1, LAB_NONE);
    for (int64_t k = 0; k < ntiles; ++k) {
        const int64_t t = order[k], t0 = t * tile, t1 = t0 + tile < total ? t0 + tile : total;
        uint32_t last = LAB_NONE;
        for (int64_t q = t1 - 1; q >= t0 && last == LAB_NONE; --q) {
            const Ev e = classify(s, ids, doc, q);
            last = lab_event(e.doc, e.open, e.close);
        }
        tiles[(size_t)t] = last;
    }
    uint32_t carry = LAB_NONE;
    for (int64_t t = 0; t < ntiles; ++t) {
        const uint32_t ev = tiles[(size_t)t];
        tiles[(size_t)t] = carry == LAB_IN ? 1u : 0u;
        carry = lab_combine(carry, ev);
    }
    const uint32_t end_inside = carry == LAB_IN ? 1u : 0u;
    std::vector<uint64_t> tile_cnt((size_t)ntiles + 1, 0);
    std::vector<uint32_t> local((size_t)total + 1, 0);  // trained ids of the position's tile in front of it
    uint64_t n_trained = 0, n_spans = 0, n_unterm = 0;
    for (int64_t k = ntiles - 1; k >= 0; --k) {
        const int64_t t = order[k], t0 = t * tile, t1 = t0 + tile < total ? t0 + tile : total;
        uint32_t inside = tiles[(size_t)t], tr = 0, sp = 0, un = 0;
        for (int64_t q = t0; q < t1; ++q) {
            const Ev e = classify(s, ids, doc, q);
            local[(size_t)q] = tr;
            bool trained;
            inside = lab_step(inside, e.doc, e.open, e.close, s.train_close != 0, trained, tr, sp, un);
            labels[q] = trained ? ids[q] : s.ignore;
            if (mask) mask[q] = trained ? 1 : 0;
        }
        tile_cnt[(size_t)t] = tr;
        n_trained += tr;
        n_spans += sp;
        n_unterm += un;
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
            int64_t v = (int64_t)n_trained;
            if (p < total) v = (int64_t)tile_cnt[(size_t)(p / tile)] + (int64_t)local[(size_t)p];
            trained_off[d] = v;
        }
    counts[0] = (int64_t)n_trained;
    counts[1] = (int64_t)n_spans;
    counts[2] = (int64_t)(n_unterm + end_inside);
    counts[3] = 0;
    return 0;
}
