// Loss labels for marked id spans (td_labels.hip, td_api_labels.cpp): what the kernels, the host library and the CPU model
// (tests/twin/labels_model.cpp) share.  Compiled for host and device, like td_common.h.
//
// The rule (the contract, include/tokendagger_hip.h): per document [a, z) an OPEN event at q when some opener of length k has
// ids[q-k+1 .. q] == opener with q-k+1 >= a, a CLOSE event at q when ids[q] is a closer; inside(i) = the last event in [a, i)
// is an open event; trained(i) = inside(i) && (!close(i) || TRAIN_CLOSE).  No opener contains a closer, so no position is
// both.
//
// As a scan: every position is one of NONE, IN (open event) or OUT (close event, or the reset in front of a document's first
// id), the operator is "rightmost non-NONE" (lab_combine), and inside(i) is the exclusive scan at i.  A position that starts
// a document AND carries an event of its own is the reset followed by the event: lab_event gives the event.  lab_step is one
// step of the sequential walk and what every implementation counts by.
#pragma once
#include <stdint.h>

#include "td_common.h"

namespace td {

constexpr int LAB_HALO = TD_LABELS_MAX_OPEN_LEN - 1;  // ids in front of a position an opener match may read

struct LabSpec {  // td_labels_spec, checked and narrowed (td_api_labels.cpp); a kernel argument
    int32_t n_open, n_close;
    int32_t ignore;
    int32_t train_close;
    int32_t open_len[TD_LABELS_MAX_OPEN];
    int32_t open_ids[TD_LABELS_MAX_OPEN][TD_LABELS_MAX_OPEN_LEN];
    int32_t close_ids[TD_LABELS_MAX_CLOSE];
};

enum : uint32_t { LAB_NONE = 0, LAB_IN = 1, LAB_OUT = 2 };

TD_HD uint32_t lab_combine(uint32_t left, uint32_t right) { return right != LAB_NONE ? right : left; }

TD_HD bool lab_is_close(const LabSpec& s, int32_t id) {
    bool c = false;
    for (int k = 0; k < s.n_close; ++k) c |= s.close_ids[k] == id;
    return c;
}

// The openers whose LAST id is `id`, one bit each: the common case is this one compare an opener and no match.
TD_HD uint32_t lab_last_mask(const LabSpec& s, int32_t id) {
    uint32_t m = 0;
    for (int o = 0; o < s.n_open; ++o) m |= (s.open_ids[o][s.open_len[o] - 1] == id) ? 1u << o : 0u;
    return m;
}

// Does one of the openers `cand` (lab_last_mask of ids[q]) end at q?  get(p) = ids[p]; avail = min(q - a + 1, 8) ids of q's
// document end at q: an opener longer than that would reach across the document start.
template <class Get>
TD_HD bool lab_open_match(const LabSpec& s, uint32_t cand, const Get& get, int64_t q, int avail) {
    for (int o = 0; o < s.n_open; ++o) {
        if (!((cand >> o) & 1u)) continue;
        const int k = s.open_len[o];
        if (k > avail) continue;
        bool same = true;
        for (int j = 1; j < k; ++j) same = same && get(q - j) == s.open_ids[o][k - 1 - j];
        if (same) return true;
    }
    return false;
}

TD_HD uint32_t lab_event(bool doc, bool open, bool close) { return open ? LAB_IN : (close || doc) ? LAB_OUT : LAB_NONE; }

// One position of the walk.  inside: the state in front of the position, of the document before it when `doc` (a document starts
// here).  Adds to the three counts, sets trained, returns the state behind the position.
TD_HD uint32_t lab_step(uint32_t inside, bool doc, bool open, bool close, bool train_close, bool& trained, uint32_t& n_trained,
                        uint32_t& n_spans, uint32_t& n_unterminated) {
    if (doc) {
        n_unterminated += inside;
        inside = 0;
    }
    trained = inside && (!close || train_close);
    n_trained += trained ? 1u : 0u;
    if (open) {
        n_spans += inside ? 0u : 1u;
        inside = 1;
    } else if (close) {
        inside = 0;
    }
    return inside;
}

}  // namespace td
