// Whole documents packed into rows by best-fit decreasing (td_pack.hip): the contract is in include/tokendagger_hip.h
// (TD_ROWS_BESTFIT, td_pack_rows).  The placement is sequential by nature, so it is planned on the host over RUNS of equal-length
// items (pack_plan_runs); every per-document and per-slot step runs on the device.  The workgroup size, the tile and the grid cap,
// and the device helpers shared with the other layouts, are in td_rows_common.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "td_rows_lab.h"

#include <vector>

namespace td {

constexpr int PACK_HDR = 8;           // int64 words of the header the host reads back (PackHdr)
constexpr int64_t PACK_RUNS_FIRST = 8192;  // runs read back with the header; more (S > 8192) take a second copy

// The header the items kernel and the run-length encode leave on the device (zeroed before the launch).
enum PackHdr { PH_FULL = 0, PH_REAL = 1, PH_CUT = 2, PH_ITEMS = 3, PH_ERR = 4, PH_ERR_DOC = 5, PH_RUNS = 6 };

// A run of `count` sorted items of length `len` placed into one row: slots [slot, slot + count * len) of row `row`.  first_item
// indexes the sorted remainder items, first_seg the segments.
struct PackPlacement {
    int64_t len, row, slot, count, first_item, first_seg;
};

// The host plan: rows 0 .. full - 1 hold one full chunk each (segment f = row f); the mixed rows full .. rows - 1 follow.
struct PackPlan {
    int64_t S = 0, full = 0, rows = 0, segs = 0, real = 0;
    std::vector<PackPlacement> pl;
    std::vector<int64_t> fill;      // [mixed rows] real slots
    std::vector<int64_t> seg0;      // [mixed rows + 1] first segment of the row; seg0[mixed rows] = segs
};

// Best-fit decreasing over runs: run r has counts[r] items of length lens[r] (1 <= len < S, lengths strictly decreasing).  A
// row that takes one item of a run keeps taking them until its free count drops below the length, so it takes
// min(k, free / len) at once.  O((runs + row visits) * log).
void pack_plan_runs(int64_t S, int64_t full, int64_t real, const int64_t* lens, const int64_t* counts, int64_t n_runs, PackPlan& out);

struct PackArgs {
    const int32_t* ids;       // [n_tokens]
    int64_t n_tokens;
    const int64_t* tok_off;   // [n_docs + 1]
    int64_t n_docs;
    int64_t S;
    int b, e, truncate;
    int32_t bos, eos, pad;
    // items kernel
    uint32_t* key;            // [n_docs] S - remainder (S: no remainder item): an ascending stable sort is (length desc, doc asc)
    uint32_t* val;            // [n_docs] the document
    int64_t* full;            // [n_docs] full chunks of the document
    long long* hdr;           // [PACK_HDR] (PackHdr)
    // segments kernel
    const int64_t* pref;      // [n_docs] exclusive scan of full
    const uint32_t* sorted_doc;  // [n_docs] documents in item order
    const PackPlacement* pl;  // [n_pl]
    int64_t n_pl;
    const int64_t* fill;      // [n_mixed]
    const int64_t* seg0;      // [n_mixed + 1]
    int64_t full_rows, n_mixed, n_items, rows, segs;
    int64_t* seg_start;       // [segs + 1] flat slot of the segment's start; seg_start[segs] = rows * S
    int64_t* seg_doc;         // [segs] document or -1
    int64_t* seg_q0;          // [segs] the segment's first slot inside its document's slot sequence
    // outputs (any but out may be null)
    int32_t* out;             // [rows * S]
    int32_t* pos;             // [rows * S]
    int32_t* cu;              // [segs + 1]
    int32_t* lengths;         // [rows]
    int64_t* docs;            // [segs]
};

// What the host fills and the launchers take: PackArgs, and behind it the label stream of the pair form (lab.src null: one stream).
// The one-stream kernels get the PackArgs slice alone, so that their arguments are what they were without the pair form.
struct PackLabArgs : PackArgs {
    LabArgs lab;
};

// td_pack_items: per document n_d, its full chunks and remainder, the offsets' checks and the totals into hdr.
hipError_t launch_pack_items(const PackArgs& a, hipStream_t stream);
// The scan of full chunks, the stable sort of (key, document) and the run-length encode of the sorted keys (unique keys at
// runs_key, counts at runs_cnt, the number of runs at hdr[PH_RUNS]).  temp: nullptr to ask for temp_bytes.
hipError_t pack_sort_runs(void* temp, size_t& temp_bytes, const PackArgs& a, uint32_t* key_out, uint32_t* val_out, int64_t* pref,
                          uint32_t* runs_key, uint32_t* runs_cnt, hipStream_t stream);
// td_pack_segments then td_pack_slots.
hipError_t launch_pack_outputs(const PackLabArgs& a, hipStream_t stream);

}  // namespace td
