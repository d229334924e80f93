// Loss labels (td_labels.hip): the kernels' arguments and their launch, for the host library.  The rule and the pieces shared
// with the CPU model are in td_labels.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "td_labels.h"

namespace td {

constexpr int LAB_TILE = 4096;     // ids a workgroup labels per tile (sixteen a lane)
constexpr int LAB_THREADS = 256;
constexpr int LAB_PER = LAB_TILE / LAB_THREADS;
enum { LAB_H_BAD = 0, LAB_H_TRAINED, LAB_H_SPANS, LAB_H_UNTERM, LAB_H_END, LAB_HEAD_WORDS = 8 };  // LabelArgs::head

struct LabelArgs {
    const int32_t* ids;          // [n_tokens]
    int64_t n_tokens;            // ids the buffer holds: tok_off[n_docs] above it is an error, no id at or above it is read
    const int64_t* tok_off;      // [n_docs + 1]
    int64_t n_docs;
    LabSpec spec;
    int32_t* labels;             // [n_tokens]
    uint8_t* mask;               // [n_tokens] or null
    int64_t* trained_off;        // [n_docs + 1] or null
    long long* counts;           // [4] trained ids, spans, unterminated documents, 0
    // workspace
    unsigned long long* head;    // [LAB_HEAD_WORDS], zeroed before the launch: bad offsets, the three counts, the state at the end
    uint32_t* bits;              // [n_tokens / 32 + 2], zeroed before the launch: a non-empty document starts at this id
    uint8_t* tiles;              // [tiles, rounded up to 16 * 1024]: a tile's last event, then the state in front of the tile
    unsigned long long* tile_cnt;  // [tiles rounded likewise] (trained_off only): a tile's trained ids, then those in front of it
    uint32_t* aux;               // [tiles * LAB_THREADS] (trained_off only): a lane's trained ids in front of it in its tile << 16 | trained bits
    int* err;
    long long* err_pos;
};

int64_t labels_tiles(int64_t n_tokens);         // tiles of a call (at least one)
int64_t labels_tiles_rounded(int64_t n_tokens);  // entries of LabelArgs::tiles / tile_cnt
// td_lab_docs, td_lab_tiles, td_lab_carry, td_lab_apply, [td_lab_count_carry,] td_lab_finish
hipError_t launch_labels(const LabelArgs& a, hipStream_t stream);
// Its last two alone, for another labelling pass (td_ranges.hip) that left td_lab_apply's results: head (LAB_H_TRAINED, LAB_H_SPANS,
// LAB_H_UNTERM as counts[0 .. 2]; LAB_H_BAD: nothing is written), and with trained_off tile_cnt and aux.  Reads tok_off, n_docs,
// counts, trained_off and those.
hipError_t launch_labels_finish(const LabelArgs& a, hipStream_t stream);

}  // namespace td
