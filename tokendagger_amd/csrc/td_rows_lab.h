// The label stream of the pair form of the row layouts (td_*_rows_labeled*, include/tokendagger_hip.h: td_rows_labels): what
// RowsLabArgs, PackLabArgs and WindowLabArgs add to the one-stream arguments; all zero in a one-stream call.
#pragma once
#include <stdint.h>

namespace td {

struct LabArgs {
    const int32_t* src;       // [n_tokens], index-aligned with ids; null: no label stream
    int32_t* dst;             // [rows_cap * S], placed like out
    int32_t bos, eos, pad;    // what dst holds where out holds the inserted BOS / EOS / a pad slot
    int mask_overlap;         // WINDOWS: body slot j < overlap of a window k > 0 holds pad
};

}  // namespace td
