// Per-document duplicate-line and duplicate-paragraph statistics (td_repetition.hip), for the host library: the kernels' arguments
// (td_repetition_args.h) and their launch.
#pragma once
#include <hip/hip_runtime_api.h>

#include "td_repetition_args.h"

namespace td {

// td_rp_docs, td_rp_summary, td_rp_prefix, td_rp_reset, td_rp_tiles and td_rp_finish on `stream`: a.stats ([n_docs][RP_COLS]) and a.totals
// (may be null).  a.head is zeroed by the caller on the same stream; a.carry has room for two elements a tile of the text, a.table for
// rp_slots(a.max_units) words, 16-byte aligned.  Nothing is written when the offsets are bad or the text has more units than a.max_units.
hipError_t launch_repetition(const RpArgs& a, hipStream_t stream);

}  // namespace td
