// Per-document text statistics (td_textstats.hip), for the host library: the kernels' arguments (td_textstats_args.h) and their launch.
#pragma once
#include <hip/hip_runtime_api.h>

#include "td_textstats_args.h"

namespace td {

// td_ts_docs, td_ts_reset, under TS_RUNS td_ts_carry and td_ts_prefix, td_ts_tiles and td_ts_totals on `stream`: a.stats
// ([n_docs][TS_COLS]) and a.totals (may be null).  a.head is zeroed by the caller on the same stream; a.carry has room for four words a
// tile of the text under TS_RUNS.  Nothing is written when the offsets are bad.
hipError_t launch_textstats(const TsArgs& a, hipStream_t stream);

}  // namespace td
