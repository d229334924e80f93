// Address masking (td_mask.hip), for the host library: the kernels' arguments (td_mask_args.h) and their launch.
#pragma once
#include <hip/hip_runtime_api.h>

#include "td_mask_args.h"

namespace td {

// RW_RUN_MEASURE: td_ma_docs, td_ma_reset, td_ma_tiles<measure>, td_ma_scan and td_ma_sums on `stream`: a.stats, a.totals (may be null),
// a.counts, a word a tile in a.dirty, the tiles' places in a.tile_base (a word a tile and one more), TD_E_CAPACITY against
// a.out_capacity, and in a.out_doc_off (not null) the entries of the documents that start at the text's end; a.out is not touched.
// a.head is zeroed by the caller on the same stream.
// RW_RUN_WRITE: td_ma_tiles<write>: a.out (null: not written) and the rest of a.out_doc_off from a.dirty and a.tile_base; nothing when
// the output did not fit.
hipError_t launch_mask(const MaArgs& a, hipStream_t stream, int phases);

}  // namespace td
