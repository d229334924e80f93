// Line filtering (td_linefilter.hip), for the host library: the kernels' arguments (td_linefilter_args.h) and their launch.
#pragma once
#include <hip/hip_runtime_api.h>

#include "td_linefilter_args.h"

namespace td {

// RW_RUN_MEASURE: td_lf_docs, td_lf_reset, td_lf_carry, td_lf_prefix, td_lf_tiles<measure>, td_lf_scan and td_lf_totals on `stream`:
// a.stats, a.totals (may be null), a.counts, the windows' kept bytes in a.masks (a word of 16 bits a window of the text and 256 more),
// the tiles' places in a.tile_base (a word a tile and one more), TD_E_CAPACITY against a.out_capacity, and in a.out_doc_off (not null)
// the entries of the documents that start at the text's end; a.out is not touched.  a.elems: an element a tile, a.carry: two pieces a
// tile.  a.head is zeroed by the caller on the same stream.
// RW_RUN_WRITE: td_lf_tiles<write>: a.out (null: not written) and the rest of a.out_doc_off from a.masks and a.tile_base; nothing when
// the output did not fit.
hipError_t launch_linefilter(const LfArgs& a, hipStream_t stream, int phases);

}  // namespace td
