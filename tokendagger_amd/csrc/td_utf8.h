// UTF-8 validation and repair (td_utf8.hip), for the host library: the kernels' arguments (td_utf8_args.h) and their launches.
#pragma once
#include <hip/hip_runtime_api.h>

#include "td_utf8_args.h"

namespace td {

// td_utf8_docs, td_utf8_prepare, td_utf8_check and td_utf8_sums on `stream`: a.flags, a.first_bad (may be null) and a.counts (counts[1]
// alone is counted).  a.head is zeroed by the caller on the same stream; a.dirty and a.n_bad are null.  Nothing is written when the
// offsets are bad.
hipError_t launch_utf8_check(const U8Args& a, hipStream_t stream);

// RW_RUN_MEASURE: td_utf8_docs, td_utf8_prepare, td_utf8_tiles<measure>, td_utf8_scan and td_utf8_sums on `stream`: a.flags (not null),
// a.first_bad and a.n_bad (may be null), a.counts, the tiles' places in a.tile_base (room for a word a tile of the text and one more),
// TD_E_CAPACITY against a.out_capacity, and in a.out_doc_off the entries of the documents that start at the text's end; a.out is not
// touched.  a.dirty (a byte a window of the text and one more) and a.head are zeroed by the caller on the same stream.
// RW_RUN_WRITE: td_utf8_tiles<write>: a.out and the rest of a.out_doc_off from what the measure phase left in a.tile_base, a.dirty and
// a.head (a phase of its own so that a host form can size a.out from counts[0] in between); nothing when the output did not fit.
hipError_t launch_utf8(const U8Args& a, hipStream_t stream, int phases);

}  // namespace td
