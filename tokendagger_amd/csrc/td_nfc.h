// Unicode NFC normalisation (td_nfc.hip), for the host library: the kernels' arguments (td_nfc_args.h) and their launches.
#pragma once
#include <hip/hip_runtime_api.h>

#include "td_nfc_args.h"

namespace td {

// td_nfc_docs, td_nfc_clear, td_nfc_check and td_nfc_sums on `stream`: a.flags and a.counts (counts[1] alone is counted).  a.head is
// zeroed by the caller on the same stream; a.changed is null.  Nothing is written when the offsets are bad.
hipError_t launch_nfc_check(const NfcArgs& a, hipStream_t stream);

// RW_RUN_MEASURE: td_nfc_docs, td_nfc_clear, td_nfc_tiles<measure>, td_nfc_scan and td_nfc_sums on `stream`: a.flags, a.changed (neither
// is null), a.counts, the tiles' places in a.tile_base (room for a word a tile of the text and one more), TD_E_CAPACITY against
// a.out_capacity, and in a.out_doc_off the entries of the documents that start at the text's end; a.out is not touched.
// RW_RUN_WRITE: td_nfc_tiles<write>: a.out and the rest of a.out_doc_off from what the measure phase left in a.tile_base and a.head (a
// phase of its own so that a host form can size a.out from counts[0] in between); nothing when the output did not fit.
hipError_t launch_nfc(const NfcArgs& a, hipStream_t stream, int phases);

}  // namespace td
