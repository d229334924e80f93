// Per-document word n-gram repetition statistics (td_wordgrams.hip), for the host library: the kernels' arguments
// (td_wordgrams_args.h) and their launch.
#pragma once
#include <hip/hip_runtime_api.h>

#include "td_wordgrams_args.h"

namespace td {

// The kernels of a call on `stream` (td_wordgrams.hip lists them): a.stats ([n_docs][WG_COLS]) and a.totals (may be null).  a.head is
// zeroed by the caller on the same stream; a.carry has room for two elements a tile of the text, a.rec, a.occ and a.flag for a.max_units
// words, a.cum for one more, a.table and a.cnt for rp_slots(a.max_units) words (16-byte aligned), a.first_word, a.long_doc and
// a.long_first for n_docs + 1, a.lhead for WG_L_HEAD.  Nothing is written when the offsets are bad or the text has more words than
// a.max_units.
hipError_t launch_word_ngrams(const WgArgs& a, hipStream_t stream);

}  // namespace td
