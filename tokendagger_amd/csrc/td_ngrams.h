// N-gram matches (td_ngrams.hip), for the host library: the kernels' arguments (td_ngram_args.h) and their launch.
#pragma once
#include <hip/hip_runtime_api.h>

#include "td_ngram_args.h"

namespace td {

// td_ng_docs, td_ng_clear, td_ng_tiles and td_ng_finish on `stream`; a.head is zeroed by the caller on the same stream, every output by
// td_ng_clear (a.pat_counts only with zero_pat_counts), and by nobody when the offsets are bad.  n_pats: the entries of a.pat_counts.
hipError_t launch_ngram_matches(const NgramArgs& a, int64_t n_pats, bool zero_pat_counts, hipStream_t stream);

}  // namespace td
