// Word-list matches (td_wordlist.hip), for the host library: the kernels' arguments (td_wordlist_args.h) and their launch.
#pragma once
#include <hip/hip_runtime_api.h>

#include "td_wordlist_args.h"

namespace td {

// td_wl_docs, td_wl_reset, td_wl_tiles<resident> and td_wl_totals on `stream`: a.stats, a.totals and a.entry_hits (either may be null).
// resident: the set's blob fits WL_LDS_BYTES and every workgroup probes its own copy in LDS; otherwise the blob is probed where it lies.
// a.head is zeroed by the caller on the same stream.
hipError_t launch_wordlist(const WlArgs& a, bool resident, hipStream_t stream);

}  // namespace td
