// Token counts (td_counts.hip), for the host library: the kernel's arguments (td_counts_args.h) and their launch.
#pragma once
#include <hip/hip_runtime_api.h>

#include "td_counts_args.h"

namespace td {

// td_cnt_tiles<groups> on cnt_grid(a.n_tokens) workgroups; a.info is zeroed (and a.counts zeroed or kept) by the caller, on the same stream
hipError_t launch_token_counts(const CountsArgs& a, hipStream_t stream);

}  // namespace td
