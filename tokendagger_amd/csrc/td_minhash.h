// MinHash signatures (td_minhash.hip), for the host library: the kernels' arguments (td_minhash_args.h) and their launch.
#pragma once
#include <hip/hip_runtime_api.h>

#include "td_minhash_args.h"

namespace td {

// td_mh_docs, td_mh_clear, td_mh_tiles and (with a.bands > 0) td_mh_finish on `stream`; a.head is zeroed by the caller on the same
// stream, sig and counts by td_mh_clear, and by nobody when the offsets are bad.
hipError_t launch_minhash(const MhashArgs& a, hipStream_t stream);

// td_mh_params on `stream`: table[j] = mh_param(seed, j) for j < num_perm, the same values td_minhash_params gives on the host.
hipError_t launch_minhash_params(MhParam* table, uint64_t seed, int num_perm, hipStream_t stream);

}  // namespace td
