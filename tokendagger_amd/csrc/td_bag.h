// Bag models (td_bag.hip), for the host library: the kernels' arguments (td_bag_args.h), the scratch they need and their launch.
#pragma once
#include <hip/hip_runtime_api.h>

#include "td_bag_args.h"

namespace td {

// What a call of n_bytes and n_docs needs at most: records, chunks of BAG_CHUNK units, tiles.  A document of len bytes holds at most
// (len + 1) / 2 tokens: a document's edge separates two tokens as a delimiter does, so the documents count, and one-byte documents
// make a token a byte.
inline int64_t bag_max_recs(int64_t n_bytes, int64_t n_docs) { return std::min<int64_t>(n_bytes, (n_bytes + n_docs) / 2) + 1; }
inline int64_t bag_max_chunks(int64_t n_bytes, int64_t n_docs) { return (bag_max_recs(n_bytes, n_docs) + n_docs) / BAG_CHUNK + 1; }
inline int64_t bag_max_tiles(int64_t n_bytes) { return (n_bytes + 16 + RW_TILE - 1) / RW_TILE + 1; }

// td_bag_docs, td_bag_tiles<0>, td_bag_scan, td_bag_reset, td_bag_tiles<1>, td_bag_features, td_bag_output and td_bag_totals on `stream`.
// a.head is zeroed on the same stream in front of them (rewrite_check_locked); a.bhead needs no zeroing: td_bag_scan stores it.
hipError_t launch_bag(const BagArgs& a, hipStream_t stream);

}  // namespace td
