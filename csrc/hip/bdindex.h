// bdindex.h — occurrence -> unique id through the bucketed dedup's outputs
// (bdedup.hip) without a materialised inverse index:
//   uid(j) = ubase[bkt[j]] + luid[pos_of[j]]
// bkt / pos_of are read coalesced, ubase is L2-resident, luid is one gather.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace ss {

struct BdIndex {
  const uint32_t* pos_of;
  const uint32_t* luid;
  const uint32_t* bkt;
  const uint32_t* ubase;
  __device__ __forceinline__ uint32_t uid(long long j) const {
    const uint32_t p = pos_of[j];
    if (p == 0xFFFFFFFFu) return 0xFFFFFFFFu;
    const uint32_t l = luid[p];
    return l == 0xFFFFFFFFu ? 0xFFFFFFFFu : ubase[bkt[j]] + l;
  }
};

// The bucketed dedup's output as the bucket kernels walk it, one workgroup
// per bucket b (a BdLayout scratch through bd_view, or a server merge's own
// arrays).  Host-side only: the kernels take the arrays as separate
// __restrict__ arguments, and no kernel takes them all.
struct BucketView {
  int P = 0;                         // buckets
  const uint32_t* bstart = nullptr;  // [P + 1], by bucket: its first position
  const uint32_t* ubase = nullptr;   // [P], by bucket: unique id of its first distinct key
  const uint32_t* unum = nullptr;    // [P], by bucket: its distinct keys
  const uint32_t* pj = nullptr;      // by position: the occurrence's index in the call's keys
  const uint32_t* luid = nullptr;    // by position: the key's id inside its bucket (~0: none)
  const uint64_t* bkeys = nullptr;   // by bstart[b] + in-bucket id: the distinct keys, staged
};
// ... as launch_srv_dedup writes it
struct BucketViewOut {
  uint32_t *bstart, *ubase, *unum, *pj, *luid;
  uint64_t* bkeys;
};

}  // namespace ss
