// ss/evict.h — which rows an eviction removes, shared by the gfx950 table
// kernels (csrc/hip/evict.hip) and the host CPU table (host_table.h), as
// ss/optim.h is for the initialisers and the update rules: one definition, so
// a CPU server and an MI355X server forget the same keys.
//
// A row is a victim iff every condition that is set holds:
//   w_below    max_j |w_j| <= w_below over the `dim` parameters (zero-init LR
//              and FTRL with L1: dead weights are exactly 0).  A kOptFTRLzn
//              row stores no w: the condition is on the derived weight
//              ftrl_weight(z, n), which the caller's `ld(j)` returns for
//              j < dim (evict.hip k_evict_mark)
//   acc_below  max_j acc_j <= acc_below over the optimizer's sum-of-squares
//              block (AdaGrad s1, FTRL n = s2, FTRLzn n = s1, Adam v = s2; SGD
//              has none).
//              With a key-seeded initialiser this loses nothing: a key whose
//              accumulator is tiny has barely moved from the initial row it
//              gets back when it returns.
// Comparisons are `<=` on the fp32 values a row reads as, so a NaN coordinate
// (the 0xFFFFFFFF "not written yet" fill, the kInitMarker payload) makes the
// row a survivor.
#pragma once
#include <cmath>
#include <cstdint>

#include "ss/optim.h"

namespace ss {

struct EvictRule {
  int use_w, use_acc;  // which conditions are set (at least one)
  float w_below, acc_below;
};

// index of the first float of the sum-of-squares block inside a row
// (parameters, then optimizer state), -1 for a rule without one
SS_HD int evict_acc_offset(int opt_kind, int dim) {
  return (opt_kind == kOptAdaGrad || opt_kind == kOptFTRLzn)
             ? dim
             : ((opt_kind == kOptFTRL || opt_kind == kOptAdam) ? 2 * dim : -1);
}

// `ld(j)`: coordinate j of the row as fp32.  acc_off: evict_acc_offset.
template <class Ld>
SS_HD bool evict_victim(const EvictRule& r, uint32_t dim, int acc_off, Ld&& ld) {
  if (!r.use_w && !r.use_acc) return false;
  if (r.use_w)
    for (uint32_t j = 0; j < dim; ++j)
      if (!(std::fabs(ld(j)) <= r.w_below)) return false;
  if (r.use_acc) {
    if (acc_off < 0) return false;
    for (uint32_t j = 0; j < dim; ++j)
      if (!(ld((uint32_t)acc_off + j) <= r.acc_below)) return false;
  }
  return true;
}

}  // namespace ss
