// evict.hip — in-place eviction of cold keys from the HBM table (gfx950).
//
// The table is open-addressed with linear probing inside [lo, hi) (ProbeSeq:
// a key's region, the whole table when rbits is 0), so a slot cannot simply
// be emptied: a key stored behind it would no longer be found.  But a maximal
// run of occupied slots between two EMPTY slots — a *cluster*, wrapping
// cyclically inside the region — contains the home slot of every key in it
// (a key sits at the first slot from its home that was free when it came, and
// no slot between the two has been emptied since).  Clusters are therefore
// repaired independently, one lane each, with plain loads and stores: walk
// the cluster in probe order from its first slot; vacate each victim's slot,
// and move each survivor behind the first victim to the first vacant slot
// from its home, if one comes before its own slot.  Every survivor stays
// findable, because after its step every slot from its home to its slot
// holds a key, and later steps only vacate slots further along the walk.
//
// Two launches (ss/evict.h has the rule):
//   k_evict_mark    one pass over the slots: flag[s] = occupied | victim << 1,
//                   from the table as it is before any slot is rewritten (a
//                   lane looking for a cluster boundary beside a lane that
//                   vacates slots would split a cluster in two); counts the
//                   victims and notes which regions have an EMPTY slot
//   k_evict_repair  the lane of a cluster's first slot walks the cluster if
//                   it holds a victim
// A region without any EMPTY slot (the state a TableFullError leaves) has no
// cluster boundary: the host rebuilds it through a buffer of its survivors
// (k_evict_clear, then launch_export / launch_assign).
//
// A vacated slot is byte-identical to a never-used slot of a fresh
// allocation: key EMPTY, row all 0xFF bytes or, in a prefilled table, the
// initial row — the CAS and the claimed inserts both rely on it (fresh_or
// reads 0xFFFFFFFF as "not written yet"; a prefilled insert writes no row).
#include "ss_device.h"
#include "ss_launch.h"
#include "ss/evict.h"

namespace ss {

static constexpr uint8_t kEvOcc = 1, kEvVictim = 2;

// the row of slot s as a never-used slot holds it
__device__ __forceinline__ void vacate_row(const DevTable& t, uint64_t s, float state_init) {
  if (t.prefilled) {
    for (uint32_t j = 0; j < t.width; ++j) row_st(t, s, j, j < t.dim ? 0.f : state_init);
    return;
  }
  char* r = t.base + s * (uint64_t)t.stride + t.row_off;
  if (t.bf16)
    for (uint32_t j = 0; j < t.width; ++j) reinterpret_cast<unsigned short*>(r)[j] = 0xFFFFu;
  else
    for (uint32_t j = 0; j < t.width; ++j) reinterpret_cast<uint32_t*>(r)[j] = 0xFFFFFFFFu;
}

// row bits of slot `from` to slot `to`, unchanged
__device__ __forceinline__ void move_row(const DevTable& t, uint64_t from, uint64_t to) {
  const char* a = t.base + from * (uint64_t)t.stride + t.row_off;
  char* b = t.base + to * (uint64_t)t.stride + t.row_off;
  if (t.bf16)
    for (uint32_t j = 0; j < t.width; ++j)
      reinterpret_cast<unsigned short*>(b)[j] = reinterpret_cast<const unsigned short*>(a)[j];
  else
    for (uint32_t j = 0; j < t.width; ++j)
      reinterpret_cast<uint32_t*>(b)[j] = reinterpret_cast<const uint32_t*>(a)[j];
}

// `mask` (optional, one byte per slot): the victims as given, instead of the rule
__global__ __launch_bounds__(256) void k_evict_mark(DevTable t, EvictRule rule, int acc_off,
                                                    const uint8_t* __restrict__ mask,
                                                    uint8_t* __restrict__ flag,
                                                    uint8_t* rhas, unsigned long long* nvict) {
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  unsigned long long nv = 0;
  for (unsigned long long s = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; s < t.cap;
       s += stride) {
    const uint64_t key = *slot_key(t, s);
    uint8_t f = 0;
    if (key == kEmptyKey) {
      // benign race: every writer stores the same byte
      const uint64_t r = t.rbits ? s / t.rlen : 0;
      if (!rhas[r]) rhas[r] = 1;
    } else {
      const bool v = mask ? mask[s] != 0
                          : evict_victim(rule, t.dim, acc_off, [&](uint32_t j) {
                              // [z | n] rows: w_below reads the derived weight
                              return t.zn && j < t.dim
                                         ? pull_val(t, row_ld(t, s, 0), row_ld(t, s, 1))
                                         : row_ld(t, s, j);
                            });
      f = kEvOcc | (v ? kEvVictim : 0);
      nv += v;
    }
    flag[s] = f;
  }
  for (int o = 32; o > 0; o >>= 1) nv += __shfl_down(nv, o, 64);
  if ((threadIdx.x & 63) == 0 && nv) ctr_add(nvict, nv);
}

// The exception to probe_slot's "a key only ever changes EMPTY -> key inside
// a launch": this launch empties and moves keys, and never runs beside a
// probe (the caller orders it behind every stream that uses the table).
__global__ __launch_bounds__(256) void k_evict_repair(DevTable t, const uint8_t* __restrict__ flag,
                                                      float state_init) {
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long s = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; s < t.cap;
       s += stride) {
    if (!(flag[s] & kEvOcc)) continue;
    ProbeSeq c;  // the walk: slot s inside its region
    c.lo = t.rbits ? (s / t.rlen) * t.rlen : 0;
    c.hi = c.lo + (t.rbits ? t.rlen : t.cap);
    c.s = s;
    if (flag[s == c.lo ? c.hi - 1 : s - 1] & kEvOcc) continue;  // not a cluster's first slot
    const uint64_t len = c.len();
    // a slot behind the walk is vacant: until the first victim every key's
    // slots from its home to its own still hold keys, and nothing moves
    bool vac = false;
    for (uint64_t n = 0; n < len; ++n, c.next()) {
      const uint64_t p = c.s;
      const uint8_t f = flag[p];
      if (!(f & kEvOcc)) break;  // the cluster's end
      if (f & kEvVictim) {
        *slot_key(t, p) = kEmptyKey;
        vacate_row(t, p, state_init);
        vac = true;
        continue;
      }
      if (!vac) continue;
      // the first vacant slot from the key's home, if one comes before p
      // (the probe stays inside this cluster; the bound only guards a table
      // whose invariant broke)
      const uint64_t key = *slot_key(t, p);
      ProbeSeq q = probe_seq(t, key);
      uint64_t m = 0;
      while (q.s != p && m < len && *slot_key(t, q.s) != kEmptyKey) {
        q.next();
        ++m;
      }
      if (q.s == p || m >= len) continue;  // it stays where it is
      move_row(t, p, q.s);
      *slot_key(t, q.s) = key;
      *slot_key(t, p) = kEmptyKey;
      vacate_row(t, p, state_init);
    }
  }
}

// vacate the slots of [s0, s0 + n): the victims (`victims_only`) or all
__global__ __launch_bounds__(256) void k_evict_clear(DevTable t, unsigned long long s0, long long n,
                                                     const uint8_t* __restrict__ flag,
                                                     int victims_only, float state_init) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const unsigned long long s = s0 + i;
    const uint8_t f = flag[s];
    if (!(f & kEvOcc) || (victims_only && !(f & kEvVictim))) continue;
    *slot_key(t, s) = kEmptyKey;
    vacate_row(t, s, state_init);
  }
}

// ---------------------------------------------------------------- launchers
static int evict_grid(unsigned long long n) {
  unsigned long long b = (n + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 16384 ? 16384 : b));
}

void launch_evict_mark(const DevTable& t, const EvictRule& rule, int opt_kind, const uint8_t* mask,
                       uint8_t* flag, uint8_t* rhas, unsigned long long* nvict, hipStream_t st) {
  if (!flag || !rhas || !nvict) throw_error("evict: flag / region / counter buffers");
  const int acc_off = evict_acc_offset(opt_kind, (int)t.dim);
  if (!mask) {
    if (!rule.use_w && !rule.use_acc) throw_error("evict: a rule needs w_below or acc_below");
    if (rule.use_acc && (acc_off < 0 || (uint32_t)acc_off + t.dim > t.width))
      throw_error("evict: acc_below needs an optimizer with a sum-of-squares block");
  }
  hipLaunchKernelGGL(k_evict_mark, dim3(evict_grid(t.cap)), dim3(256), 0, st, t, rule, acc_off,
                     mask, flag, rhas, nvict);
  check_launch("k_evict_mark");
}

void launch_evict_repair(const DevTable& t, const uint8_t* flag, float state_init,
                         hipStream_t st) {
  hipLaunchKernelGGL(k_evict_repair, dim3(evict_grid(t.cap)), dim3(256), 0, st, t, flag,
                     state_init);
  check_launch("k_evict_repair");
}

void launch_evict_clear(const DevTable& t, unsigned long long s0, long long n, const uint8_t* flag,
                        int victims_only, float state_init, hipStream_t st) {
  if (n <= 0) return;
  if (s0 + (unsigned long long)n > t.cap) throw_error("evict: slot range outside the table");
  hipLaunchKernelGGL(k_evict_clear, dim3(evict_grid((unsigned long long)n)), dim3(256), 0, st, t,
                     s0, n, flag, victims_only, state_init);
  check_launch("k_evict_clear");
}

}  // namespace ss
