// w2v_tile.h — the stages the word2vec MFMA tile kernels of w2v.hip share
// (k_w2v_sgns, k_w2v_sgns_bf16, k_w2v_win_bf16, k_w2v_cbow_bf16): tile
// constants, the bf16 pack and row staging, the A·Bᵀ MFMA k-loop over LDS
// tiles, the window tiles' index set-up, and the block's loss reduction.  Every
// helper is inlined into its kernel; none knows which kernel called it.  The
// positive-pair loop of the pairs kernels, the k-strided MFMA loops and the
// window tiles' gradient write-out stay written out in their kernels: as
// helpers they changed the kernels' register allocation or step time
// (profiles/refactor_w2v_tiles_ab.md).
#pragma once
#include "ss_device.h"
#include "ss/w2v_window.h"

namespace ss {

static constexpr uint32_t kInv = 0xFFFFFFFFu;
static constexpr int kT = 64;  // centers per tile
static constexpr int kS = 64;  // shared negatives per tile
static constexpr int kMaxC = 16;  // contexts per center held in registers (window <= 8)
// 8 waves per workgroup: the LDS tiles (~116 KB at D = 128) allow one
// workgroup per CU, and the positive-pair loop is a per-wave latency chain
// (one context-row round trip per center), so 8 waves halve it per wave and
// double the loads in flight per CU (4 waves: 223 us per 16K-center step)
static constexpr int kNW = 8;
static constexpr int kWG = 64 * kNW;
static constexpr int kWU = 96;  // window rows per tile: 64 + 2W (W <= 15), 3 x 32
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float softplus(float x) {
  return fmaxf(x, 0.f) + __logf(1.f + __expf(-fabsf(x)));
}
__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + __expf(-x)); }

// 32x32 C/D map of v_mfma_f32_32x32x* (cdna_hip_programming.md §3):
// col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
__device__ __forceinline__ int mrow(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

__device__ __forceinline__ unsigned short f2bf(float f) {
  uint32_t u = __float_as_uint(f);
  u += 0x7FFFu + ((u >> 16) & 1u);  // round to nearest even (finite inputs)
  return (unsigned short)(u >> 16);
}
__device__ __forceinline__ float bf2f(unsigned short b) { return __uint_as_float((uint32_t)b << 16); }

// four floats -> four packed bf16 (one 8-B LDS store)
__device__ __forceinline__ uint2 pack_bf16x4(float4 v) {
  return make_uint2(f2bf(v.x) | ((uint32_t)f2bf(v.y) << 16), f2bf(v.z) | ((uint32_t)f2bf(v.w) << 16));
}

// rows -> bf16 tiles: N0 + N1 + N2 consecutive LDS rows of stride D + 8 take
// the rows id0[..], id1[..], id2[..] of uvals (kInv: a zero row).  Every load
// of the thread is issued before the first LDS store (one memory round trip
// per tile instead of one per loop trip: the loop form serialised 14
// dependent gathers per thread at D = 128).
template <int D, int N0, int N1, int N2>
__device__ __forceinline__ void w2v_stage_rows(unsigned short* __restrict__ tiles,
                                               const float* __restrict__ uvals, int tid,
                                               const uint32_t* id0, const uint32_t* id1,
                                               const uint32_t* id2) {
  constexpr int PB = D + 8, NE = (N0 + N1 + N2) * (D / 4), PER = (NE + kWG - 1) / kWG;
  float4 v[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int e = tid + i * kWG, r = e / (D / 4), d = 4 * (e - r * (D / 4));
    const uint32_t id = e >= NE ? kInv : r < N0 ? id0[r] : r < N0 + N1 ? id1[r - N0] : id2[r - N0 - N1];
    v[i] = id != kInv ? *reinterpret_cast<const float4*>(uvals + (long long)id * D + d)
                      : make_float4(0.f, 0.f, 0.f, 0.f);
  }
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int e = tid + i * kWG, r = e / (D / 4), d = 4 * (e - r * (D / 4));
    if (e < NE) *reinterpret_cast<uint2*>(tiles + r * PB + d) = pack_bf16x4(v[i]);
  }
}

// ---- bf16 MFMA (v_mfma_f32_32x32x16_bf16, fp32 accumulate) over LDS tiles.
// Lane map (cdna_hip_programming.md §3): lane l (r32 = l&31, h = l>>5) holds
// A[r32][8h + j] and B[8h + j][r32], j = 0..7; C/D as the fp32 form (mrow).
// acc += A·Bᵀ for the 32 x 32 block at (i0, j0) of two row-major tiles, K in
// steps of 16: A[i][k] = Am[i0 + i][k], B[k][j] = Bm[j0 + j][k], both
// fragments one 16-B read.
template <int K>
__device__ __forceinline__ f32x16 mfma_abt(const unsigned short* Am, int lda, int i0,
                                           const unsigned short* Bm, int ldb, int j0, int r32, int h,
                                           f32x16 acc = {}) {
#pragma unroll
  for (int k0 = 0; k0 < K; k0 += 16) {
    const bf16x8 a = *reinterpret_cast<const bf16x8*>(Am + (i0 + r32) * lda + k0 + 8 * h);
    const bf16x8 b = *reinterpret_cast<const bf16x8*>(Bm + (j0 + r32) * ldb + k0 + 8 * h);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
  }
  return acc;
}

// ---- window tiles (the batch layout of ss/w2v_window.h: a run of Rn = B + 2W
// stream positions, the centers its middle B).  Index set-up of tile `tile`,
// first center t0: window row l = run position t0 + l gets its meta word
// (-1 outside the tile's 64 + 2W rows, the run, or masked) and row id, the
// shared negatives their row ids.  The caller's barrier follows.
__device__ __forceinline__ void w2v_win_index(int tid, int tile, long long t0, long long Rn, int W,
                                              const int32_t* __restrict__ meta,
                                              const uint32_t* __restrict__ inv_w,
                                              const uint32_t* __restrict__ inv_n, int32_t* mw,
                                              uint32_t* rw, uint32_t* rn) {
  if (tid < kWU) {
    const long long q = t0 + tid;
    const bool in = tid < kT + 2 * W && q < Rn;
    const int32_t m = in ? meta[q] : -1;
    mw[tid] = m;
    rw[tid] = m >= 0 ? inv_w[q] : kInv;
  } else if (tid < kWU + kS) {
    rn[tid - kWU] = inv_n[(long long)tile * kS + (tid - kWU)];
  }
}

// ---- end of a tile kernel: the block's loss into loss_sum through the kNW
// partials `red`; a count held by wave 0's lanes (the window kernels keep
// their per-center counts in tid < kT) into cnt_sum.
__device__ __forceinline__ void w2v_block_sums(float loss, float* red, float* __restrict__ loss_sum,
                                               float cnt = 0.f, float* __restrict__ cnt_sum = nullptr) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int o = 32; o > 0; o >>= 1) loss += __shfl_down(loss, o, 64);
  if (lane == 0) red[w] = loss;
  __syncthreads();
  if (tid == 0 && loss_sum) {
    float tot = 0.f;
#pragma unroll
    for (int i = 0; i < kNW; ++i) tot += red[i];
    ctr_addf(loss_sum, tot);
  }
  if (w == 0 && cnt_sum) {
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
    if (lane == 0) ctr_addf(cnt_sum, cnt);
  }
}

}  // namespace ss
