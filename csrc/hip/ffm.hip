// ffm.hip — field-aware factorization machine, fused forward/backward (gfx950).
//
// Row of a key = [w | v_0 | .. | v_{F-1}], each v_j of K floats (dim = 1 + F*K);
// the field of an occurrence is its column in the [B, F] batch.  With R_i the
// row of occurrence i of a sample and R_i[j] its block j:
//
//   z = sum_i w_i + sum_{i<j} <R_i[j], R_j[i]>
//   g = sigmoid(z) - y,   dz/dw_i = 1,   dz/dR_i[j] = R_j[i] (j != i),   dz/dR_i[i] = 0
//
// Same contract as k_fm_fwd_bwd: inv[B*F] unique ids (kInvalidU: no occurrence,
// takes no part as i or as j), uvals / ugrad [U, dim], ugrad zeroed on entry and
// summed into with float atomics, loss to the sharded counter, pred optional.
//
// Design
// ------
// Tile.  A group of G lanes owns one sample.  Its F rows are copied once from
// global into an LDS tile T[F][LD], the whole row with w at column 0, and
// every later read is served from LDS.  The copy walks the flat element index
// e = i * dim + c with consecutive lanes on consecutive e, so a wave reads 256
// contiguous bytes of a row (less where it crosses into the next row).  Rows
// are 4 * dim bytes with dim odd: a row starts on a 4-byte boundary only, and
// a 16-byte load would need a peel of 0..3 floats that differs per row; the
// copy therefore uses dword loads, which coalesce to the same 128-byte
// requests, and leaves the alignment to the memory system.  All F * dim loads
// of a lane are independent of each other (ids sit in LDS before the walk),
// so they pipeline.
//
// Ownership.  A lane owns ORDERED elements (i, c) with c - 1 = j * K + k, the
// same walk as the copy.  For each it reads a = T[i][c] (along the row) and its
// partner b = T[j][1 + i * K + k] (down the tile's block column i), and
//   z = sum_{c = 0} a  +  1/2 sum_{c > 0, j != i} a * b :
// every unordered pair is met twice, once from each side; the halving is exact.
// That is F * (F - 1) * K FMAs per sample instead of half as many, 24 per lane at
// F = 39, K = 4 — nothing beside the B * F * dim atomics — and it buys a
// backward with no index transposition: after the one reduction the element
// (i, c) sends g * b to ugrad[u_i][c], so consecutive lanes add into
// consecutive floats of one ugrad row (c = 0: g itself, the w gradient).  The
// unordered alternative (both blocks of a pair held in registers across the
// reduction) needs a register array sized by F * (F - 1) * K / G, up to 64, and
// scatters its two blocks to two rows, K floats each; b is re-read from LDS
// after the reduction instead, one conflict-free read per atomic.
// The diagonal block (i, i) is copied with its row and never read or written.
//
// Banks.  Reading a is contiguous.  Reading b, lanes step through rows j at the
// fixed block i: address j * LD + 1 + i * K + k.  LD is the smallest value
// >= dim with LD = K (mod 32), so that address is (j * K + k) + const + 32 m j
// with LD = K + 32 m: the 64 lanes of a wave inside one row i touch 64
// consecutive banks' worth of words on a 32-bank LDS (two clean passes), and on
// 64 banks lanes c and c +- 32 would need j and j +- 32 / K of different
// parity, which 32 / K in {16, 8, 4} rules out: conflict-free.  What is left:
// a wave that straddles the end of row i reads block columns i and i + 1 in
// one instruction, at most 2-way; the id test su[j] is a broadcast.
//
// Samples per workgroup (256 lanes; the launcher picks G):
//   G =  16, 16 samples: F * dim <= 128 (F = 2..7 at small K), tiles < 1 KB
//   G =  64,  4 samples: F <= 16, a wave per sample, tile <= 8.6 KB
//   G = 256,  1 sample : F > 16; 25.7 KB at F = 39, K = 4 (6 workgroups per CU
//            of 160 KB keep other samples' loads and atomics in flight), 66.8 KB
//            at F = 64, K = 4 (2 per CU)
// The launcher computes the bytes, raises the kernel's dynamic-LDS limit once,
// and refuses a shape outside K in {2, 4, 8}, 2 <= F <= 64, F * K <= 256.
//
// No matrix instruction: an MFMA shares each operand row or column across a
// whole output tile, and here every pair's two K-vectors are its own — the
// "matrix" is F * (F - 1) / 2 unrelated K-long dots.
#include "sample_group.h"
#include "ss_device.h"
#include "ss_launch.h"

namespace ss {

static constexpr uint32_t kFfmInvalid = 0xFFFFFFFFu;
static constexpr int kFfmMaxFK = 256;
static constexpr int kFfmLdsLimit = 72 * 1024;  // the largest shape needs 66816 B

// row stride of the LDS tile in floats: >= dim and = K (mod 32)
static int ffm_row_stride(int F, int K) {
  const int dim = 1 + F * K;
  return dim + ((K - dim) % 32 + 32) % 32;
}

// lanes per sample
static int ffm_group(int F, int K) {
  return F * (1 + F * K) <= 128 ? 16 : (F <= 16 ? 64 : 256);
}

// The flat walk e = i * dim + c over a sample's elements, G apart per step.
struct FfmWalk {
  int i, c, di, dc;
  __device__ __forceinline__ FfmWalk(int l, int G, int dim)
      : i(l / dim), c(l % dim), di(G / dim), dc(G % dim) {}
  __device__ __forceinline__ void next(int dim) {
    i += di;
    c += dc;
    if (c >= dim) {
      c -= dim;
      ++i;
    }
  }
};

template <int K, int G>
__global__ __launch_bounds__(256) void k_ffm_fwd_bwd(const uint32_t* __restrict__ inv,
                                                     const float* __restrict__ labels, int B,
                                                     int F, int LD,
                                                     const float* __restrict__ uvals,
                                                     float* __restrict__ ugrad,
                                                     float* __restrict__ loss_sum,
                                                     float* __restrict__ pred) {
  extern __shared__ __attribute__((aligned(16))) float ffm_smem[];
  __shared__ float sred[4];
  __shared__ float sloss[4];
  constexpr int SPW = 256 / G;
  const int t = threadIdx.x, q = t / G, l = t % G;
  const int dim = 1 + F * K, n = F * dim;
  float* T = ffm_smem + q * (F * LD + F);
  uint32_t* su = reinterpret_cast<uint32_t*>(T + F * LD);
  const long long s = (long long)blockIdx.x * SPW + q;
  const bool live = s < B;
  for (int i = l; i < F; i += G) su[i] = live ? inv[s * F + i] : kFfmInvalid;
  __syncthreads();

  // rows -> tile, once; a row without an occurrence is zeros
  {
    FfmWalk w(l, G, dim);
#pragma unroll 4
    for (int e = l; e < n; e += G, w.next(dim)) {
      const uint32_t u = su[w.i];
      T[w.i * LD + w.c] = u != kFfmInvalid ? uvals[(long long)u * dim + w.c] : 0.f;
    }
  }
  __syncthreads();

  // z: the w column, and every ordered (i, j) element against its partner
  float acc = 0.f;
  {
    FfmWalk w(l, G, dim);
    for (int e = l; e < n; e += G, w.next(dim)) {
      const float a = T[w.i * LD + w.c];
      if (w.c == 0) {
        acc += a;
      } else {
        const int j = (w.c - 1) / K, k = (w.c - 1) % K;
        if (j != w.i) acc += 0.5f * a * T[j * LD + 1 + w.i * K + k];
      }
    }
  }
  float z;
  if constexpr (G <= 64) {
    z = group_sum(acc, G);
  } else {
    acc = group_sum(acc, 64);
    if ((t & 63) == 0) sred[t >> 6] = acc;
    __syncthreads();
    z = sred[0] + sred[1] + sred[2] + sred[3];
  }
  float g = 0.f, lo = 0.f;
  if (live) {
    const float y = labels[s];
    const float p = 1.f / (1.f + __expf(-z));
    g = p - y;
    if (l == 0) {
      if (pred) pred[s] = p;
      lo = fmaxf(z, 0.f) + __logf(1.f + __expf(-fabsf(z))) - y * z;
    }
  }
  const float bl = block_sum_256(lo, sloss);
  if (t == 0 && loss_sum) ctr_addf(loss_sum, bl);

  // gradient: element (i, c) adds into ugrad[u_i][c]
  {
    FfmWalk w(l, G, dim);
    for (int e = l; e < n; e += G, w.next(dim)) {
      const uint32_t u = su[w.i];
      if (u == kFfmInvalid) continue;
      float* gr = ugrad + (long long)u * dim + w.c;
      if (w.c == 0) {
        atomicAdd(gr, g);
      } else {
        const int j = (w.c - 1) / K, k = (w.c - 1) % K;
        if (j != w.i && su[j] != kFfmInvalid) atomicAdd(gr, g * T[j * LD + 1 + w.i * K + k]);
      }
    }
  }
}

// Raise a kernel's dynamic-LDS limit once per process.
template <auto Kernel>
static void ffm_smem_attr_once() {
  static const bool done = (check_hip(hipFuncSetAttribute((const void*)Kernel,
                                                          hipFuncAttributeMaxDynamicSharedMemorySize,
                                                          kFfmLdsLimit),
                                      "ffm smem attr"),
                            true);
  (void)done;
}

template <int K, int G>
static void ffm_launch(const uint32_t* inv, const float* labels, int B, int F, int LD, size_t bytes,
                       const float* uvals, float* ugrad, float* loss_sum, float* pred,
                       hipStream_t st) {
  ffm_smem_attr_once<k_ffm_fwd_bwd<K, G>>();
  constexpr int SPW = 256 / G;
  const int blocks = (B + SPW - 1) / SPW;
  hipLaunchKernelGGL((k_ffm_fwd_bwd<K, G>), dim3(blocks), dim3(256), bytes, st, inv, labels, B, F,
                     LD, uvals, ugrad, loss_sum, pred);
}

void launch_ffm_fwd_bwd(const uint32_t* inv, const float* labels, int B, int F, int K,
                        const float* uvals, float* ugrad, float* loss_sum, float* pred,
                        hipStream_t st) {
  if (B <= 0) return;
  if (K != 2 && K != 4 && K != 8) throw_error("ffm_fwd_bwd: K must be 2, 4 or 8");
  if (F < 2 || F > 64) throw_error("ffm_fwd_bwd: F must be in [2,64]");
  if (F * K > kFfmMaxFK) throw_error("ffm_fwd_bwd: F*K must be at most 256 (dim <= 257)");
  const int LD = ffm_row_stride(F, K), G = ffm_group(F, K);
  const size_t bytes = (size_t)(256 / G) * (F * LD + F) * sizeof(float);
  if (bytes > (size_t)kFfmLdsLimit)
    throw_error("ffm_fwd_bwd: the sample tile needs " + std::to_string(bytes) +
                " bytes of LDS, over the limit of " + std::to_string(kFfmLdsLimit));
  with_value<2, 4, 8>(K, "ffm_fwd_bwd: K must be 2, 4 or 8", [&](auto k) {
    constexpr int KK = k.value;
    with_value_or<256, 16, 64>(G, [&](auto g) {
      ffm_launch<KK, g.value>(inv, labels, B, F, LD, bytes, uvals, ugrad, loss_sum, pred, st);
    });
  });
  check_launch("k_ffm_fwd_bwd");
}

}  // namespace ss
