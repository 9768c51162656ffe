// DTNN (Deep Tensor Neural Network) pair interaction, fused in both directions, and the device collation of its batches.
//
// For a pair list sorted by its first atom (mem_i non-decreasing, mem_j) and atom rows ah = C . W_cf + b_cf (N x H):
//
//     Y[i] = sum over the pairs p with mem_i[p] = i of  tanh( ((g_p . W_df + b_df) (.) ah[mem_j[p]]) . W_fc )
//
// where the Gaussian row g_p (K values) is either generated in registers from ONE float per pair, the distance
// (exp(-(d - s_k)^2 / (2 step^2)), s_k = distance_min + k step: the model's path), or read from a P x K matrix (the
// layer's contract).  Neither pass writes a P x K or P x H tensor: the backward regenerates g_p, recomputes the hidden
// rows and the tanh from d, ah and the weights, and produces d_ah (atomics by mem_j), dW_df, db_df and dW_fc.
//
// Layout.  A wave owns a tile of 32 pairs.  All products run on v_mfma_f32_32x32x16_bf16 with the three-way bf16 split
// of split_bf16.h (six products, fp32 accumulation).  The K -> H product is taken TRANSPOSED, D[h][pair], with the
// weight fragment as the A operand (split once per workgroup, resident in LDS as ready-made fragments: one
// ds_read_b128 each) and the Gaussians as the B operand: lane l holds pair l & 31 and generates exactly the 8 values
// k = 16 ks + 8 (l >> 5) + j of its fragment.  The result has the pair on the lane and 16 hidden columns per 32-column
// block in the registers, which is the operand layout of the next product that sums over the hidden index: the H -> E
// product (and in the backward the E -> H one) takes the registers as they are, with a weight image whose k slots are
// permuted to the accumulator's register order.  No activation passes through LDS in the forward.
//
// The weight-gradient products sum over the PAIRS, which sit on the lanes: their operands go through a per-wave LDS
// tile once (32 x 64 floats, pitch 68), the Gaussians of dW_df are regenerated for the transposed fragment (lane = k),
// and the partial sums stay in the accumulators of the persistent wave until its last tile, then one atomic per
// element.  Dynamic LDS: 72 KB (forward) / 132 KB (backward) at the widest shape.
#include <math.h>

#include "common.h"
#include "split_bf16.h"

namespace gcmi {
namespace {

constexpr int kDtnnThreads = 256;
constexpr int kDtnnWaves = kDtnnThreads / 64;
constexpr int kDtnnKS = 8;       // k-steps of 16 Gaussians: n_distance <= 128
constexpr int kDtnnTileFloats = 32 * kTilePitch + 64;  // + 32 doubles: the pairs' scaled distances
constexpr float kHalfLog2e = 0.72134752044448170368f;

struct DtnnArgs {
  const float* src;  // FROM_D: P distances; else P x ldg Gaussian rows
  int64_t ldg;
  const int32_t* mem_i;
  const int32_t* mem_j;
  int32_t P, N, K, H, E, n_tiles;
  const float* ah;
  int64_t ldah;
  const float *w_df, *b_df, *w_fc;  // contiguous K x H, H, H x E
  double dmin, inv_step;
  float* y;  // forward: N x E, zeroed by the launcher, added into
  int64_t ldy;
  const float* dy;  // backward
  int64_t lddy;
  float* dah;  // N x H, zeroed by the launcher
  int64_t lddah;
  float *dw_df, *db_df, *dw_fc;  // added into
};

__device__ __forceinline__ bool dev_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the feature a lane's accumulator register r holds inside a 32-column block (its other index is on the lane)
// k slot (half, j) of k-step s of a product that takes accumulator registers as its operand -> the feature index
__device__ __forceinline__ int slot_feat(int s, int half, int j) { return 16 * s + 8 * (j >> 2) + 4 * half + (j & 3); }

// Fragment images of the weights, built once per workgroup, piece-major (s = the piece: a whole image apart, indexed
// by hand where they are written and read):
//   WDF[s][nt][ks][lane]: A[row h = 32 nt + (lane & 31)][k = 16 ks + 8 half + j] = W_df[k][h]
//   FC1[s][et][ks][lane]: row / column e = 32 et + (lane & 31), slots h = slot_feat(ks, half, j): W_fc[h][e]
//   FC2[s][ht][ks][lane]: row h = 32 ht + (lane & 31), slots e = slot_feat(ks, half, j): W_fc[h][e]
template <int NTH, int NTE, bool BWD>
__device__ __forceinline__ void build_images(const DtnnArgs& a, u32x4* WDF, u32x4* FC1, u32x4* FC2) {
  const int K = a.K, H = a.H, E = a.E;
  for (int f = threadIdx.x; f < NTH * kDtnnKS * 64; f += kDtnnThreads) {
    const int lane = f & 63, ks = (f >> 6) % kDtnnKS, nt = (f >> 6) / kDtnnKS;
    const int h = 32 * nt + (lane & 31), half = lane >> 5;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = 16 * ks + 8 * half + j;
      v[j] = (k < K && h < H) ? a.w_df[(int64_t)k * H + h] : 0.f;
    }
    const Frag3 fr = split_frag(v);
#pragma unroll
    for (int s = 0; s < 3; ++s) WDF[((s * NTH + nt) * kDtnnKS + ks) * 64 + lane] = fr.p[s];
  }
  for (int f = threadIdx.x; f < NTE * 2 * NTH * 64; f += kDtnnThreads) {
    const int lane = f & 63, ks = (f >> 6) % (2 * NTH), et = (f >> 6) / (2 * NTH);
    const int e = 32 * et + (lane & 31), half = lane >> 5;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int h = slot_feat(ks, half, j);
      v[j] = (h < H && e < E) ? a.w_fc[(int64_t)h * E + e] : 0.f;
    }
    const Frag3 fr = split_frag(v);
#pragma unroll
    for (int s = 0; s < 3; ++s) FC1[((s * NTE + et) * 2 * NTH + ks) * 64 + lane] = fr.p[s];
  }
  if constexpr (BWD) {
    for (int f = threadIdx.x; f < NTH * 2 * NTE * 64; f += kDtnnThreads) {
      const int lane = f & 63, ks = (f >> 6) % (2 * NTE), ht = (f >> 6) / (2 * NTE);
      const int h = 32 * ht + (lane & 31), half = lane >> 5;
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int e = slot_feat(ks, half, j);
        v[j] = (h < H && e < E) ? a.w_fc[(int64_t)h * E + e] : 0.f;
      }
      const Frag3 fr = split_frag(v);
#pragma unroll
      for (int s = 0; s < 3; ++s) FC2[((s * NTH + ht) * 2 * NTE + ks) * 64 + lane] = fr.p[s];
    }
  }
}

// exp(-(d - s_k)^2 / (2 step^2)) from u = (d - distance_min) / step - k
__device__ __forceinline__ float gaussian_of(double u0, int k) {
  const float u = (float)(u0 - (double)k);
  return exp2f(-kHalfLog2e * u * u);
}

// 4 consecutive columns c0.. of one row (nullptr row: zeros); columns >= C read as zero
__device__ __forceinline__ float4 load4(const float* row, int c0, int C, bool vec) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (row == nullptr) return v;
  if (vec && c0 + 4 <= C) return *reinterpret_cast<const float4*>(row + c0);
  if (c0 + 0 < C) v.x = row[c0 + 0];
  if (c0 + 1 < C) v.y = row[c0 + 1];
  if (c0 + 2 < C) v.z = row[c0 + 2];
  if (c0 + 3 < C) v.w = row[c0 + 3];
  return v;
}

// One pair per lane (& 31): what the tile walk knows about it
struct PairLane {
  int i, j;     // i = -1: no pair (past the end)
  double u0;    // FROM_D: (d - distance_min) / step
  const float* grow;  // !FROM_D: its Gaussian row, or nullptr
};

template <bool FROM_D>
__device__ __forceinline__ PairLane load_pair(const DtnnArgs& a, int p) {
  PairLane q;
  const bool valid = p < a.P;
  q.i = valid ? a.mem_i[p] : -1;
  int j = valid ? a.mem_j[p] : 0;
  q.j = j < 0 ? 0 : (j >= a.N ? a.N - 1 : j);
  if (q.i >= a.N) q.i = -1;
  q.u0 = 0.0;
  q.grow = nullptr;
  if constexpr (FROM_D) {
    q.u0 = ((double)(valid ? a.src[p] : 0.f) - a.dmin) * a.inv_step;
  } else {
    q.grow = valid ? a.src + (int64_t)p * a.ldg : nullptr;
  }
  return q;
}

// dh[nt] (lane = pair, registers = hidden columns) = W_df^T g, then + b_df, and m = dh (.) ah[j]; ahv keeps ah[j]
template <bool FROM_D, int NTH>
__device__ __forceinline__ void tile_hidden(const DtnnArgs& a, const u32x4* WDF, const PairLane& q, int lane,
                                            f32x16 (&dh)[NTH], f32x16 (&ahv)[NTH]) {
  const int half = lane >> 5;
  const int KS = (a.K + 15) >> 4;
  const bool gvec = !FROM_D && (a.ldg % 4 == 0) && dev_aligned16(a.src);
#pragma unroll
  for (int nt = 0; nt < NTH; ++nt) dh[nt] = zero_acc();
  for (int ks = 0; ks < KS; ++ks) {
    Frag3 fb;
    const int k0 = 16 * ks + 8 * half;
    if constexpr (FROM_D) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = gaussian_of(q.u0, k0 + j);
      fb = split_frag(v);
    } else {
      fb = split_frag(load4(q.grow, k0, a.K, gvec), load4(q.grow, k0 + 4, a.K, gvec));
    }
#pragma unroll
    for (int nt = 0; nt < NTH; ++nt) {
      const Frag3 w = {{WDF[((0 * NTH + nt) * kDtnnKS + ks) * 64 + lane], WDF[((1 * NTH + nt) * kDtnnKS + ks) * 64 + lane],
                        WDF[((2 * NTH + nt) * kDtnnKS + ks) * 64 + lane]}};
      mfma_split6(dh[nt], w, fb);
    }
  }
  const bool avec = (a.ldah % 4 == 0) && dev_aligned16(a.ah);
  const float* arow = a.ah + (int64_t)q.j * a.ldah;
#pragma unroll
  for (int nt = 0; nt < NTH; ++nt) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int h0 = 32 * nt + 8 * g + 4 * half;
      const float4 b = load4(a.b_df, h0, a.H, false);
      const float4 x = load4(arow, h0, a.H, avec);
      dh[nt][4 * g + 0] += b.x; dh[nt][4 * g + 1] += b.y; dh[nt][4 * g + 2] += b.z; dh[nt][4 * g + 3] += b.w;
      ahv[nt][4 * g + 0] = x.x; ahv[nt][4 * g + 1] = x.y; ahv[nt][4 * g + 2] = x.z; ahv[nt][4 * g + 3] = x.w;
    }
  }
}

// the fragment of k-step s of a product whose operand is a row of accumulator tiles
template <int NT>
__device__ __forceinline__ Frag3 acc_frag(const f32x16 (&x)[NT], int s) {
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = x[s >> 1][8 * (s & 1) + j];
  return split_frag(v);
}

// ---------------------------------------------------------------------------------------------------- forward
template <bool FROM_D, int NTH, int NTE>
__global__ __launch_bounds__(kDtnnThreads) void dtnn_fwd_kernel(const DtnnArgs a) {
  extern __shared__ u32x4 dtnn_smem[];
  u32x4* WDF = dtnn_smem;
  u32x4* FC1 = WDF + 3 * NTH * kDtnnKS * 64;
  build_images<NTH, NTE, false>(a, WDF, FC1, nullptr);
  __syncthreads();
  const int lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
  const int gw = blockIdx.x * kDtnnWaves + (threadIdx.x >> 6), nw = gridDim.x * kDtnnWaves;
  for (int tile = gw; tile < a.n_tiles; tile += nw) {
    const int p0 = tile * 32;
    const PairLane q = load_pair<FROM_D>(a, p0 + l31);
    f32x16 dh[NTH], ahv[NTH];
    tile_hidden<FROM_D, NTH>(a, WDF, q, lane, dh, ahv);
#pragma unroll
    for (int nt = 0; nt < NTH; ++nt) dh[nt] *= ahv[nt];
    // z (rows = pairs in the registers, lane = output column): A = m taken from the accumulators, B = FC1
    f32x16 z[NTE];
#pragma unroll
    for (int et = 0; et < NTE; ++et) z[et] = zero_acc();
#pragma unroll
    for (int s = 0; s < 2 * NTH; ++s) {
      const Frag3 fa = acc_frag<NTH>(dh, s);
#pragma unroll
      for (int et = 0; et < NTE; ++et) {
        Frag3 w;
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) w.p[pc] = FC1[((pc * NTE + et) * 2 * NTH + s) * 64 + lane];
        mfma_split6(z[et], fa, w);
      }
    }
#pragma unroll
    for (int et = 0; et < NTE; ++et)
#pragma unroll
      for (int r = 0; r < 16; ++r) z[et][r] = tanhf(z[et][r]);
    // per run of equal first atoms: the sum over its rows, one atomic per column (a run may continue in the next tile)
    const int nvalid = min(32, a.P - p0);
    int row = 0;
    while (row < nvalid) {
      const int i = __shfl(q.i, row);
      const unsigned long long neq = __ballot(lane < 32 && l31 > row && q.i != i);
      const int end = neq ? __ffsll((long long)neq) - 1 : 32;
#pragma unroll
      for (int et = 0; et < NTE; ++et) {
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rr = acc_row(r, half);
          s += (rr >= row && rr < end) ? z[et][r] : 0.f;
        }
        s += __shfl_xor(s, 32);
        const int e = 32 * et + l31;
        if (lane < 32 && i >= 0 && e < a.E) unsafeAtomicAdd(a.y + (int64_t)i * a.ldy + e, s);
      }
      row = end;
    }
  }
}

// ---------------------------------------------------------------------------------------------------- backward
// (lane = pair, registers = columns) -> the per-wave LDS tile T[pair][column]
template <int NT>
__device__ __forceinline__ void tile_store(float* T, const f32x16 (&x)[NT], int lane) {
  const int half = lane >> 5, l31 = lane & 31;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<float4*>(T + l31 * kTilePitch + 32 * t + 8 * g + 4 * half) =
          make_float4(x[t][4 * g], x[t][4 * g + 1], x[t][4 * g + 2], x[t][4 * g + 3]);
}
// the fragment with this lane's column c and the 8 pairs 16 ks + 8 half + j as its k slots
__device__ __forceinline__ Frag3 tile_frag(const float* T, int ks, int c, int half) {
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = T[(16 * ks + 8 * half + j) * kTilePitch + c];
  return split_frag(v);
}

template <bool FROM_D, int NTH, int NTE>
__global__ __launch_bounds__(kDtnnThreads) void dtnn_bwd_kernel(const DtnnArgs a) {
  extern __shared__ u32x4 dtnn_smem[];
  u32x4* WDF = dtnn_smem;
  u32x4* FC1 = WDF + 3 * NTH * kDtnnKS * 64;
  u32x4* FC2 = FC1 + 3 * NTE * 2 * NTH * 64;
  const int wave = threadIdx.x >> 6;
  float* T = reinterpret_cast<float*>(FC2 + 3 * NTH * 2 * NTE * 64) + wave * kDtnnTileFloats;
  double* U0 = reinterpret_cast<double*>(T + 32 * kTilePitch);
  build_images<NTH, NTE, true>(a, WDF, FC1, FC2);
  __syncthreads();
  const int lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
  const int gw = blockIdx.x * kDtnnWaves + wave, nw = gridDim.x * kDtnnWaves;
  const int KT = (a.K + 31) >> 5;
  const bool dyvec = (a.lddy % 4 == 0) && dev_aligned16(a.dy);
  f32x16 accdf[4][NTH], accfc[NTH][NTE], accb[NTH];
#pragma unroll
  for (int nt = 0; nt < NTH; ++nt) {
    accb[nt] = zero_acc();
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) accdf[kt][nt] = zero_acc();
#pragma unroll
    for (int et = 0; et < NTE; ++et) accfc[nt][et] = zero_acc();
  }
  const int rounds = (a.n_tiles + nw - 1) / nw;  // the same for every wave of the workgroup: barriers inside
  for (int it = 0; it < rounds; ++it) {
    const int tile = gw + it * nw;
    const bool active = tile < a.n_tiles;  // wave-uniform
    const int p0 = tile * 32;
    f32x16 m[NTH], dz[NTE], ddh[NTH];
    if (active) {
      const PairLane q = load_pair<FROM_D>(a, p0 + l31);
      f32x16 dh[NTH], ahv[NTH];
      tile_hidden<FROM_D, NTH>(a, WDF, q, lane, dh, ahv);
#pragma unroll
      for (int nt = 0; nt < NTH; ++nt) m[nt] = dh[nt] * ahv[nt];
      // z^T (lane = pair, registers = output columns): A = FC1, B = m from the accumulators
#pragma unroll
      for (int et = 0; et < NTE; ++et) dz[et] = zero_acc();
#pragma unroll
      for (int s = 0; s < 2 * NTH; ++s) {
        const Frag3 fb = acc_frag<NTH>(m, s);
#pragma unroll
        for (int et = 0; et < NTE; ++et) {
          const Frag3 w = {{FC1[((0 * NTE + et) * 2 * NTH + s) * 64 + lane], FC1[((1 * NTE + et) * 2 * NTH + s) * 64 + lane],
                            FC1[((2 * NTE + et) * 2 * NTH + s) * 64 + lane]}};
          mfma_split6(dz[et], w, fb);
        }
      }
      // dz = dY[i] (.) (1 - tanh^2); zero where there is no pair or no column
      const float* dyrow = q.i >= 0 ? a.dy + (int64_t)q.i * a.lddy : nullptr;
#pragma unroll
      for (int et = 0; et < NTE; ++et)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float4 gy = load4(dyrow, 32 * et + 8 * g + 4 * half, a.E, dyvec);
          const float gv[4] = {gy.x, gy.y, gy.z, gy.w};
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float t = tanhf(dz[et][4 * g + c]);
            dz[et][4 * g + c] = gv[c] * (1.f - t * t);
          }
        }
      // dm^T (lane = pair, registers = hidden columns): A = FC2, B = dz from the accumulators
      f32x16 dm[NTH];
#pragma unroll
      for (int nt = 0; nt < NTH; ++nt) dm[nt] = zero_acc();
#pragma unroll
      for (int s = 0; s < 2 * NTE; ++s) {
        const Frag3 fb = acc_frag<NTE>(dz, s);
#pragma unroll
        for (int nt = 0; nt < NTH; ++nt) {
          const Frag3 w = {{FC2[((0 * NTH + nt) * 2 * NTE + s) * 64 + lane], FC2[((1 * NTH + nt) * 2 * NTE + s) * 64 + lane],
                            FC2[((2 * NTH + nt) * 2 * NTE + s) * 64 + lane]}};
          mfma_split6(dm[nt], w, fb);
        }
      }
      // d_ah[j] += dm (.) dh; ddh = dm (.) ah[j]; db_df += ddh
      float* drow = a.dah + (int64_t)q.j * a.lddah;
#pragma unroll
      for (int nt = 0; nt < NTH; ++nt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int h = 32 * nt + acc_row(r, half);
          if (q.i >= 0 && h < a.H) unsafeAtomicAdd(drow + h, dm[nt][r] * dh[nt][r]);
        }
        ddh[nt] = dm[nt] * ahv[nt];
        accb[nt] += ddh[nt];
      }
      tile_store<NTH>(T, m, lane);
    }
    __syncthreads();
    // dW_fc += m^T dz: A = m with the hidden column on the lane, B = dz with the output column on the lane
    Frag3 fm[2][NTH];
    if (active) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int nt = 0; nt < NTH; ++nt) fm[ks][nt] = tile_frag(T, ks, 32 * nt + l31, half);
    }
    __syncthreads();
    if (active) tile_store<NTE>(T, dz, lane);
    __syncthreads();
    if (active) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int et = 0; et < NTE; ++et) {
          const Frag3 fz = tile_frag(T, ks, 32 * et + l31, half);
#pragma unroll
          for (int nt = 0; nt < NTH; ++nt) mfma_split6(accfc[nt][et], fm[ks][nt], fz);
        }
    }
    __syncthreads();
    if (active) {
      tile_store<NTH>(T, ddh, lane);
      if constexpr (FROM_D) {
        const int p = p0 + l31;
        if (lane < 32) U0[l31] = ((double)(p < a.P ? a.src[p] : 0.f) - a.dmin) * a.inv_step;
      }
    }
    __syncthreads();
    // dW_df += g^T ddh: A = the Gaussians with k on the lane (regenerated), B = ddh with the hidden column on the lane
    if (active) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        Frag3 fd[NTH];
#pragma unroll
        for (int nt = 0; nt < NTH; ++nt) fd[nt] = tile_frag(T, ks, 32 * nt + l31, half);
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
          if (kt < KT) {
            const int k = 32 * kt + l31;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const int pr = 16 * ks + 8 * half + j;
              if constexpr (FROM_D) {
                v[j] = gaussian_of(U0[pr], k);
              } else {
                v[j] = (p0 + pr < a.P && k < a.K) ? a.src[(int64_t)(p0 + pr) * a.ldg + k] : 0.f;
              }
            }
            const Frag3 fg = split_frag(v);
#pragma unroll
            for (int nt = 0; nt < NTH; ++nt) mfma_split6(accdf[kt][nt], fg, fd[nt]);
          }
        }
      }
    }
    __syncthreads();
  }
  // flush: one atomic per element and wave
#pragma unroll
  for (int nt = 0; nt < NTH; ++nt) {
    const int c = 32 * nt + l31;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int k = 32 * kt + acc_row(r, half);
        if (kt < KT && k < a.K && c < a.H) unsafeAtomicAdd(a.dw_df + (int64_t)k * a.H + c, accdf[kt][nt][r]);
      }
#pragma unroll
    for (int et = 0; et < NTE; ++et)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int h = 32 * nt + acc_row(r, half), e = 32 * et + l31;
        if (h < a.H && e < a.E) unsafeAtomicAdd(a.dw_fc + (int64_t)h * a.E + e, accfc[nt][et][r]);
      }
    // db_df: the registers hold hidden columns, the lanes of a half the pairs
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float s = accb[nt][r];
#pragma unroll
      for (int o = 1; o < 32; o <<= 1) s += __shfl_xor(s, o);
      const int h = 32 * nt + acc_row(r, half);
      if (l31 == 0 && h < a.H) unsafeAtomicAdd(a.db_df + h, s);
    }
  }
}

template <bool BWD, bool FROM_D, int NTH, int NTE>
int launch_dtnn(const DtnnArgs& a, hipStream_t st) {
  size_t lds = (size_t)(3 * NTH * kDtnnKS + 3 * NTE * 2 * NTH) * 64 * 16;
  if (BWD) lds += (size_t)3 * NTH * 2 * NTE * 64 * 16 + (size_t)kDtnnWaves * kDtnnTileFloats * 4;
  void (*kern)(const DtnnArgs);
  if constexpr (BWD) {
    kern = dtnn_bwd_kernel<FROM_D, NTH, NTE>;
  } else {
    kern = dtnn_fwd_kernel<FROM_D, NTH, NTE>;
  }
  static LdsLimit lim;  // per instantiation
  if (lds > 64 * 1024 && !raise_lds_limit(lim, reinterpret_cast<const void*>(kern), lds)) {
    set_error("dtnn_pair: hipFuncSetAttribute(max dynamic LDS = %zu) failed", lds);
    return GCMI_ERR_LAUNCH;
  }
  // persistent waves: a few tiles each, so that the weight images (and the backward's flush) are paid once per several
  const int per_wg = kDtnnWaves * (BWD ? 4 : 2);
  const int grid = std::max(1, std::min((a.n_tiles + per_wg - 1) / per_wg, BWD ? 256 : 512));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kDtnnThreads), lds, st, a);
  GCMI_CHECK_LAUNCH(BWD ? "dtnn_pair_bwd" : "dtnn_pair_fwd");
  return GCMI_OK;
}

template <bool BWD>
int dispatch_dtnn(const DtnnArgs& a, bool from_d, hipStream_t st) {
  const int nth = (a.H + 31) / 32, nte = (a.E + 31) / 32;
#define GCMI_DTNN_CASE(D, TH, TE) \
  if (from_d == D && nth == TH && nte == TE) return launch_dtnn<BWD, D, TH, TE>(a, st);
  GCMI_DTNN_CASE(true, 1, 1) GCMI_DTNN_CASE(true, 1, 2) GCMI_DTNN_CASE(true, 2, 1) GCMI_DTNN_CASE(true, 2, 2)
  GCMI_DTNN_CASE(false, 1, 1) GCMI_DTNN_CASE(false, 1, 2) GCMI_DTNN_CASE(false, 2, 1) GCMI_DTNN_CASE(false, 2, 2)
#undef GCMI_DTNN_CASE
  set_error("dtnn_pair: no kernel for n_hidden %d, n_embedding %d", a.H, a.E);
  return GCMI_ERR_UNSUPPORTED;
}

int check_dtnn(const char* what, const float* d_src, int64_t ld_src, int32_t from_distance, const int32_t* d_mem_i,
               const int32_t* d_mem_j, int64_t n_pairs, int32_t n_atoms, const float* d_ah, int64_t ldah,
               int32_t n_hidden, const float* d_w_df, const float* d_b_df, int32_t n_distance, const float* d_w_fc,
               int32_t n_embedding, double step) {
  GCMI_CHECK_ARG(n_embedding > 0 && n_embedding <= 64 && n_hidden > 0 && n_hidden <= 64 && n_distance > 0 &&
                     n_distance <= 128,
                 "%s: n_embedding %d, n_hidden %d, n_distance %d outside 1..64, 1..64, 1..128", what, n_embedding,
                 n_hidden, n_distance);
  GCMI_CHECK_ARG(n_pairs >= 0 && n_pairs < ((int64_t)1 << 31) - 64 && n_atoms >= 0 && ldah >= n_hidden,
                 "%s: bad sizes (%lld pairs, %d atoms, ldah %lld)", what, (long long)n_pairs, n_atoms, (long long)ldah);
  GCMI_CHECK_ARG(n_pairs == 0 || n_atoms > 0, "%s: pairs without atoms", what);
  GCMI_CHECK_ARG(from_distance ? (step > 0.0 || step < 0.0) : ld_src >= n_distance,
                 "%s: %s", what, from_distance ? "zero distance step" : "Gaussian rows shorter than n_distance");
  GCMI_CHECK_ARG(d_w_df && d_b_df && d_w_fc, "%s: NULL weights", what);
  GCMI_CHECK_ARG(n_pairs == 0 || (d_src && d_mem_i && d_mem_j && d_ah), "%s: NULL buffer", what);
  return GCMI_OK;
}

// the fields both directions fill alike: the pair list, the atom rows, the weights (arguments as check_dtnn's)
DtnnArgs dtnn_inputs(const float* d_src, int64_t ld_src, int32_t from_distance, const int32_t* d_mem_i,
                     const int32_t* d_mem_j, int64_t n_pairs, int32_t n_atoms, const float* d_ah, int64_t ldah,
                     int32_t n_hidden, const float* d_w_df, const float* d_b_df, int32_t n_distance, const float* d_w_fc,
                     int32_t n_embedding, double distance_min, double step) {
  DtnnArgs a = {};
  a.src = d_src; a.ldg = ld_src; a.mem_i = d_mem_i; a.mem_j = d_mem_j;
  a.P = (int32_t)n_pairs; a.N = n_atoms; a.K = n_distance; a.H = n_hidden; a.E = n_embedding;
  a.n_tiles = (int32_t)((n_pairs + 31) / 32);
  a.ah = d_ah; a.ldah = ldah; a.w_df = d_w_df; a.b_df = d_b_df; a.w_fc = d_w_fc;
  a.dmin = distance_min; a.inv_step = from_distance ? 1.0 / step : 0.0;
  return a;
}

// ---------------------------------------------------------------------------------------------------- collation
// atom_off / pair_off [B + 1]: exclusive sums of n and n^2 over the batch's molecules (one workgroup)
__global__ __launch_bounds__(256) void dtnn_offsets_kernel(const int32_t* __restrict__ n_atoms_all, int32_t n_mols_all,
                                                           const int32_t* __restrict__ mol_idx, int32_t B,
                                                           int32_t* __restrict__ atom_off, int32_t* __restrict__ pair_off) {
  __shared__ int sa[256], sp[256];
  const int t = threadIdx.x;
  const int chunk = (B + 255) / 256;
  const int b0 = min(t * chunk, B), b1 = min(b0 + chunk, B);
  int na = 0, np = 0;
  for (int b = b0; b < b1; ++b) {
    const int mi = mol_idx[b];
    const int n = (mi >= 0 && mi < n_mols_all) ? n_atoms_all[mi] : 0;
    na += n;
    np += n * n;
  }
  sa[t] = na;
  sp[t] = np;
  __syncthreads();
  if (t == 0) {
    int ra = 0, rp = 0;
    for (int k = 0; k < 256; ++k) {
      const int xa = sa[k], xp = sp[k];
      sa[k] = ra;
      sp[k] = rp;
      ra += xa;
      rp += xp;
    }
    atom_off[B] = ra;
    pair_off[B] = rp;
  }
  __syncthreads();
  na = sa[t];
  np = sp[t];
  for (int b = b0; b < b1; ++b) {
    const int mi = mol_idx[b];
    const int n = (mi >= 0 && mi < n_mols_all) ? n_atoms_all[mi] : 0;
    atom_off[b] = na;
    pair_off[b] = np;
    na += n;
    np += n * n;
  }
}

// one workgroup per molecule of the batch: its atom numbers and its n x n pairs in row-major (i, j) order
__global__ __launch_bounds__(256) void dtnn_collate_kernel(const int32_t* __restrict__ z_all,
                                                           const float* __restrict__ dist_all,
                                                           const int32_t* __restrict__ n_atoms_all, int32_t n_mols_all,
                                                           int32_t A, const int32_t* __restrict__ mol_idx,
                                                           const int32_t* __restrict__ atom_off,
                                                           const int32_t* __restrict__ pair_off, int32_t n_atoms_cap,
                                                           int64_t n_pairs_cap, int32_t* __restrict__ z,
                                                           float* __restrict__ d, int32_t* __restrict__ mem_i,
                                                           int32_t* __restrict__ mem_j) {
  const int b = blockIdx.x;
  const int mi = mol_idx[b];
  if (mi < 0 || mi >= n_mols_all) return;
  const int n = n_atoms_all[mi];
  const int a0 = atom_off[b];
  const int64_t q0 = pair_off[b];
  if (n <= 0 || n > A || a0 < 0 || a0 + n > n_atoms_cap || q0 < 0 || q0 + (int64_t)n * n > n_pairs_cap) return;
  for (int x = threadIdx.x; x < n; x += blockDim.x) z[a0 + x] = z_all[(int64_t)mi * A + x];
  const float* D = dist_all + (int64_t)mi * A * A;
  for (int q = threadIdx.x; q < n * n; q += blockDim.x) {
    const int i = q / n, j = q - i * n;
    d[q0 + q] = D[i * A + j];
    mem_i[q0 + q] = a0 + i;
    mem_j[q0 + q] = a0 + j;
  }
}

}  // namespace
}  // namespace gcmi

using namespace gcmi;

extern "C" {

int gcmi_dtnn_pair_fwd(const float* d_src, int64_t ld_src, int32_t from_distance, const int32_t* d_mem_i,
                       const int32_t* d_mem_j, int64_t n_pairs, int32_t n_atoms, const float* d_ah, int64_t ldah,
                       int32_t n_hidden, const float* d_w_df, const float* d_b_df, int32_t n_distance,
                       const float* d_w_fc, int32_t n_embedding, double distance_min, double step, float* d_y,
                       int64_t ldy, void* stream) {
  const int rc = check_dtnn("dtnn_pair_fwd", d_src, ld_src, from_distance, d_mem_i, d_mem_j, n_pairs, n_atoms, d_ah, ldah,
                            n_hidden, d_w_df, d_b_df, n_distance, d_w_fc, n_embedding, step);
  if (rc != GCMI_OK) return rc;
  GCMI_CHECK_ARG(ldy >= n_embedding && (n_atoms == 0 || d_y), "dtnn_pair_fwd: bad output");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n_atoms == 0) return GCMI_OK;
  if (hipMemset2DAsync(d_y, ldy * sizeof(float), 0, n_embedding * sizeof(float), n_atoms, st) != hipSuccess) {
    set_error("dtnn_pair_fwd: clearing the output failed");
    return GCMI_ERR_LAUNCH;
  }
  if (n_pairs == 0) return GCMI_OK;
  DtnnArgs a = dtnn_inputs(d_src, ld_src, from_distance, d_mem_i, d_mem_j, n_pairs, n_atoms, d_ah, ldah, n_hidden, d_w_df,
                           d_b_df, n_distance, d_w_fc, n_embedding, distance_min, step);
  a.y = d_y; a.ldy = ldy;
  return dispatch_dtnn<false>(a, from_distance != 0, st);
}

int gcmi_dtnn_pair_bwd(const float* d_src, int64_t ld_src, int32_t from_distance, const int32_t* d_mem_i,
                       const int32_t* d_mem_j, int64_t n_pairs, int32_t n_atoms, const float* d_ah, int64_t ldah,
                       int32_t n_hidden, const float* d_w_df, const float* d_b_df, int32_t n_distance,
                       const float* d_w_fc, int32_t n_embedding, double distance_min, double step, const float* d_dy,
                       int64_t lddy, float* d_dah, int64_t lddah, float* d_dw_df, float* d_db_df, float* d_dw_fc,
                       void* stream) {
  const int rc = check_dtnn("dtnn_pair_bwd", d_src, ld_src, from_distance, d_mem_i, d_mem_j, n_pairs, n_atoms, d_ah, ldah,
                            n_hidden, d_w_df, d_b_df, n_distance, d_w_fc, n_embedding, step);
  if (rc != GCMI_OK) return rc;
  GCMI_CHECK_ARG(lddy >= n_embedding && lddah >= n_hidden && d_dw_df && d_db_df && d_dw_fc &&
                     (n_atoms == 0 || (d_dy && d_dah)),
                 "dtnn_pair_bwd: bad gradient buffers");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n_atoms == 0) return GCMI_OK;
  if (hipMemset2DAsync(d_dah, lddah * sizeof(float), 0, n_hidden * sizeof(float), n_atoms, st) != hipSuccess) {
    set_error("dtnn_pair_bwd: clearing d_ah failed");
    return GCMI_ERR_LAUNCH;
  }
  if (n_pairs == 0) return GCMI_OK;
  DtnnArgs a = dtnn_inputs(d_src, ld_src, from_distance, d_mem_i, d_mem_j, n_pairs, n_atoms, d_ah, ldah, n_hidden, d_w_df,
                           d_b_df, n_distance, d_w_fc, n_embedding, distance_min, step);
  a.dy = d_dy; a.lddy = lddy; a.dah = d_dah; a.lddah = lddah;
  a.dw_df = d_dw_df; a.db_df = d_db_df; a.dw_fc = d_dw_fc;
  return dispatch_dtnn<true>(a, from_distance != 0, st);
}

int gcmi_dtnn_collate(const int32_t* d_z_all, const float* d_dist_all, const int32_t* d_n_atoms_all,
                      int32_t n_mols_all, int32_t max_atoms, const int32_t* d_mol_idx, int32_t n_batch,
                      int32_t n_atoms, int64_t n_pairs, int32_t* d_atom_off, int32_t* d_pair_off, int32_t* d_z,
                      float* d_d, int32_t* d_mem_i, int32_t* d_mem_j, void* stream) {
  GCMI_CHECK_ARG(n_mols_all >= 0 && max_atoms > 0 && max_atoms <= 64 && n_batch >= 0 && n_atoms >= 0 && n_pairs >= 0 &&
                     n_pairs < ((int64_t)1 << 31),
                 "dtnn_collate: bad sizes");
  GCMI_CHECK_ARG(d_atom_off && d_pair_off, "dtnn_collate: NULL offsets");
  GCMI_CHECK_ARG(n_batch == 0 || (d_z_all && d_dist_all && d_n_atoms_all && d_mol_idx), "dtnn_collate: NULL resident set");
  GCMI_CHECK_ARG(n_atoms == 0 || d_z, "dtnn_collate: NULL atom output");
  GCMI_CHECK_ARG(n_pairs == 0 || (d_d && d_mem_i && d_mem_j), "dtnn_collate: NULL pair output");
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(dtnn_offsets_kernel, dim3(1), dim3(256), 0, st, d_n_atoms_all, n_mols_all, d_mol_idx, n_batch,
                     d_atom_off, d_pair_off);
  GCMI_CHECK_LAUNCH("dtnn_offsets");
  if (n_batch == 0) return GCMI_OK;
  hipLaunchKernelGGL(dtnn_collate_kernel, dim3(n_batch), dim3(256), 0, st, d_z_all, d_dist_all, d_n_atoms_all, n_mols_all,
                     max_atoms, d_mol_idx, d_atom_off, d_pair_off, n_atoms, n_pairs, d_z, d_d, d_mem_i, d_mem_j);
  GCMI_CHECK_LAUNCH("dtnn_collate");
  return GCMI_OK;
}

}  // extern "C"
