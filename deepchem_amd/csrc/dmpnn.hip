// D-MPNN (directed message passing, Yang et al. 2019) message aggregation over a batch whose directed bonds are sorted
// by SOURCE atom: atom a owns the contiguous run R(a) = [out_ptr[a], out_ptr[a + 1]) of its outgoing bonds, and rev[b]
// is the position of the reverse bond of b.  The bonds ARRIVING at a are exactly rev[b], b in R(a), so the reference's
//
//     message[mapping][b].sum(1)        (a bonds x max_degree x d gather, then a sum)
//
// is, for b in R(a),   q[b] = S[a] - x[rev[b]],   S[a] = sum over k in R(a) of x[rev[k]]:
// each arriving row is read once per atom and nothing of size bonds x degree exists.
//
// One kernel, two directions (gcmi_dmpnn_message):
//
//   forward      S[a] = sum_{b in R(a)} x[rev[b]]          gathered reads,
//                q[b] = S[a] - x[rev[b]]                   contiguous writes; S and q each optional
//   transposed   T[a] = sum_{b in R(a)} g[b]               contiguous reads,
//                dx[rev[b]] = T[a] - g[b] + dS[a]          scattered whole rows; g or dS may be absent
//
// rev is an involution without fixed points, so the transposed direction writes every bond row exactly once: no
// atomics, and the result does not depend on scheduling.  The transposed direction is the adjoint of the forward one
// (of x -> (q, S) with the cotangents (g, dS)); with only T requested it is the per-atom sum of the outgoing rows.
//
// Layout.  A group of G lanes (G a power of two, 64 / G atoms per wave) owns one atom; a lane owns V = 4 (16-byte
// pieces) or 1 columns per step and walks the row in steps of G * V columns.  The first kDmpnnKeep rows of a run stay
// in registers between the sum and the subtraction (degree <= 4 covers organic molecules); longer runs read the rest
// again, from L2.  An atom without bonds writes a zero S row and nothing else.  Indices are re-checked in the kernel
// (a row outside [0, n_bonds) is skipped): the host validates a batch once, before any launch.
//
// The fused update (gcmi_dmpnn_update_fwd), for d <= 320:
//
//     h[b] = act( input[b] + (S[a] - x[rev[b]]) . W_h^T )          a = the source atom of b, act = none or ReLU
//
// The aggregated rows are the A operand of the product and exist in LDS only.  A wave owns a tile of 32 consecutive
// bond rows.  Per chunk of 64 columns it stages, lane = column, the gathered rows x[rev[k]] of EVERY bond k of the
// atoms its tile touches -- the runs of the first and the last atom may begin before and end after the tile, at most
// 31 rows each at the degree cap of 32, so 94 rows (96 x 68 floats of LDS per wave) always suffice -- and turns every
// run into its aggregated rows in place (sum, then sum - row: each lane reads only what it wrote itself).  The
// tile's 32 rows are then read as MFMA fragments (row on the lane, 8 consecutive k: two ds_read_b128, row pitch 68
// floats), split three ways (split_bf16.h) and multiplied, six v_mfma_f32_32x32x16_bf16 per fragment pair, with the
// weight fragments: W_h is split ONCE per call by a prep kernel into a fragment image in a caller-supplied scratch
// ([k-step][column block][piece][lane] 16-byte entries: one coalesced 1 KB read per wave and fragment, from L2).  The
// accumulators are 32 rows x up to 320 columns per wave (160 registers); the epilogue adds the input rows, applies
// the activation and writes h.  Rows and columns past the edge are zero in both operands.
#include "common.h"
#include "split_bf16.h"

namespace gcmi {
namespace {

constexpr int kDmpnnThreads = 256;
constexpr int kDmpnnKeep = 4;

__device__ __forceinline__ float vsub(float a, float b) { return a - b; }
__device__ __forceinline__ float4 vsub(float4 a, float4 b) {
  return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);
}

struct DmpnnArgs {
  const float* x;  // bond rows read (forward: x; transposed: g); nullptr: zeros (transposed only)
  int64_t ldx;
  const float* add;  // transposed: dS, n_atoms rows added to every written row; nullptr: none
  int64_t ldadd;
  float* s;  // n_atoms rows: the run sums; nullptr: not wanted
  int64_t lds;
  float* q;  // bond rows written; nullptr: not wanted
  int64_t ldq;
  const int32_t* out_ptr;
  const int32_t* rev;
  int32_t n_atoms, n_bonds, d;
  int32_t group;  // lanes per atom
};

// TRANSPOSED = false: rows are READ at rev[b] and written at b; true: read at b and written at rev[b]
template <int V, bool TRANSPOSED>
__global__ __launch_bounds__(kDmpnnThreads) void dmpnn_message_kernel(const DmpnnArgs p) {
  using VT = typename Vec<V>::T;
  const int G = p.group;
  const int per_block = kDmpnnThreads / G;
  const int sub = (int)threadIdx.x / G, lane = (int)threadIdx.x % G;
  for (int64_t a = (int64_t)blockIdx.x * per_block + sub; a < p.n_atoms; a += (int64_t)gridDim.x * per_block) {
    int b0 = p.out_ptr[a], b1 = p.out_ptr[a + 1];
    b0 = b0 < 0 ? 0 : b0;
    b1 = b1 > p.n_bonds ? p.n_bonds : b1;
    for (int c = lane * V; c < p.d; c += G * V) {
      VT keep[kDmpnnKeep];
      VT sum = vzero(VT());
      if (p.x) {
#pragma unroll
        for (int j = 0; j < kDmpnnKeep; ++j) {
          keep[j] = vzero(VT());
          const int b = b0 + j;
          if (b < b1) {
            const int r = TRANSPOSED ? b : p.rev[b];
            if ((unsigned)r < (unsigned)p.n_bonds) keep[j] = *reinterpret_cast<const VT*>(p.x + (int64_t)r * p.ldx + c);
            sum = vadd(sum, keep[j]);
          }
        }
        for (int b = b0 + kDmpnnKeep; b < b1; ++b) {
          const int r = TRANSPOSED ? b : p.rev[b];
          if ((unsigned)r < (unsigned)p.n_bonds) sum = vadd(sum, *reinterpret_cast<const VT*>(p.x + (int64_t)r * p.ldx + c));
        }
      } else {
#pragma unroll
        for (int j = 0; j < kDmpnnKeep; ++j) keep[j] = vzero(VT());
      }
      if (p.s) *reinterpret_cast<VT*>(p.s + a * p.lds + c) = sum;
      if (!p.q) continue;
      VT base = sum;
      if (p.add) base = vadd(base, *reinterpret_cast<const VT*>(p.add + a * p.ldadd + c));
#pragma unroll
      for (int j = 0; j < kDmpnnKeep; ++j) {
        const int b = b0 + j;
        if (b < b1) {
          const int w = TRANSPOSED ? p.rev[b] : b;
          if ((unsigned)w < (unsigned)p.n_bonds) *reinterpret_cast<VT*>(p.q + (int64_t)w * p.ldq + c) = vsub(base, keep[j]);
        }
      }
      for (int b = b0 + kDmpnnKeep; b < b1; ++b) {
        const int r = TRANSPOSED ? b : p.rev[b];
        const int w = TRANSPOSED ? p.rev[b] : b;
        if ((unsigned)r >= (unsigned)p.n_bonds || (unsigned)w >= (unsigned)p.n_bonds) continue;
        VT v = vzero(VT());
        if (p.x) v = *reinterpret_cast<const VT*>(p.x + (int64_t)r * p.ldx + c);
        *reinterpret_cast<VT*>(p.q + (int64_t)w * p.ldq + c) = vsub(base, v);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------- fused update
constexpr int kUpdThreads = 128;
constexpr int kUpdWaves = kUpdThreads / 64;
constexpr int kUpdStage = 96;   // staged rows per wave: 32 + 2 * 31 at the degree cap, rounded up
constexpr int kUpdMaxD = 320;

struct UpdArgs {
  const float* x;  // n_bonds x ldx: the rows that are aggregated
  int64_t ldx;
  const float* inp;  // n_bonds x ldi
  int64_t ldi;
  const u32x4* img;  // fragment image of W_h (dmpnn_wprep_kernel)
  float* h;          // n_bonds x ldh
  int64_t ldh;
  const int32_t *out_ptr, *rev, *src;
  int32_t n_atoms, n_bonds, d, n_tiles, act;
};

// W (d x d, nn.Linear layout, out x in) -> B fragments of h = q . W^T: entry ((ks * NB + nb) * 3 + piece) * 64 + lane holds
// W[32 nb + (lane & 31)][16 ks + 8 (lane >> 5) + 0..7], zero past either edge
__global__ __launch_bounds__(256) void dmpnn_wprep_kernel(const float* __restrict__ w, int64_t ldw, int d, int n_ks,
                                                          int n_nb, u32x4* __restrict__ img) {
  const int total = n_ks * n_nb * 64;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    const int lane = idx & 63, f = idx >> 6;
    const int nb = f % n_nb, ks = f / n_nb;
    const int n = 32 * nb + (lane & 31), k0 = 16 * ks + 8 * (lane >> 5);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (n < d && k0 + j < d) ? w[(int64_t)n * ldw + k0 + j] : 0.f;
    const Frag3 fr = split_frag(v);
#pragma unroll
    for (int p = 0; p < 3; ++p) img[((int64_t)f * 3 + p) * 64 + lane] = fr.p[p];
  }
}

template <int NB>
__global__ __launch_bounds__(kUpdThreads) void dmpnn_update_kernel(const UpdArgs a) {
  __shared__ __attribute__((aligned(16))) float upd_smem[kUpdWaves][kUpdStage * kTilePitch];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
  float* X = upd_smem[wave];
  const int n_chunks = (a.d + 63) / 64, n_ks = (a.d + 15) / 16, n_nb = (a.d + 31) / 32;
  const int per_pass = (int)gridDim.x * kUpdWaves;
  const int passes = (a.n_tiles + per_pass - 1) / per_pass;  // the same for every wave: the barriers below are uniform
  for (int pass = 0; pass < passes; ++pass) {
    const int tile = (pass * (int)gridDim.x + (int)blockIdx.x) * kUpdWaves + wave;
    const bool active = tile < a.n_tiles;
    int r0 = 0, valid = 0, s0 = 0, n_stage = 0;
    if (active) {
      r0 = tile * 32;
      valid = a.n_bonds - r0 < 32 ? a.n_bonds - r0 : 32;
      int a_lo = a.src[r0], a_hi = a.src[r0 + valid - 1];
      a_lo = a_lo < 0 ? 0 : (a_lo >= a.n_atoms ? a.n_atoms - 1 : a_lo);
      a_hi = a_hi < a_lo ? a_lo : (a_hi >= a.n_atoms ? a.n_atoms - 1 : a_hi);
      s0 = a.out_ptr[a_lo];
      int s1 = a.out_ptr[a_hi + 1];
      s0 = s0 < 0 ? 0 : (s0 > r0 ? r0 : s0);
      s1 = s1 > a.n_bonds ? a.n_bonds : (s1 < r0 + valid ? r0 + valid : s1);
      n_stage = s1 - s0 < kUpdStage ? s1 - s0 : kUpdStage;  // (more than 94 only above the degree cap: the host refuses that)
    }
    f32x16 acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;
    for (int kc = 0; kc < n_chunks; ++kc) {
      if (active) {  // stage the gathered rows, lane = column, and aggregate every run in place
        const int c = kc * 64 + lane;
        const bool in = c < a.d;
        int i = 0;
        while (i < n_stage) {
          int at = a.src[s0 + i];
          at = at < 0 ? 0 : (at >= a.n_atoms ? a.n_atoms - 1 : at);
          int e = a.out_ptr[at + 1] - s0;
          e = e <= i ? i + 1 : (e > n_stage ? n_stage : e);
          float sum = 0.f;
          for (int j = i; j < e; ++j) {
            const int r = a.rev[s0 + j];
            const float v = (in && (unsigned)r < (unsigned)a.n_bonds) ? a.x[(int64_t)r * a.ldx + c] : 0.f;
            X[j * kTilePitch + lane] = v;
            sum += v;
          }
          for (int j = i; j < e; ++j) X[j * kTilePitch + lane] = sum - X[j * kTilePitch + lane];
          i = e;
        }
      }
      __syncthreads();
      if (active) {
        const int row = r0 - s0 + l31;
        const bool have = l31 < valid && row < n_stage;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const int ks = kc * 4 + kk;
          if (ks < n_ks) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = 0.f;
            if (have) {
              const float4* src = reinterpret_cast<const float4*>(X + row * kTilePitch + kk * 16 + 8 * half);
              const float4 u0 = src[0], u1 = src[1];
              v[0] = u0.x; v[1] = u0.y; v[2] = u0.z; v[3] = u0.w;
              v[4] = u1.x; v[5] = u1.y; v[6] = u1.z; v[7] = u1.w;
            }
            const Frag3 fa = split_frag(v);
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
              if (nb < n_nb) {
                mfma_split6(acc[nb], fa, load_frag3(a.img + ((int64_t)(ks * n_nb + nb) * 3) * 64 + lane));
              }
            }
          }
        }
      }
      __syncthreads();  // the next chunk overwrites the staged rows
    }
    if (active) {
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const int n = 32 * nb + l31;
        if (n < a.d) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int m = acc_row(r, half);
            if (m < valid) {
              float v = a.inp[(int64_t)(r0 + m) * a.ldi + n] + acc[nb][r];
              if (a.act) v = v > 0.f ? v : 0.f;
              a.h[(int64_t)(r0 + m) * a.ldh + n] = v;
            }
          }
        }
      }
    }
  }
}

template <int NB>
void launch_update(const UpdArgs& a, int grid, hipStream_t st) {
  hipLaunchKernelGGL((dmpnn_update_kernel<NB>), dim3(grid), dim3(kUpdThreads), 0, st, a);
}

inline int64_t update_scratch_floats(int d) { return (int64_t)((d + 15) / 16) * ((d + 31) / 32) * 3 * 64 * 4; }

}  // namespace
}  // namespace gcmi

using namespace gcmi;

extern "C" {

int gcmi_dmpnn_message(int32_t transposed, const float* d_x, int64_t ldx, int32_t d, const int32_t* d_out_ptr,
                       const int32_t* d_rev, int32_t n_atoms, int32_t n_bonds, const float* d_add, int64_t ldadd,
                       float* d_s, int64_t lds, float* d_q, int64_t ldq, void* stream) {
  GCMI_CHECK_ARG(transposed == 0 || transposed == 1, "dmpnn_message: transposed must be 0 or 1");
  GCMI_CHECK_ARG(d >= 1 && n_atoms >= 0 && n_bonds >= 0, "dmpnn_message: bad shape (d %d, atoms %d, bonds %d)", d,
                 n_atoms, n_bonds);
  GCMI_CHECK_ARG(d_s || d_q, "dmpnn_message: NULL outputs (neither the atom sums nor the bond rows are wanted)");
  GCMI_CHECK_ARG(d_out_ptr && d_rev, "dmpnn_message: NULL out_ptr / rev");
  GCMI_CHECK_ARG(transposed ? (d_x || d_add) : d_x != nullptr, "dmpnn_message: NULL input rows");
  GCMI_CHECK_ARG(transposed || !d_add, "dmpnn_message: the added atom rows belong to the transposed direction");
  GCMI_CHECK_ARG((!d_x || ldx >= d) && (!d_add || ldadd >= d) && (!d_s || lds >= d) && (!d_q || ldq >= d),
                 "dmpnn_message: ld < d");
  GCMI_CHECK_ARG(aligned4(d_x) && aligned4(d_add) && aligned4(d_s) && aligned4(d_q) && aligned4(d_out_ptr) &&
                     aligned4(d_rev),
                 "dmpnn_message: a buffer is not 4-byte aligned");
  GCMI_CHECK_ARG(!d_q || d_q != d_x, "dmpnn_message: the bond rows cannot be written in place");
  if (n_atoms == 0) return GCMI_OK;
  if (n_bonds == 0) {  // no kernel: the atom sums of a batch without bonds are zero rows
    if (d_s && hipMemset2DAsync(d_s, (size_t)lds * sizeof(float), 0, (size_t)d * sizeof(float), (size_t)n_atoms,
                                (hipStream_t)stream) != hipSuccess) {
      (void)hipGetLastError();
      set_error("dmpnn_message: clearing the atom sums failed");
      return GCMI_ERR_LAUNCH;
    }
    return GCMI_OK;
  }
  const bool v4 = d % 4 == 0 && (!d_x || vec_width(d_x, ldx, d) == 4) && (!d_add || vec_width(d_add, ldadd, d) == 4) &&
                  (!d_s || vec_width(d_s, lds, d) == 4) && (!d_q || vec_width(d_q, ldq, d) == 4);
  const int steps = v4 ? d / 4 : d;
  int group = 1;
  while (group < 64 && group < steps) group *= 2;
  DmpnnArgs p{d_x, ldx, d_add, ldadd, d_s, lds, d_q, ldq, d_out_ptr, d_rev, n_atoms, n_bonds, d, group};
  const int per_block = kDmpnnThreads / group;
  const dim3 grid(grid_for(((int64_t)n_atoms + per_block - 1) / per_block * kDmpnnThreads, kDmpnnThreads));
  hipStream_t st = (hipStream_t)stream;
  if (v4 && transposed)
    hipLaunchKernelGGL((dmpnn_message_kernel<4, true>), grid, dim3(kDmpnnThreads), 0, st, p);
  else if (v4)
    hipLaunchKernelGGL((dmpnn_message_kernel<4, false>), grid, dim3(kDmpnnThreads), 0, st, p);
  else if (transposed)
    hipLaunchKernelGGL((dmpnn_message_kernel<1, true>), grid, dim3(kDmpnnThreads), 0, st, p);
  else
    hipLaunchKernelGGL((dmpnn_message_kernel<1, false>), grid, dim3(kDmpnnThreads), 0, st, p);
  GCMI_CHECK_LAUNCH("dmpnn_message");
  return GCMI_OK;
}

int gcmi_dmpnn_update_fwd(const float* d_x, int64_t ldx, const float* d_input, int64_t ldi, const float* d_w, int64_t ldw,
                          int32_t d_hidden, int32_t act, const int32_t* d_out_ptr, const int32_t* d_rev,
                          const int32_t* d_bond_src, int32_t n_atoms, int32_t n_bonds, float* d_img_scratch,
                          int64_t scratch_floats, float* d_h, int64_t ldh, void* stream) {
  GCMI_CHECK_ARG(d_hidden >= 1 && n_atoms >= 0 && n_bonds >= 0, "dmpnn_update_fwd: bad shape (d_hidden %d, atoms %d, bonds %d)",
                 d_hidden, n_atoms, n_bonds);
  GCMI_CHECK_ARG(act == 0 || act == 1, "dmpnn_update_fwd: act must be 0 (none) or 1 (ReLU)");
  GCMI_CHECK_ARG(d_x && d_input && d_w && d_out_ptr && d_rev && d_bond_src && d_img_scratch && d_h,
                 "dmpnn_update_fwd: NULL buffer");
  GCMI_CHECK_ARG(ldx >= d_hidden && ldi >= d_hidden && ldw >= d_hidden && ldh >= d_hidden, "dmpnn_update_fwd: ld < d");
  GCMI_CHECK_ARG(aligned4(d_x) && aligned4(d_input) && aligned4(d_w) && aligned4(d_h) && aligned4(d_out_ptr) &&
                     aligned4(d_rev) && aligned4(d_bond_src) && aligned16(d_img_scratch),
                 "dmpnn_update_fwd: a buffer is not 4-byte aligned (the scratch: 16-byte)");
  GCMI_CHECK_ARG(d_h != d_x, "dmpnn_update_fwd: the aggregated rows cannot be overwritten in place");
  if (d_hidden > kUpdMaxD) {
    set_error("dmpnn_update_fwd: d_hidden %d above %d: no other kernel stands behind this entry (run the message kernel and "
              "the segmented product)", d_hidden, kUpdMaxD);
    return GCMI_ERR_UNSUPPORTED;
  }
  GCMI_CHECK_ARG(scratch_floats >= update_scratch_floats(d_hidden), "dmpnn_update_fwd: scratch of %lld floats, %lld needed",
                 (long long)scratch_floats, (long long)update_scratch_floats(d_hidden));
  if (n_bonds == 0 || n_atoms == 0) return GCMI_OK;
  hipStream_t st = (hipStream_t)stream;
  const int n_ks = (d_hidden + 15) / 16, n_nb = (d_hidden + 31) / 32;
  u32x4* img = reinterpret_cast<u32x4*>(d_img_scratch);
  hipLaunchKernelGGL(dmpnn_wprep_kernel, dim3(grid_for((int64_t)n_ks * n_nb * 64, 256)), dim3(256), 0, st, d_w, ldw,
                     d_hidden, n_ks, n_nb, img);
  GCMI_CHECK_LAUNCH("dmpnn_wprep");
  const int n_tiles = (n_bonds + 31) / 32;
  UpdArgs a{d_x, ldx, d_input, ldi, img, d_h, ldh, d_out_ptr, d_rev, d_bond_src, n_atoms, n_bonds, d_hidden, n_tiles, act};
  const int grid = std::max(1, std::min((n_tiles + kUpdWaves - 1) / kUpdWaves, 2048));
  if (n_nb <= 1) launch_update<1>(a, grid, st);
  else if (n_nb <= 2) launch_update<2>(a, grid, st);
  else if (n_nb <= 3) launch_update<3>(a, grid, st);
  else if (n_nb <= 5) launch_update<5>(a, grid, st);
  else if (n_nb <= 8) launch_update<8>(a, grid, st);
  else launch_update<10>(a, grid, st);
  GCMI_CHECK_LAUNCH("dmpnn_update_fwd");
  return GCMI_OK;
}

}  // extern "C"
