// Forward product of a GraphConv / dense block over activations STORED AS bf16 (gcmi_model_desc.storage == 1):
//
//     out = relu([S | X] . [W_rel[d]; W_self[d]] + b[d])        GraphConv.forward (models/torch_models/layers.py:6204-6246)
//     out = relu(P . W^T + b)                                   nn.Linear + ReLU (graphconvmodel.py:222-223)
//
// plus, for the training forward, the column sums of out and out^2 (of the ROUNDED values: the statistics describe
// what is stored and what the backward reads) for the BatchNorm that follows.
//
// What bf16 storage changes against fwd_fused.hip, beyond half the bytes per row:
//   * a stored operand IS its own first bf16 piece: no three-way split of the activations (the vector work that bounds
//     the fp32 kernels), and the product needs the weight pieces x ONE operand piece = 3 MFMAs per k-step instead of 6
//     (fp32 weights split exactly as before, fp32 accumulation);
//   * the operand tile goes to LDS as it arrives (16-byte pieces of 8 elements, no conversion) and a fragment of
//     v_mfma_f32_32x32x16_bf16 is ONE ds_read_b128: half the LDS traffic and a quarter of the fragment instructions;
//   * LDS per workgroup is 25-35 KB (operand tile + output tile, the weight fragments live in registers as in
//     fwd_reg_kernel), so three or four four-wave workgroups share a CU and one's loads, stores and barriers overlap the
//     others' products.
// The weights are the matrix core's A operand and the activations its B operand, so the accumulator holds out^T
// (lane = row of the tile, registers = four runs of four consecutive output columns): bias, ReLU and the rounding are
// applied there, a lane writes 8-byte pieces of its row to an LDS output tile, and the tile leaves as whole rows
// (16 bytes per lane) at the start of the next iteration, where the BatchNorm sums are taken from the rounded values.
#include "common.h"
#include "split_bf16.h"

namespace gcmi {

struct FwdHArgs {
  const bf16_t* in[2];
  int32_t ldin[2];       // elements, multiples of 8; columns [k_in, KO) of the rows are zero (or absent: ld < KO)
  int32_t k_in;          // columns of every operand (<= KO)
  const float* w[2];
  const float* bias;
  void* out;             // bf16 rows, or fp32 rows (the kernel's F32OUT form)
  int32_t ldo;           // elements, multiple of 8
  int32_t relu;
  double* stats;         // bn.hip scratch layout, or nullptr
  const u32x4* wimg;     // the segments' weight fragments, split and in lane order (wprep_kernel below)
#ifdef GCMI_FWD_H_DIAG_BUILD  // diagnostic build only (tools/fwd_h_diag.sh): phase switches and phase clocks
  int32_t diag_flags;    // 1 no products, 2 no global stores, 4 no operand loads, 8 no epilogue
  unsigned long long* diag_out;
#endif
};

// ---- weight fragments, prepared once per launch.  The kernels keep a wave's weight fragments in registers and reload
// them when its tile range crosses into another degree's segment.  Read from the fp32 parameter block that is eight
// strided dword loads per fragment and lane, which the compiler (short of registers) issues one at a time, each behind
// a full wait: 64 dependent L2 round trips per segment change, 20-40 us that EVERY workgroup pays at its start.  This
// kernel splits every fragment of every segment once -- [segment][32-column tile][k-step][piece][lane] 16-byte entries
// -- so that a reload is NKS * 3 coalesced 1 KiB wave loads with one wait behind them.
template <bool TRANS>
__global__ void __launch_bounds__(256)
wprep_kernel(SegTable st, const float* __restrict__ w0, const float* __restrict__ w1, int k_in, int KO, int NOPS,
             int NOUT, u32x4* __restrict__ wimg) {
  const int NKS = NOPS * KO / 16, TW = NOUT / 32;
  const int total = st.n_seg * TW * NKS * 64;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    const int lane = e & 63;
    int t = e >> 6;
    const int ks = t % NKS; t /= NKS;
    const int tw = t % TW;
    const int seg = t / TW;
    const int n = tw * 32 + (lane & 31);
    const int c0 = ks * 16 + 8 * (lane >> 5);
    const int o = c0 >= KO ? 1 : 0;
    const int ck0 = c0 - o * KO;
    const int64_t woff = o == 1 ? pick_n(st.w_off[1], seg) : pick_n(st.w_off[0], seg);
    const float* w = o == 1 ? w1 : w0;
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int ck = ck0 + q;
      const bool ok = woff >= 0 && ck < k_in && w != nullptr;
      v[q] = ok ? (TRANS ? w[woff + (int64_t)n * k_in + ck] : w[woff + (int64_t)ck * NOUT + n]) : 0.f;
    }
    const Frag3 f = split_frag(v);
    u32x4* dst = wimg + (size_t)((seg * TW + tw) * NKS + ks) * 3 * 64 + lane;
    store_frag3(dst, f);
  }
}

// ------------------------------------------------------------------------------------------------------------------
// The product, with the operand rows brought in by LDS-DMA, two tiles ahead.
// One tile of prefetch per workgroup in registers (the retired fwd_h_kernel) ran at memory latency: with two four-wave
// workgroups per CU an iteration was load issue -> ~0.5 us of products -> wait for loads that were issued half a
// microsecond ago (~4 us per tile and workgroup, measured 150-190 us per launch = 3 TB/s).  Here the rows go
// HBM -> LDS directly (global_load_lds_dwordx4: no registers, per-lane source address, lane-linear LDS image) into a
// ring of D + 1 tile buffers, D tiles ahead, and a tile is waited for with a COUNTED s_waitcnt: the memory queue is in
// order, so "all but the youngest D * (stores of one tile) + (D - 1) * (loads of one tile)" is exactly "tile i has
// landed".  For that count to hold every tile issues the same number of loads and stores: a tile beyond the
// workgroup's last one is loaded again into a buffer nobody reads, rows beyond a ragged tile's end are stored to a
// per-thread dump slot.
// The LDS image has no padding (the DMA writes 64 consecutive 16-byte chunks per wave instruction); bank conflicts of
// the fragment reads (ds_read_b128: 16 lanes per cycle, one 16-byte chunk = one "bank quad" each) are avoided by the
// SOURCE side instead: chunk position jpos of row r holds piece j = jpos ^ f(r) of that row, f chosen per row length so
// that the 16 rows of a read group hit 16 different bank quads (RQ 16: r & 15; RQ 20: (r >> 2) & 3, which stays inside
// an aligned group of four pieces; RQ 8: (r >> 1) & 7).
typedef __attribute__((address_space(3))) void* lds_ptr_h;
__device__ __forceinline__ void glds16_h(const void* gsrc, unsigned lds_dst) {
  unsigned keep;
  lds_dst = __builtin_amdgcn_readfirstlane(lds_dst);  // wave-uniform by construction
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}

__device__ u32x4 g_fwdh_dump[512 * 256];  // where the rows beyond a ragged tile's end are stored: one slot per thread

// NOPS operands of KO (padded) columns each, NOUT output columns, NPW = 3 bf16 pieces kept of every weight (exact to
// 2^-24); TRANS: weights stored NOUT x k_in (nn.Linear)
// F32OUT: the operands are bf16 rows that hold their values EXACTLY (the first GraphConv over small-integer atom
// features, fp32 storage: model.hip), so nothing of the product is lost against the split-fp32 kernels and the output
// stays fp32 -- rows of 16-byte pieces of FOUR columns, the BatchNorm sums taken from the unrounded values.
template <int NOPS, int KO, int NOUT, bool TRANS, bool F32OUT = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
fwd_hd_kernel(SegTable st, int n_tiles, FwdHArgs a, int rev) {
  constexpr int NT = 256, ROWS = 64, D = 2, NBUF = D + 1, NPW = 3;
  constexpr int NC = NOPS * KO;
  constexpr int NKS = NC / 16;
  constexpr int TW = NOUT / 32, TPW = TW / 2;
  static_assert(TW % 2 == 0 && KO % 8 == 0 && NC % 16 == 0, "tile shapes");
  constexpr int IQ = KO / 8, RQ = NOPS * IQ;            // 16-byte pieces of an operand row / of a tile row
  static_assert(RQ == 8 || RQ == 16 || RQ == 20, "a swizzle exists for these row lengths");
  constexpr int TILE_CHUNKS = ROWS * RQ;
  constexpr int TILE_BYTES = TILE_CHUNKS * 16;
  constexpr int LPW = TILE_CHUNKS / NT;                  // DMA instructions per wave and tile
  static_assert(TILE_CHUNKS % NT == 0, "tile loads divide evenly");
  constexpr int OES = F32OUT ? 4 : 2;                    // bytes of an output element
  constexpr int OPC = 16 / OES;                          // columns of a 16-byte output piece
  constexpr int OPB = NOUT * OES + 16, OQ = NOUT / OPC, OPASS = ROWS * OQ / NT;
  static_assert(ROWS * OQ % NT == 0 && NT % OQ == 0, "a thread keeps its column piece over the passes");
  constexpr int kWaitSteady = D * OPASS + (D - 1) * LPW;  // younger than tile i's loads when iteration i starts
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  unsigned char* As = lds_raw;                                         // [NBUF][ROWS][RQ] chunks
  unsigned char* Outs = lds_raw + (size_t)NBUF * TILE_BYTES;           // [ROWS][OPB]
  __shared__ SegTableLds tl;
  __shared__ __attribute__((aligned(16))) float bias_s[NOUT];
  __shared__ double stat_s[2][NOUT];

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int half = lane >> 5;
  const int l31 = lane & 31;
  const int rb = wave & 1, twb = wave >> 1;
  auto swz = [](int r) { return RQ == 16 ? (r & 15) : RQ == 20 ? ((r >> 2) & 3) : ((r >> 1) & 7); };

  tl.fill(st);
  for (int c = tid; c < 2 * NOUT; c += NT) stat_s[c / NOUT][c % NOUT] = 0.0;
  __syncthreads();

  const TileRange tiles = tile_range<true>(n_tiles, rev);
  const int my_tiles = tiles.count();
  SegCursor cur_issue, cur_run;  // of the tile being requested, D tiles ahead, and of the tile being multiplied
  cur_issue.init(tl, st.n_seg, tiles.at(0));
  cur_run = cur_issue;
  const unsigned as_base = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lds_ptr_h)As);

  // ---- LDS-DMA of tile `it` (clamped to the workgroup's last tile) into ring buffer it % NBUF: LPW instructions per
  // wave, always.  Rows beyond a ragged tile's end re-read its last row (finite values, never stored).
  // what does not depend on the tile is formed once: this lane's row of the tile, its byte column and its operand for
  // each of the LPW instructions of a tile
  int d_row[LPW];
  unsigned d_col[LPW], d_ldb[LPW];
  const char* d_base[LPW];
#pragma unroll
  for (int p = 0; p < LPW; ++p) {
    const int c = (p * 4 + wave) * 64 + lane;  // instruction t = 4 p + wave covers chunks [64 t, 64 t + 64)
    const int r = c / RQ, jpos = c - r * RQ;
    const int j = jpos ^ swz(r);
    const int o = NOPS == 2 ? (j >= IQ ? 1 : 0) : 0;
    const int q = j - o * IQ;
    const int ld = o == 1 ? a.ldin[1] : a.ldin[0];
    d_row[p] = r;
    d_col[p] = (unsigned)(8 * q + 8 <= ld ? 8 * q : 0) * 2u;
    d_ldb[p] = (unsigned)ld * 2u;
    d_base[p] = reinterpret_cast<const char*>(o == 1 ? a.in[1] : a.in[0]);
  }
  auto issue_tile = [&](int it) {
    int row0_, valid_;
    cur_issue.seek<ROWS>(tl, tiles.at(it < my_tiles ? it : my_tiles - 1), row0_, valid_);
    const unsigned buf = as_base + (unsigned)(it % NBUF) * TILE_BYTES + (unsigned)wave * 1024u;
#pragma unroll
    for (int p = 0; p < LPW; ++p) {
      const int rc = d_row[p] < valid_ ? d_row[p] : valid_ - 1;
      const unsigned off = (unsigned)(row0_ + rc) * d_ldb[p] + d_col[p];
      glds16_h(d_base[p] + off, buf + (unsigned)p * 4096u);
    }
  };

  u32x4 wf[TPW][NKS][NPW];
  auto load_w = [&](int seg_) {
    // (wprep_kernel's images: [segment][32-column tile][k-step][piece][lane])
    const u32x4* base = a.wimg + (size_t)seg_ * TW * NKS * 3 * 64 + lane;
#pragma unroll
    for (int j = 0; j < TPW; ++j)
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
        for (int pc = 0; pc < NPW; ++pc)
          wf[j][ks][pc] = base[(size_t)(((twb + 2 * j) * NKS + ks) * 3 + pc) * 64];
  };

  float ps1[OPC], ps2[OPC];
#pragma unroll
  for (int i = 0; i < OPC; ++i) ps1[i] = ps2[i] = 0.f;
  auto flush_stats = [&]() {
    const int q = tid % OQ;
#pragma unroll
    for (int i = 0; i < OPC; ++i) {
      atomicAdd(&stat_s[0][OPC * q + i], (double)ps1[i]);
      atomicAdd(&stat_s[1][OPC * q + i], (double)ps2[i]);
      ps1[i] = ps2[i] = 0.f;
    }
  };
  u32x4* const my_dump = &g_fwdh_dump[(blockIdx.x % 512) * 256 + tid];
  // OPASS stores per thread, always (rows beyond the tile's end go to the dump slot): the counted wait above relies on it
  auto store_out = [&](int row0_, int valid_) {
#pragma unroll
    for (int p = 0; p < OPASS; ++p) {
      const int slot = tid + p * NT;
      const int r = slot / OQ, q = slot - r * OQ;
      const bool live = r < valid_;
      const u32x4 v = *reinterpret_cast<const u32x4*>(Outs + r * OPB + q * 16);
      const unsigned off = ((unsigned)(row0_ + r) * (unsigned)a.ldo + (unsigned)OPC * q) * (unsigned)OES;
      u32x4* dst = live ? reinterpret_cast<u32x4*>(reinterpret_cast<char*>(a.out) + off) : my_dump;
      *dst = v;
      if (a.stats != nullptr && live) {
        float f[OPC];
        if constexpr (F32OUT) {
          f[0] = __uint_as_float(v.x); f[1] = __uint_as_float(v.y);
          f[2] = __uint_as_float(v.z); f[3] = __uint_as_float(v.w);
        } else {
          widen8(uint4{v.x, v.y, v.z, v.w}, f);
        }
#pragma unroll
        for (int i = 0; i < OPC; ++i) {
          ps1[i] += f[i];
          ps2[i] = fmaf(f[i], f[i], ps2[i]);
        }
      }
    }
  };

  const int my_row = rb * 32 + l31;
  const int my_swz = swz(my_row);
  auto products = [&](int it) {
    f32x16 acc[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j) acc[j] = zero_acc();
    const unsigned char* arow = As + (size_t)(it % NBUF) * TILE_BYTES + (size_t)my_row * RQ * 16;
    auto frag = [&](int ks) { return *reinterpret_cast<const u32x4*>(arow + (((2 * ks + half) ^ my_swz) * 16)); };
    u32x4 xa = frag(0);
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      const u32x4 x = xa;
      if (ks + 1 < NKS) xa = frag(ks + 1);
#pragma unroll
      for (int j = 0; j < TPW; ++j) {
#pragma unroll
        for (int pc = NPW - 1; pc >= 0; --pc)
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(wf[j][ks][pc]), as_bf16x8(x), acc[j], 0, 0, 0);
      }
    }
    unsigned char* orow = Outs + my_row * OPB;
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c0 = (twb + 2 * j) * 32 + 8 * g + 4 * half;
        const float4 bv = *reinterpret_cast<const float4*>(bias_s + c0);
        float v0 = acc[j][4 * g + 0] + bv.x, v1 = acc[j][4 * g + 1] + bv.y;
        float v2 = acc[j][4 * g + 2] + bv.z, v3 = acc[j][4 * g + 3] + bv.w;
        if (a.relu) {
          v0 = v0 > 0.f ? v0 : 0.f; v1 = v1 > 0.f ? v1 : 0.f;
          v2 = v2 > 0.f ? v2 : 0.f; v3 = v3 > 0.f ? v3 : 0.f;
        }
        if constexpr (F32OUT) *reinterpret_cast<float4*>(orow + c0 * 4) = make_float4(v0, v1, v2, v3);
        else *reinterpret_cast<uint2*>(orow + c0 * 2) = narrow4(v0, v1, v2, v3);
      }
    }
  };

#ifdef GCMI_FWD_H_DIAG_BUILD
  const int dflags = a.diag_flags;
  const bool stamp = a.diag_out != nullptr && blockIdx.x == 0 && tid == 0;
  unsigned long long tk[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t0 = 0, t1 = 0;
#define DIAG_T(k) do { if (stamp) { t1 = __builtin_amdgcn_s_memtime(); tk[k] += t1 - t0; t0 = t1; } } while (0)
#define DIAG_ON(bit) (!(dflags & (bit)))
#else
#define DIAG_T(k) do { } while (0)
#define DIAG_ON(bit) true
#endif
#pragma unroll
  for (int d = 0; d < D; ++d) issue_tile(d);
  int cur_seg = -1;
#ifdef GCMI_FWD_H_DIAG_BUILD
  if (stamp) t0 = __builtin_amdgcn_s_memtime();
#endif
  for (int i = 0; i < my_tiles; ++i) {
    int row0, valid;
    const int seg = cur_run.seek<ROWS>(tl, tiles.at(i), row0, valid);
    DIAG_T(0);
    // tile i has landed: in the steady state all but the D * OPASS stores and (D - 1) * LPW loads issued after its loads;
    // the first D iterations (no stores of earlier tiles in the queue yet) simply wait for everything
    if (i < D) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kWaitSteady) : "memory");
    DIAG_T(1);
    if (seg != cur_seg) {  // uniform; everyone passed the barrier that ended the previous tile's products
      const int64_t boff = tl.b[seg];
      for (int n = tid; n < NOUT; n += NT) bias_s[n] = (a.bias != nullptr && boff >= 0) ? a.bias[boff + n] : 0.f;
    }
    __syncthreads();  // every wave's part of tile i is in LDS; buffer (i + D) % NBUF (tile i - 1) and Outs are free
    DIAG_T(2);
    if (DIAG_ON(4)) issue_tile(i + D);
    DIAG_T(3);
    if (seg != cur_seg) {
      cur_seg = seg;
      load_w(seg);
    }
    if (DIAG_ON(1)) products(i);
    DIAG_T(4);
    __syncthreads();
    DIAG_T(5);
    if (DIAG_ON(2)) store_out(row0, valid);
    if (a.stats != nullptr && (i & 31) == 31) flush_stats();  // fp32 partials over <= 32 tiles x OPASS rows, then fp64
    DIAG_T(6);
  }
#ifdef GCMI_FWD_H_DIAG_BUILD
  if (stamp) {
    for (int k = 0; k < 7; ++k) a.diag_out[k] = tk[k];
    a.diag_out[7] = (unsigned long long)my_tiles;
  }
#endif
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the look-ahead loads of tiles beyond the last one
  if (a.stats != nullptr) {
    flush_stats();
    __syncthreads();
    for (int c = tid; c < 2 * NOUT; c += NT) {
      const int which = c / NOUT, col = c - which * NOUT;
      atomicAdd(a.stats + (size_t)2 * NOUT * (1 + (blockIdx.x % kBnReplicas)) + (size_t)which * NOUT + col,
                stat_s[which][col]);
    }
  }
}

template <int NOPS, int KO, int NOUT, bool TRANS, bool F32OUT = false>
static int launch_fwd_hd(const SegTable& st, int n_tiles, const FwdHArgs& a, hipStream_t sm) {
  constexpr int RQ = NOPS * KO / 8;
  const size_t shmem = (size_t)3 * 64 * RQ * 16 + (size_t)64 * (NOUT * (F32OUT ? 4 : 2) + 16);
  auto kern = fwd_hd_kernel<NOPS, KO, NOUT, TRANS, F32OUT>;
  static LdsLimit lim;  // per instantiation
  const int occ = raise_lds_limit(lim, reinterpret_cast<const void*>(kern), shmem, 256, shmem);
  if (!occ) return GCMI_ERR_UNSUPPORTED;
  const int per_cu = std::min(occ, 2);  // (g_fwdh_dump is sized for 512 workgroups)
  const int grid = std::min(n_tiles, 256 * per_cu);
#ifdef GCMI_FWD_H_DIAG_BUILD
  static unsigned long long* d_diag = nullptr;
  static const int dflags = getenv("GCMI_FWD_H_DIAG") ? atoi(getenv("GCMI_FWD_H_DIAG")) : 0;
  FwdHArgs aa = a;
  if (!d_diag && hipMalloc(&d_diag, 8 * sizeof(unsigned long long)) != hipSuccess) d_diag = nullptr;
  aa.diag_flags = dflags;
  aa.diag_out = d_diag;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), shmem, sm, st, n_tiles, aa, next_sweep_direction());
  GCMI_CHECK_LAUNCH("fwd_hd");
  static int printed = 0;
  if (d_diag && printed < 12) {  // serialises the stream: diagnostics only
    unsigned long long h[8];
    if (hipStreamSynchronize(sm) == hipSuccess && hipMemcpy(h, d_diag, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess && h[7])
      fprintf(stderr, "fwd_hd<%d,%d,%d> flags %d tiles %llu | cycles per tile: tile_info %.0f wait %.0f barrierA %.0f issue %.0f "
                      "products %.0f barrierB %.0f store %.0f\n", NOPS, KO, NOUT, dflags, h[7], (double)h[0] / h[7],
              (double)h[1] / h[7], (double)h[2] / h[7], (double)h[3] / h[7], (double)h[4] / h[7], (double)h[5] / h[7],
              (double)h[6] / h[7]);
    ++printed;
  }
  return GCMI_OK;
#else
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), shmem, sm, st, n_tiles, a, next_sweep_direction());
  GCMI_CHECK_LAUNCH("fwd_hd");
  return GCMI_OK;
#endif
}

// The same images for a caller outside this file (fwd_fused.hip's fwd_reg_kernel): [segment][32-column tile][k-step]
// [piece][lane] 16-byte entries, (n_seg * (n_out / 32) * (n_ops * ko / 16) * 3 * 64) of them, in d_scratch.
int fwd_weight_images(int32_t n_seg, const int64_t* w1_off, const int64_t* w2_off, const float* d_w1, const float* d_w2,
                      int32_t k_in, int32_t ko, int32_t n_ops, int32_t n_out, int32_t trans_w, float* d_scratch,
                      hipStream_t sm) {
  if (n_seg > kMaxProductSeg || d_scratch == nullptr || !aligned16(d_scratch)) return GCMI_ERR_UNSUPPORTED;
  if ((int64_t)n_seg * (n_out / 32) * (n_ops * ko / 16) * 3 * 256 > kFwdHWimgFloats) return GCMI_ERR_UNSUPPORTED;
  SegTable st;  // (wprep_kernel reads n_seg and the weight offsets only: no bounds, no bias)
  fill_seg_table(st, n_seg, nullptr, nullptr, w1_off, n_ops == 2 ? w2_off : nullptr, nullptr, 64);
  const int entries = n_seg * (n_out / 32) * (n_ops * ko / 16) * 64;
  const int blocks = std::min((entries + 255) / 256, 1024);
  u32x4* wimg = reinterpret_cast<u32x4*>(d_scratch);
  if (trans_w)
    hipLaunchKernelGGL(wprep_kernel<true>, dim3(blocks), dim3(256), 0, sm, st, d_w1, d_w2, k_in, ko, n_ops, n_out, wimg);
  else
    hipLaunchKernelGGL(wprep_kernel<false>, dim3(blocks), dim3(256), 0, sm, st, d_w1, d_w2, k_in, ko, n_ops, n_out, wimg);
  GCMI_CHECK_LAUNCH("fwd weight images");
  return GCMI_OK;
}

// The shapes of fwd_shape (common.h).  Anything else: GCMI_ERR_UNSUPPORTED (bf16 storage is for these shapes).
template <typename TO>
int fwd_h_gemm(const SegProduct<bf16_t, TO>& p, double* d_stats, float* d_wimg_scratch, hipStream_t sm) {
  // (fp32 output rows: the exact-operand form of the first GraphConv)
  constexpr bool kF32Out = sizeof(TO) == sizeof(float);
  if (d_wimg_scratch == nullptr || !aligned16(d_wimg_scratch) || gemm_exact_mode()) return GCMI_ERR_UNSUPPORTED;
  const FwdShape shape = fwd_shape(p);
  if (shape == kFwdNone || (kF32Out && shape != kFwdConv80)) return GCMI_ERR_UNSUPPORTED;
  SegTable st;
  const int64_t tiles = fill_seg_table(st, p, 64);
  if (tiles == 0) return GCMI_OK;
  FwdHArgs a;
  memset(&a, 0, sizeof(a));
  a.in[0] = p.op[0].a; a.ldin[0] = (int32_t)p.op[0].ld; a.in[1] = p.op[1].a; a.ldin[1] = (int32_t)p.op[1].ld;
  a.k_in = p.op[0].k; a.w[0] = p.op[0].w; a.w[1] = p.op[1].w; a.bias = p.bias; a.out = p.out; a.ldo = (int32_t)p.ldo;
  a.relu = p.act; a.stats = d_stats;
  // the segments' weight fragments, split once (kFwdHWimgFloats of scratch cover every shape above)
  const int rc = fwd_weight_images(p.n_seg, p.op[0].w_off, p.op[1].w_off, p.op[0].w, p.op[1].w, p.op[0].k,
                                   shape == kFwdConv80 ? 80 : 64, shape == kFwdDense ? 1 : 2, p.n_out, p.trans_w,
                                   d_wimg_scratch, sm);
  if (rc != GCMI_OK) return rc;
  a.wimg = reinterpret_cast<const u32x4*>(d_wimg_scratch);
  if constexpr (kF32Out) return launch_fwd_hd<2, 80, 64, false, true>(st, (int)tiles, a, sm);
  if (shape == kFwdConv80) return launch_fwd_hd<2, 80, 64, false>(st, (int)tiles, a, sm);
  if (shape == kFwdConv) return launch_fwd_hd<2, 64, 64, false>(st, (int)tiles, a, sm);
  return launch_fwd_hd<1, 64, 128, true>(st, (int)tiles, a, sm);
}
template int fwd_h_gemm(const SegProduct<bf16_t, float>&, double*, float*, hipStream_t);
template int fwd_h_gemm(const SegProduct<bf16_t, bf16_t>&, double*, float*, hipStream_t);

}  // namespace gcmi
