// One pass over the rows for everything the backward of a GraphConv / dense block does with the gradient of its
// pre-activation (autograd of models/torch_models/layers.py:6204-6246 and graphconvmodel.py:222-229):
//
//     G   = relu'(x) * (A*dy + B*x + C)              BatchNorm backward, elementwise part (bn.hip), never written
//     dW_o += In_o^T . G   (o = rel, self | dense)   weight gradients, bias gradient = column sums of G
//     dIn_o = G . W_o^T                              gradients of the block's inputs
//
// The separate kernels (bn_bwd_dx, two wgrad launches, two dgrad launches) each stream N x 64..128 floats; together
// they move 896 floats per atom for a K = 64 GraphConv and 640 (+ per-molecule rows) for the dense layer.  Here a
// 64-row tile of G is formed once in LDS from the prefetched dy / x rows (for the dense layer dy itself is recomputed
// from the per-molecule GraphGather gradient, readout_dy of bn.hip) and both products read it from there:
// 384 / 256 floats per atom.
//
// Workgroup = 8 waves on one 64-row tile of ONE degree segment: waves 0-3 form dIn (32 rows x 32..64 columns each,
// weights as three bf16 images in LDS, built once per segment), waves 4-7 accumulate dW in registers over all tiles
// of the segment the workgroup walks (one (operand, 32-column group of G) each; the rows of In arrive as per-lane
// dword loads one tile ahead, as in wgrad3_kernel) and add them to the gradient with one float atomic per element at
// the end of the segment.  Arithmetic = the exact three-way bf16 split of gemm_split.hip (six products per term on
// v_mfma_f32_32x32x16_bf16, fp32 accumulation).  A block that needs no input gradient (the first GraphConv) runs
// the four weight-gradient waves only.
//
// The dense fp32 form (RD && !HB) splits its In rows -- the pooled rows, the same eight fragments for all four
// weight-gradient waves -- once per tile: all 512 threads transpose what they prefetched across the lanes of their
// wave in phase (a) and store the three bf16 pieces as an image [piece][column][row] in LDS (in_img_col), published by
// the barrier that was there; a weight-gradient wave reads an In fragment as three ds_read_b128, splits only its own
// columns of G, and requests the next tile's rows behind its products instead of in front of them.
#include <atomic>
#include <type_traits>

#include "common.h"
#include "split_bf16.h"

namespace gcmi {

constexpr int kFRows = 64;

struct FusedArgs {
  // sources of G
  // (leading dimensions and element offsets are 32-bit: every array is < 4 GB, checked by the launchers; an
  // address is then a scalar base plus one 32-bit register instead of a 64-bit register pair per load stream)
  const float* dy;       // incoming gradient rows (nullptr: recomputed from the readout gradient)
  int32_t lddy;
  const float* x;        // BatchNorm input = the block's ReLU output
  int32_t ldx;
  const float* coef;     // [A | B | C], 3 * NG floats; nullptr: G = relu'(x) * dy
  const int32_t* membership;
  const float* g2;       // n_mols x ldg2: [dsum | dmax]
  int32_t ldg2;
  const int32_t* arg;    // n_mols x NG
  // weight-gradient operands
  const float* in[2];
  int32_t ldin[2];
  int32_t k_in;
  const float* w;
  float* dw;
  float* db;
  // input gradients (DGRAD)
  float* dout[2];
  int32_t lddout[2];
  // DGRAD, optional: column sums for the BatchNorm backward of the block BELOW this one, whose output P is this
  // block's input.  With dP this block's input gradient, sum dP and sum dP * P give that BatchNorm's sum dy and
  // sum dy * y without a pass over dy (bn.hip: bn_bwd_params_pool_kernel).  For a GraphConv block
  // dP = dXs + gather(dS), and over a symmetric adjacency sum gather(dS) * P = sum dS * gather(P) = sum dS * S:
  // both tiles and both operands are in LDS here.  Scratch layout of bn.hip: [2F unused][replica][F | F] doubles.
  double* psums;
  // diagnostics (GCMI_FUSED_DIAG=1): 100 MHz ticks spent per phase by wave 0 and wave 4 (or 3) of workgroup 0
  unsigned long long* diag;
};

// The In image of the dense fp32 form: the place of column c of In among the 64 columns of a piece.  A column is 144
// bytes (36 banks) apart from the next, so places that differ mod 16 lie in different 16-byte slots of the 256-byte
// bank row.  A ds_read_b128 of a weight-gradient wave is served in groups of 16 lanes that hold every value of
// c mod 16 once, with c bit 4 a function of c bits 2..3 within a group: the low four bits of the place must be a
// bijection of c bits 0..3 there.  The phase (a) stores (8 bytes, 16 consecutive lanes = columns 4q + j, q = 0..15, at
// one row offset; banks mod 32) need the low THREE bits of the place to take all eight values over q, which the
// identity does not (c mod 8 has two): so place bits 0..3 = c bits 2, 3, 0 ^ 4, 1.  Bits 4..5 stay.
__host__ __device__ constexpr int in_img_col(int c) {
  return (c & 0x30) | ((c >> 2) & 3) | (((c ^ (c >> 4)) & 1) << 2) | ((c & 2) << 2);
}
constexpr bool in_img_col_is_a_permutation() {
  unsigned long long seen = 0;
  for (int c = 0; c < 64; ++c) {
    const int p = in_img_col(c);
    if (p < 0 || p > 63 || (p & 0x20) != (c & 0x20) || (seen >> p & 1ull)) return false;
    seen |= 1ull << p;
  }
  return seen == ~0ull;
}
static_assert(in_img_col_is_a_permutation(), "in_img_col must be a permutation that keeps the 32-column group");

// HB: the block's forward activations (x = its ReLU output, In = its inputs) are stored as bf16
// (gcmi_model_desc.storage == 1): they arrive as 8-byte pieces of four elements -- half the prefetch registers -- and
// are widened on their way to LDS; a weight-gradient fragment of In then IS its own first bf16 piece (one v_perm_b32
// per pair instead of the three-way split).  The products of this form keep the terms above 2^-16: the result of every
// forward product was itself rounded to 2^-9 when it was stored, so the third pieces of G and W buy nothing here --
// dW += In^T G is In x the two leading pieces of G (2 MFMAs per fragment instead of 6), dIn = G W^T the three products
// g1 w1 + g1 w2 + g2 w1 (3 instead of 6): the matrix pipe, which two waves per SIMD share and which bounds these
// kernels together with the split's vector work, does half the work.  Accumulation stays fp32; gradients (dy, the
// outputs) stay fp32.
// GB (with HB; storage == 2): the gradient STREAMS are bf16 as well -- dy arrives as 8-byte pieces, the input gradients
// leave rounded once (the column sums for the BatchNorm below are taken from the rounded values: they describe what the
// next kernel reads).
// IB without HB (the first GraphConv over small-integer atom features, fp32 storage: model.hip): In alone arrives as
// bf16 rows, which hold its values EXACTLY; x and dy are fp32.  The weight-gradient fragment of In is its one piece as
// above, but G keeps all THREE pieces (3 MFMAs per fragment instead of 6): the forward was not rounded, so nothing
// justifies dropping a term here.
template <int NG, int KT, int NOPS, bool TRANS, bool RD, bool DGRAD, bool HB = false, bool GB = false, bool IB = HB>
__global__ void __launch_bounds__(DGRAD ? 512 : 256) __attribute__((amdgpu_waves_per_eu(2)))
fused_bwd_kernel(SegTable st, int n_tiles, FusedArgs a, int rev) {
  static_assert(!GB || HB, "bf16 gradient streams come with bf16 activations");
  static_assert(IB || !HB, "bf16 activations include the block's inputs");
  static_assert(IB == HB || !DGRAD, "In alone as bf16: the weight-gradient-only form");
  constexpr int NT = DGRAD ? 512 : 256;
  constexpr int NJ = NG / 32;                 // 32-column groups of G
  constexpr int KP = KT * 32;                 // padded width of In
  constexpr int GP = NG + 4;                  // pitch of a G row in LDS (floats): 16-byte rows
  constexpr int IP = KP + 4;                  // pitch of an In row in LDS
  constexpr int WP = NG + 8;                  // pitch of a weight-image row (bf16): conflict-free b128 reads
  constexpr size_t kWBytes = !DGRAD ? 0 : sizeof(unsigned short) * (size_t)NOPS * 3 * KP * WP;
  constexpr int QPR = NG / 4;                 // 16-byte pieces of a G row
  constexpr int RPP = NT / QPR;               // rows per pass of the tile loads
  constexpr int GPASS = kFRows / RPP;         // passes
  constexpr int IQ = KP / 4;                  // 16-byte pieces of an In row
  constexpr int IPASS = kFRows * IQ / NT;     // passes of the In loads, per operand
  constexpr int STEPS = kFRows / 16;          // k-steps of the weight-gradient contraction
  // the weight-gradient waves interleave the split of the next fragment with the MFMAs of the current one; the
  // bf16 dense-layer forms have no registers left for that (80 hold their prefetched rows) and only read a fragment
  // ahead (the fp32 dense-layer form has its own branch: INIMG)
  constexpr bool INTERLEAVE = !RD;
  constexpr int OT = NOPS * KT;               // 32-column tiles of the input gradients
  constexpr int TPW = OT / 2;                 // ... per dgrad wave (two waves per 32-row block)
  constexpr int OP = OT * 32 + 8;             // pitch of a row of the input-gradient tile in LDS (floats)
  constexpr int OQ = OT * 8;                  // its 16-byte pieces
  constexpr int OPASS = DGRAD ? kFRows * OQ / NT : 1;
  // The dense fp32 form splits In ONCE per tile, in phase (a), by all threads: the four weight-gradient waves read the
  // same eight In fragments (they differ in their column group of G only), so what `read_frag` + `split_frag` would
  // build per wave stands in LDS as a prepared image [piece][column of In][row] of bf16 (in_img_col, kImgPitch).
  constexpr bool INIMG = RD && !HB;
  constexpr int kImgPitch = 2 * kFRows + 16;  // bytes of one column: 64 rows of bf16 and one 16-byte entry of padding
  constexpr int kImgPiece = KP * kImgPitch;   // bytes of one piece
  static_assert(!INIMG || (DGRAD && NOPS == 1 && NT == 512 && IQ == 16 && KP == 64),
                "the In image: four rows of a pass in the four 16-lane rows of a wave, 64 columns");
  static_assert(NOPS * NJ == 4, "four weight-gradient waves: one (operand, column group) each");
  static_assert(!DGRAD || (OT % 2 == 0), "input-gradient tiles split over two waves per row block");
  static_assert(kFRows * IQ % NT == 0, "In tile loads divide evenly");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  float* Gs = reinterpret_cast<float*>(lds_raw);
  float* Ins = Gs + kFRows * GP;                                   // [NOPS][64][IP]
  unsigned short* Wimg = reinterpret_cast<unsigned short*>(Ins + NOPS * kFRows * IP);
  float* Outs = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(Wimg) + kWBytes);  // [64][OP] (DGRAD)
  unsigned char* InImg = reinterpret_cast<unsigned char*>(Outs + kFRows * OP);               // [3][KP][kImgPitch] (INIMG)
  __shared__ SegTableLds tl;  // (tl.b: the bias-gradient rows)
  __shared__ __attribute__((aligned(16))) float coef_s[3 * NG];  // [A | B | C] of the BatchNorm backward
  __shared__ double stat_s[2][DGRAD ? KP : 1];                   // sum dP | sum dP * P per input column (psums)

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // scalar: role tests and table picks stay off the vector unit
  const int lane = tid & 63;
  const int half = lane >> 5;
  const int l31 = lane & 31;
  const bool is_dgrad = DGRAD && wave < 4;
  const int wq = wave & 3;
  // weight-gradient wave: operand wo, column group wj of G
  const int wo = wq / NJ, wj = wq % NJ;
  // input-gradient wave: row block rb, output tiles [cg * TPW, cg * TPW + TPW)
  const int rb = wq & 1, cg = wq >> 1;

  tl.fill(st);

  const TileRange tiles = tile_range<false>(n_tiles, rev);
  const int my_tiles = tiles.count();

  // ---- per-thread constants of the G phase: this thread's 16-byte column piece
  const int gq = tid % QPR;
  const int gr = tid / QPR;
  for (int c = tid; c < 3 * NG; c += NT) coef_s[c] = a.coef != nullptr ? a.coef[c] : (c < NG ? 1.f : 0.f);
  if constexpr (DGRAD)
    for (int c = tid; c < 2 * KP; c += NT) stat_s[c / KP][c % KP] = 0.0;

  __syncthreads();

  SegCursor cur;  // tile -> (segment, first row, rows), moving with the walk
  cur.init(tl, st.n_seg, tiles.at(0));
  auto tile_info = [&](int tile, int& seg, int& row0, int& valid) { seg = cur.seek<kFRows>(tl, tile, row0, valid); };

  // ---- prefetch registers (one tile ahead; the molecule index two tiles ahead): all loads are 16 bytes per lane,
  // unconditional, from clamped addresses; what lies outside the tile is zeroed when it goes to LDS
  using ActV = typename std::conditional<HB, uint2, float4>::type;  // four stored activations
  auto load_act = [](const float* base, unsigned elem) -> ActV {
    if constexpr (HB) return *reinterpret_cast<const uint2*>(reinterpret_cast<const bf16_t*>(base) + elem);
    else return *reinterpret_cast<const float4*>(base + elem);
  };
  auto act4 = [](const ActV& v) -> float4 {
    if constexpr (HB) return widen4(v);
    else return v;
  };
  using InV = typename std::conditional<IB, uint2, float4>::type;   // four elements of an In row
  auto load_in = [](const float* base, unsigned elem) -> InV {
    if constexpr (IB) return *reinterpret_cast<const uint2*>(reinterpret_cast<const bf16_t*>(base) + elem);
    else return *reinterpret_cast<const float4*>(base + elem);
  };
  auto in4 = [](const InV& v) -> float4 {
    if constexpr (IB) return widen4(v);
    else return v;
  };
  using DyV = typename std::conditional<GB && !RD, uint2, float4>::type;  // four incoming gradients
  DyV pdy[GPASS];
  float4 pgm[RD ? GPASS : 1];
  ActV px[GPASS];
  InV pin[NOPS][IPASS];
  int4 parg[RD ? GPASS : 1];
  int mem1[RD ? GPASS : 1];
  auto clampr = [](int r, int valid) { return r < valid ? r : valid - 1; };
  auto load_mem = [&](int row0, int valid, int (&mem)[RD ? GPASS : 1]) {
    if constexpr (RD) {
#pragma unroll
      for (int p = 0; p < GPASS; ++p) mem[p] = a.membership[(unsigned)(row0 + clampr(gr + p * RPP, valid))];
    }
  };
  auto load_src = [&](int row0, int valid) {
#pragma unroll
    for (int p = 0; p < GPASS; ++p) {
      const unsigned r = (unsigned)(row0 + clampr(gr + p * RPP, valid));
      px[p] = load_act(a.x, r * (unsigned)a.ldx + 4u * gq);
      if constexpr (RD) {
        const unsigned m = (unsigned)mem1[p];
        pdy[p] = *reinterpret_cast<const float4*>(a.g2 + (m * (unsigned)a.ldg2 + 4u * gq));
        pgm[p] = *reinterpret_cast<const float4*>(a.g2 + (m * (unsigned)a.ldg2 + NG + 4u * gq));
        parg[p] = *reinterpret_cast<const int4*>(a.arg + (m * (unsigned)NG + 4u * gq));
      } else {
        if constexpr (GB) pdy[p] = *reinterpret_cast<const uint2*>(reinterpret_cast<const bf16_t*>(a.dy) + (r * (unsigned)a.lddy + 4u * gq));
        else pdy[p] = *reinterpret_cast<const float4*>(a.dy + (r * (unsigned)a.lddy + 4u * gq));
      }
    }
#pragma unroll
    for (int o = 0; o < NOPS; ++o) {
#pragma unroll
      for (int p = 0; p < IPASS; ++p) {
        const int slot = tid + p * NT;
        const int r = slot / IQ, q = slot - r * IQ;
        const int ld = a.ldin[o];
        const int qc = 4 * q + 4 <= ld ? 4 * q : 0;
        pin[o][p] = load_in(a.in[o], (unsigned)(row0 + clampr(r, valid)) * (unsigned)ld + qc);
      }
    }
  };

  // ---- weight-gradient state
  // one set of accumulator registers for both roles: a weight-gradient wave keeps dW in it across the tiles of a
  // segment, an input-gradient wave starts every tile from zero
  constexpr int NACC = (DGRAD && TPW > KT) ? TPW : KT;
  f32x16 accs[NACC];
#pragma unroll
  for (int t = 0; t < NACC; ++t) accs[t] = zero_acc();
  float bsum = 0.f;
  auto flush_w = [&](int seg) {
    const int64_t woff = tl.w[NOPS == 2 ? wo : 0][seg];
    if (woff >= 0) {
      // this lane's first element; its offset is made opaque so that the 32 addresses behind it are formed here
      // and not hoisted out of the tile loop into 64 registers
      int64_t woff_lane = woff + (TRANS ? (int64_t)(wj * 32 + 4 * half) * a.k_in + l31
                                        : (int64_t)(4 * half) * NG + wj * 32 + l31);
      asm volatile("" : "+v"(woff_lane));  // (an offset, not the pointer: the pointer keeps its address space)
      float* wp = a.dw + woff_lane;
#pragma unroll
      for (int t = 0; t < KT; ++t) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int r8 = acc_row(reg, 0);  // (the half: in woff_lane)
          if constexpr (TRANS) {  // dW stored NG x k_in: the accumulator holds (column of G) x (column of In)
            if (t * 32 + l31 < a.k_in) atomicAdd(wp + (int64_t)r8 * a.k_in + t * 32, accs[t][reg]);
          } else {                // dW stored k_in x NG
            if (t * 32 + r8 + 4 * half < a.k_in) atomicAdd(wp + (t * 32 + r8) * NG, accs[t][reg]);
          }
        }
      }
    }
#pragma unroll
    for (int t = 0; t < KT; ++t) accs[t] = zero_acc();
    if (wo == 0) {
      const int64_t boff = tl.b[seg];
      const float s = bsum + __shfl_xor(bsum, 32);
      if (half == 0 && a.db != nullptr && boff >= 0) atomicAdd(a.db + boff + wj * 32 + l31, s);
    }
    bsum = 0.f;
  };

  static_assert(!DGRAD || NT % IQ == 0, "a thread keeps its column piece over the passes");
  // The input-gradient tile leaves through LDS: the waves that computed it hold (column, 16 rows) per lane, which as
  // global stores would be 32 dword stores per lane -- and, issued behind the next tile's loads, every wave's wait
  // for those loads (one instruction stream for both roles: the wait cannot tell which role it is in) would also
  // wait for the store acknowledgements.  Written out by all threads at the start of the next tile instead: whole
  // rows, 16 bytes per lane, and in program order BEFORE the loads that follow.
  // (thread -> element mapping = that of the In tile loads: a thread reads here exactly the In elements it is about
  // to overwrite with the next tile's, so no barrier is needed between the two)
  // (the sums: fp32 partials per thread over a few tiles -- a thread keeps its column piece --, then fp64 in LDS:
  // per-element fp64 products and LDS atomics cost a microsecond per tile)
  float ps1[4] = {0.f, 0.f, 0.f, 0.f}, ps2[4] = {0.f, 0.f, 0.f, 0.f};
  auto flush_psums = [&]() {
    if constexpr (DGRAD) {
      const int q = tid % IQ;  // NT % IQ == 0: the same column piece in every pass
      if (4 * q < a.k_in) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          atomicAdd(&stat_s[0][4 * q + i], (double)ps1[i]);
          atomicAdd(&stat_s[1][4 * q + i], (double)ps2[i]);
          ps1[i] = ps2[i] = 0.f;
        }
      }
    }
  };
  auto store_out = [&](int prow0, int pvalid, int pseg) {
    if constexpr (DGRAD) {
      static_assert(OQ == NOPS * IQ, "one input-gradient row piece per In row piece");
      const float deg = (float)pseg;  // segment = degree block: a row of dS is gathered by `deg` neighbours
#pragma unroll
      for (int o = 0; o < NOPS; ++o) {
        float* dst = o == 1 ? a.dout[1] : a.dout[0];
        const int ldd = o == 1 ? a.lddout[1] : a.lddout[0];
#pragma unroll
        for (int p = 0; p < IPASS; ++p) {
          const int slot = tid + p * NT;
          const int r = slot / IQ, q = slot - r * IQ;
          if (r < pvalid && 4 * q < a.k_in) {  // k_in % 4 == 0 (launcher)
            float4 v = *reinterpret_cast<const float4*>(Outs + r * OP + o * KP + 4 * q);
            if constexpr (GB) {
              const uint2 h = narrow4(v.x, v.y, v.z, v.w);
              *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(dst) + ((unsigned)(prow0 + r) * (unsigned)ldd + 4u * q)) = h;
              v = widen4(h);  // the sums below describe the stored values
            } else {
              *reinterpret_cast<float4*>(dst + ((unsigned)(prow0 + r) * (unsigned)ldd + 4u * q)) = v;
            }
            if (a.psums != nullptr) {
              const float4 in = *reinterpret_cast<const float4*>(Ins + (o * kFRows + r) * IP + 4 * q);
              const float wgt = (NOPS == 2 && o == 0) ? deg : 1.f;
              ps1[0] = fmaf(wgt, v.x, ps1[0]); ps1[1] = fmaf(wgt, v.y, ps1[1]);
              ps1[2] = fmaf(wgt, v.z, ps1[2]); ps1[3] = fmaf(wgt, v.w, ps1[3]);
              ps2[0] = fmaf(v.x, in.x, ps2[0]); ps2[1] = fmaf(v.y, in.y, ps2[1]);
              ps2[2] = fmaf(v.z, in.z, ps2[2]); ps2[3] = fmaf(v.w, in.w, ps2[3]);
            }
          }
        }
      }
    }
  };

  // ---- prologue: sources of the first tile, molecule indices of the first two
  int seg, row0, valid;
  tile_info(tiles.at(0), seg, row0, valid);
  int nseg = seg, nrow0 = row0, nvalid = valid;  // the tile after this one (itself when there is none)
  if (my_tiles > 1) tile_info(tiles.at(1), nseg, nrow0, nvalid);
  load_mem(row0, valid, mem1);
  load_src(row0, valid);
  load_mem(nrow0, nvalid, mem1);  // mem1 now describes tile 1: its sources are requested in phase (b) of tile 0
  int cur_seg = -1;
  int prow0 = row0, pvalid = 0, pseg = 0;

  const bool stamp = a.diag != nullptr && blockIdx.x == 0 && lane == 0 && (wave == 0 || wave == NT / 64 - 1);
  unsigned long long d_a = 0, d_w1 = 0, d_b = 0, d_w2 = 0, t0 = 0, t1 = 0;
  for (int i = 0; i < my_tiles; ++i) {
    if (stamp) t0 = wall_clock64();
    if (seg != cur_seg) {
      if (cur_seg >= 0 && !is_dgrad) flush_w(cur_seg);
      cur_seg = seg;
      if constexpr (DGRAD) {
        // the segment's weight blocks as three bf16 images [operand][piece][input column][column of G]
        // (everyone passed the barrier that ended the previous tile: nobody reads the old images any more)
        constexpr int NE = NOPS * KP * NG;
        for (int e = tid; e < NE; e += NT) {
          int o, ko, c;
          if constexpr (TRANS) {  // w is NG x k_in: consecutive threads along k_in
            o = 0;
            c = e / KP;
            ko = e - c * KP;
          } else {                // w is k_in x NG: consecutive threads along NG
            o = e / (KP * NG);
            const int r = e - o * (KP * NG);
            ko = r / NG;
            c = r - ko * NG;
          }
          const int64_t woff = tl.w[NOPS == 2 ? (o & 1) : 0][seg];
          float v = 0.f;
          if (woff >= 0 && ko < a.k_in)
            v = TRANS ? a.w[woff + (int64_t)c * a.k_in + ko] : a.w[woff + (int64_t)ko * NG + c];
          unsigned p1, p2, p3;
          split3(v, p1, p2, p3);
          unsigned short* dst = Wimg + ((size_t)(o * 3) * KP + ko) * WP + c;
          dst[0] = (unsigned short)(p1 >> 16);
          dst[(size_t)KP * WP] = (unsigned short)(p2 >> 16);
          dst[(size_t)2 * KP * WP] = (unsigned short)(p3 >> 16);
        }
      }
    }

    // ---- phase (a): the previous tile's input gradients out (they were written before the last barrier; this also
    // reads the previous In rows, so it comes first), then G and the In rows of this tile -> LDS
    if (i > 0) {
      store_out(prow0, pvalid, pseg);
      if (a.psums != nullptr && (i & 7) == 0) flush_psums();
    }
#pragma unroll
    for (int p = 0; p < GPASS; ++p) {
      const int r = gr + p * RPP;
      float4 dy4;
      if constexpr (GB && !RD) dy4 = widen4(pdy[p]);
      else dy4 = pdy[p];
      float dyv[4] = {dy4.x, dy4.y, dy4.z, dy4.w};
      const float4 x4 = act4(px[p]);
      const float xv[4] = {x4.x, x4.y, x4.z, x4.w};
      if constexpr (RD) {
        const int rg = row0 + r;
        const float gm[4] = {pgm[p].x, pgm[p].y, pgm[p].z, pgm[p].w};
        const int av[4] = {parg[p].x, parg[p].y, parg[p].z, parg[p].w};
#pragma unroll
        for (int q = 0; q < 4; ++q) dyv[q] = dyv[q] + (av[q] == rg ? gm[q] : 0.f);
      }
      const float4 cA4 = *reinterpret_cast<const float4*>(coef_s + 4 * gq);
      const float4 cB4 = *reinterpret_cast<const float4*>(coef_s + NG + 4 * gq);
      const float4 cC4 = *reinterpret_cast<const float4*>(coef_s + 2 * NG + 4 * gq);
      const float cA[4] = {cA4.x, cA4.y, cA4.z, cA4.w}, cB[4] = {cB4.x, cB4.y, cB4.z, cB4.w};
      const float cC[4] = {cC4.x, cC4.y, cC4.z, cC4.w};
      float o[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float v = fmaf(cA[q], dyv[q], fmaf(cB[q], xv[q], cC[q]));
        o[q] = (r < valid && xv[q] > 0.f) ? v : 0.f;
      }
      *reinterpret_cast<float4*>(Gs + r * GP + 4 * gq) = make_float4(o[0], o[1], o[2], o[3]);
    }
#pragma unroll
    for (int o = 0; o < NOPS; ++o) {
#pragma unroll
      for (int p = 0; p < IPASS; ++p) {
        const int slot = tid + p * NT;
        const int r = slot / IQ, q = slot - r * IQ;
        const int tail = a.k_in - 4 * q;
        float4 v = in4(pin[o][p]);
        const bool ok = r < valid;
        v.x = (ok && tail > 0) ? v.x : 0.f;
        v.y = (ok && tail > 1) ? v.y : 0.f;
        v.z = (ok && tail > 2) ? v.z : 0.f;
        v.w = (ok && tail > 3) ? v.w : 0.f;
        *reinterpret_cast<float4*>(Ins + (o * kFRows + r) * IP + 4 * q) = v;
        if constexpr (INIMG) {
          // The four rows r0 .. r0 + 3 of this pass (r0 = 4 * wave + 32 * p) lie in the four 16-lane rows of the
          // wave: a 4 x 4 transposition across lanes 16 apart (register bit 1 <-> lane bit 5, register bit 0 <-> lane
          // bit 4) leaves the thread in lane row j with column 4q + j of rows r0 .. r0 + 3: two row pairs, split
          // exactly as split_frag splits (raw[2i], raw[2i + 1]), 8 bytes per piece of the 16-byte entry of rows
          // 8 * (r0 / 8) .. + 7.  (all 512 threads are here: the swaps need every lane)
          unsigned t0 = __float_as_uint(v.x), t1 = __float_as_uint(v.y), t2 = __float_as_uint(v.z), t3 = __float_as_uint(v.w);
          auto s02 = __builtin_amdgcn_permlane32_swap(t0, t2, false, false);
          t0 = s02[0]; t2 = s02[1];
          auto s13 = __builtin_amdgcn_permlane32_swap(t1, t3, false, false);
          t1 = s13[0]; t3 = s13[1];
          auto s01 = __builtin_amdgcn_permlane16_swap(t0, t1, false, false);
          t0 = s01[0]; t1 = s01[1];
          auto s23 = __builtin_amdgcn_permlane16_swap(t2, t3, false, false);
          t2 = s23[0]; t3 = s23[1];
          uint2 pc[3];
          split3_pair(__uint_as_float(t0), __uint_as_float(t1), pc[0].x, pc[1].x, pc[2].x);
          split3_pair(__uint_as_float(t2), __uint_as_float(t3), pc[0].y, pc[1].y, pc[2].y);
          unsigned char* dst = InImg + in_img_col(4 * (lane & 15) + (lane >> 4)) * kImgPitch + 8 * wave + 64 * p;
#pragma unroll
          for (int s = 0; s < 3; ++s) *reinterpret_cast<uint2*>(dst + s * kImgPiece) = pc[s];
        }
      }
    }
    if (stamp) { t1 = wall_clock64(); d_a += t1 - t0; }
    __syncthreads();
    if (stamp) { t0 = wall_clock64(); d_w1 += t0 - t1; }

    // ---- phase (b): next tile's sources in flight, products from LDS
    int n2seg = nseg, n2row0 = nrow0, n2valid = nvalid;
    if (i + 2 < my_tiles) tile_info(tiles.at(i + 2), n2seg, n2row0, n2valid);
    // (the In-image form: its weight-gradient waves request the next tile BEHIND their products, see there)
    if (!(INIMG && !is_dgrad)) {
      load_src(nrow0, nvalid);           // uses mem1 = molecule indices of the next tile (read when the loads issue)
      load_mem(n2row0, n2valid, mem1);   // ... which the indices of the tile after it then replace
    }
    if (is_dgrad) {
      if constexpr (DGRAD) {
        // input gradients of this tile: `accs` starts from zero (the weight-gradient waves keep theirs across tiles)
#pragma unroll
        for (int t = 0; t < TPW; ++t) accs[t] = zero_acc();
        bool on[TPW];
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
          const int ot = cg * TPW + t;
          on[t] = tl.w[NOPS == 2 ? ((ot / KT) & 1) : 0][seg] >= 0;
        }
        // units (k-step, output tile), the LDS reads of unit u + 1 issued before the split and the MFMAs of unit u:
        // with two waves per SIMD nobody else hides a read's latency
        constexpr int NKS = NG / 16, NU = NKS * TPW;
        float4 glo, ghi;
        Frag3 wv[2];
        auto read_g = [&](int ks) {
          const float* grow = Gs + (rb * 32 + l31) * GP + ks * 16 + 8 * half;
          glo = *reinterpret_cast<const float4*>(grow);
          ghi = *reinterpret_cast<const float4*>(grow + 4);
        };
        auto read_w = [&](int u) {
          const int ks = u / TPW, t = u - ks * TPW;
          const int ot = cg * TPW + t;
          const int o = ot / KT, kt = ot - o * KT;
          const unsigned short* wrow = Wimg + ((size_t)(o * 3) * KP + kt * 32 + l31) * WP + ks * 16 + 8 * half;
          wv[u & 1].p[0] = *reinterpret_cast<const u32x4*>(wrow);
          wv[u & 1].p[1] = *reinterpret_cast<const u32x4*>(wrow + (size_t)KP * WP);
          if constexpr (!HB) wv[u & 1].p[2] = *reinterpret_cast<const u32x4*>(wrow + (size_t)2 * KP * WP);
        };
        read_g(0);
        read_w(0);
        Frag3 fg;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
          const int ks = u / TPW, t = u - ks * TPW;
          if (t == 0) fg = split_frag(glo, ghi);  // this k-step's rows of G; its registers then take the next k-step's
          if (u + 1 < NU) {
            read_w(u + 1);
            if (t == TPW - 1) read_g(ks + 1);
          }
          if (on[t]) {  // uniform
            // rows of G x input columns: lane = input column, registers = rows; HB: without the 2^-16 terms
            if constexpr (!HB) mfma_split3_small(accs[t], fg, wv[u & 1]);
            mfma_split3_large(accs[t], fg, wv[u & 1]);
          }
          __builtin_amdgcn_sched_barrier(0);  // units stay in order: one set of fragments live besides the one in flight
        }
        // -> LDS, [row][tile * 32 + column]: 32 consecutive banks per half-wave, the halves 32 banks apart
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
          float* orow = Outs + (rb * 32 + 4 * half) * OP + (cg * TPW + t) * 32 + l31;
#pragma unroll
          for (int reg = 0; reg < 16; ++reg) orow[acc_row(reg, 0) * OP] = accs[t][reg];  // (orow holds the half)
        }
      }
    } else {
      const bool on = tl.w[NOPS == 2 ? wo : 0][seg] >= 0;
      const float* irow = Ins + (NOPS == 2 ? wo : 0) * kFRows * IP;
      // Fragments in order: per 16-row step the G columns, then the KT column groups of In.  The eight LDS reads of
      // fragment f + 1 are issued before fragment f is split and multiplied: with two waves per SIMD nobody else
      // hides their latency.
      constexpr int FPS = 1 + KT, NF = STEPS * FPS;
      if constexpr (INIMG) {
      // The In fragments come ready-made from the image of phase (a): three ds_read_b128 each, no `raw` and no split.
      // Only the G fragment of a 16-row step is read as rows and split here.  Per (fragment, accumulator) the six
      // MFMAs of mfma_split6 in its order, the fragments of an accumulator in the order of the steps.  A wave issues
      // in order and the six MFMAs of a chain depend on each other, so what else the wave has to do goes between
      // them: the split of the NEXT step's G in four quarters between the MFMAs of the step's first In fragment, and
      // the three reads of the next In fragment, each behind the last product that reads the piece it replaces (In as
      // operand B is read in the order 1 3 2 1 2 1; piece 1 goes to registers of its own, three products ahead).
      // (`on` is not looked at: with no weight block the products go into accumulators that flush_w drops)
      const unsigned char* ibase = InImg + in_img_col(l31) * kImgPitch + 16 * half;
      auto in_piece = [&](int f, int pc) -> u32x4 {  // f = 16-row step * KT + 32-column group (in_img_col keeps it)
        return *reinterpret_cast<const u32x4*>(ibase + (f % KT) * 32 * kImgPitch + 32 * (f / KT) + pc * kImgPiece);
      };
      float raw[8];
      auto read_g = [&](int st_) {
        const float* src = Gs + (16 * st_ + 8 * half) * GP + wj * 32 + l31;  // zero beyond `valid`
#pragma unroll
        for (int u = 0; u < 8; ++u) raw[u] = src[u * GP];
      };
      auto add_bsum = [&]() {
        if (wo == 0) {
#pragma unroll
          for (int u = 0; u < 8; ++u) bsum += raw[u];
        }
      };
      constexpr int NIF = STEPS * KT;
      read_g(0);
      Frag3 fa = {{in_piece(0, 0), in_piece(0, 1), in_piece(0, 2)}}, fg, fgn;
      add_bsum();
      fgn = split_frag(raw);
      if (STEPS > 1) read_g(1);
      unsigned q[3][4];
#pragma unroll
      for (int f = 0; f < NIF; ++f) {
        const int st_ = f / KT, t = f - st_ * KT;
        if (t == 0) fg = fgn;
        const bool more = f + 1 < NIF;
        const bool split_next = t == 0 && st_ + 1 < STEPS;  // this chain carries the split of the next step's G
        if (split_next) add_bsum();
        auto pair_split = [&](int i) {
          if (split_next) split3_pair(raw[2 * i], raw[2 * i + 1], q[0][i], q[1][i], q[2][i]);
          __builtin_amdgcn_sched_barrier(0);
        };
        const Frag3& L = TRANS ? fg : fa;
        const Frag3& R = TRANS ? fa : fg;
        Frag3 nf = fa;
        // mfma_split6(accs[t], L, R) spelled out, in its order
        accs[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(L.p[2]), as_bf16x8(R.p[0]), accs[t], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        pair_split(0);
        accs[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(L.p[0]), as_bf16x8(R.p[2]), accs[t], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (more && TRANS) nf.p[2] = in_piece(f + 1, 2);
        pair_split(1);
        accs[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(L.p[1]), as_bf16x8(R.p[1]), accs[t], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (more && TRANS) nf.p[0] = in_piece(f + 1, 0);
        pair_split(2);
        accs[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(L.p[1]), as_bf16x8(R.p[0]), accs[t], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        pair_split(3);
        accs[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(L.p[0]), as_bf16x8(R.p[1]), accs[t], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (more && TRANS) nf.p[1] = in_piece(f + 1, 1);
        if (split_next && st_ + 2 < STEPS) read_g(st_ + 2);  // `raw` is free: the G rows of the step after next
        __builtin_amdgcn_sched_barrier(0);
        accs[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(L.p[0]), as_bf16x8(R.p[0]), accs[t], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (more && !TRANS) nf = {{in_piece(f + 1, 0), in_piece(f + 1, 1), in_piece(f + 1, 2)}};
        fa = nf;
        if (split_next) {
#pragma unroll
          for (int pc = 0; pc < 3; ++pc) {
            fgn.p[pc].x = q[pc][0]; fgn.p[pc].y = q[pc][1]; fgn.p[pc].z = q[pc][2]; fgn.p[pc].w = q[pc][3];
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      // The next tile's sources, requested here and not in front of the products: with all eight waves asking at
      // once the memory pipeline takes 2.4 us to accept the last wave's 22 loads (phase clocks), and
      // these waves' products, 1.6 us that need nothing from memory, would only start then.  The input-gradient waves
      // ask first and have the queue to themselves; these waves' requests follow while those still multiply.
      load_src(nrow0, nvalid);
      load_mem(n2row0, n2valid, mem1);
      } else if constexpr (INTERLEAVE) {
      float raw[8];
      auto read_frag = [&](int f) {
        const int st_ = f / FPS, w_ = f - st_ * FPS;
        const float* src = w_ == 0 ? Gs + (16 * st_ + 8 * half) * GP + wj * 32 + l31            // zero beyond `valid`
                                   : irow + (16 * st_ + 8 * half) * IP + (w_ - 1) * 32 + l31;
        const int pitch = w_ == 0 ? GP : IP;
#pragma unroll
        for (int u = 0; u < 8; ++u) raw[u] = src[u * pitch];
      };
      // Software pipeline over fragments: in iteration f the split of fragment f + 1 (vector unit) is interleaved
      // with the six MFMAs of fragment f (a wave issues in order: behind a chain of dependent MFMAs nothing of its
      // own would issue for 6 x 32 cycles), and the LDS reads of fragment f + 2 follow the split that frees `raw`.
      read_frag(0);
      Frag3 fg, cur, nxt;
      {
        if (wo == 0) {
#pragma unroll
          for (int u = 0; u < 8; ++u) bsum += raw[u];
        }
        nxt = split_frag(raw);  // fragment 0 is a G fragment
        if (NF > 1) read_frag(1);
      }
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const int w_ = f % FPS;
        cur = nxt;
        if (w_ == 0) fg = cur;
        const bool more = f + 1 < NF;
        if (more && (f + 1) % FPS == 0 && wo == 0) {
#pragma unroll
          for (int u = 0; u < 8; ++u) bsum += raw[u];
        }
        unsigned q[3][4];
        const bool next_is_g = (f + 1) % FPS == 0;  // (compile-time under the unrolling)
        auto pair_split = [&](int i) {
          if (!more) return;
          if (IB && !next_is_g) {  // a fragment of stored bf16 values: exact in one piece
            q[0][i] = pack_exact_bf16x2(raw[2 * i], raw[2 * i + 1]);
            q[1][i] = q[2][i] = 0u;
          } else {
            split3_pair(raw[2 * i], raw[2 * i + 1], q[0][i], q[1][i], q[2][i]);
          }
        };
        if (IB && w_ != 0 && on) {  // uniform: In in one piece
          const int t = w_ - 1;
          const Frag3& L = TRANS ? fg : cur;
          const Frag3& R = TRANS ? cur : fg;
          // (In is `cur`: TRANS -> the right operand R.p[0], else the left operand L.p[0]; G in its two leading pieces
          // -- all three when the forward was not rounded --, the smaller first)
          if constexpr (!HB) {
            accs[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(TRANS ? L.p[2] : L.p[0]),
                                                              as_bf16x8(TRANS ? R.p[0] : R.p[2]), accs[t], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
          }
          pair_split(0);
          pair_split(1);
          __builtin_amdgcn_sched_barrier(0);
          accs[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(TRANS ? L.p[1] : L.p[0]),
                                                            as_bf16x8(TRANS ? R.p[0] : R.p[1]), accs[t], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          pair_split(2);
          pair_split(3);
          __builtin_amdgcn_sched_barrier(0);
          if (more && f + 2 < NF) read_frag(f + 2);  // `raw` is free: the reads of the fragment after next
          __builtin_amdgcn_sched_barrier(0);
          accs[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(L.p[0]), as_bf16x8(R.p[0]), accs[t], 0, 0, 0);
        } else if (w_ != 0 && on) {  // uniform
          const int t = w_ - 1;
          const Frag3& L = TRANS ? fg : cur;
          const Frag3& R = TRANS ? cur : fg;
          // mfma_split6(accs[t], L, R) unrolled by hand, and it must keep that order: MFMA, a quarter of the next
          // fragment's split, MFMA, ... (pinned: the scheduler would put the six dependent MFMAs back to back)
          accs[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(L.p[2]), as_bf16x8(R.p[0]), accs[t], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          pair_split(0);
          __builtin_amdgcn_sched_barrier(0);
          accs[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(L.p[0]), as_bf16x8(R.p[2]), accs[t], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          pair_split(1);
          __builtin_amdgcn_sched_barrier(0);
          accs[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(L.p[1]), as_bf16x8(R.p[1]), accs[t], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          pair_split(2);
          __builtin_amdgcn_sched_barrier(0);
          accs[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(L.p[1]), as_bf16x8(R.p[0]), accs[t], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          pair_split(3);
          __builtin_amdgcn_sched_barrier(0);
          accs[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(L.p[0]), as_bf16x8(R.p[1]), accs[t], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          if (more && f + 2 < NF) read_frag(f + 2);  // `raw` is free: the reads of the fragment after next
          __builtin_amdgcn_sched_barrier(0);
          accs[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(L.p[0]), as_bf16x8(R.p[0]), accs[t], 0, 0, 0);
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) pair_split(i);
          if (more && f + 2 < NF) read_frag(f + 2);
        }
        if (more) {
#pragma unroll
          for (int pc = 0; pc < 3; ++pc) {
            nxt.p[pc].x = q[pc][0]; nxt.p[pc].y = q[pc][1]; nxt.p[pc].z = q[pc][2]; nxt.p[pc].w = q[pc][3];
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      } else {
      float raw[2][8];
      auto read_frag = [&](int f) {
        const int st_ = f / FPS, w_ = f - st_ * FPS;
        const float* src = w_ == 0 ? Gs + (16 * st_ + 8 * half) * GP + wj * 32 + l31            // zero beyond `valid`
                                   : irow + (16 * st_ + 8 * half) * IP + (w_ - 1) * 32 + l31;
        const int pitch = w_ == 0 ? GP : IP;
#pragma unroll
        for (int u = 0; u < 8; ++u) raw[f & 1][u] = src[u * pitch];
      };
      read_frag(0);
      Frag3 fg;
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const int w_ = f % FPS;
        if (f + 1 < NF) read_frag(f + 1);
        if (w_ == 0) {
          if (wo == 0) {
#pragma unroll
            for (int u = 0; u < 8; ++u) bsum += raw[f & 1][u];
          }
          fg = split_frag(raw[f & 1]);
        } else if (on) {  // uniform
          const int t = w_ - 1;
          if constexpr (HB) {  // In in one exact piece x G in three
            u32x4 fi;
            fi.x = pack_exact_bf16x2(raw[f & 1][0], raw[f & 1][1]); fi.y = pack_exact_bf16x2(raw[f & 1][2], raw[f & 1][3]);
            fi.z = pack_exact_bf16x2(raw[f & 1][4], raw[f & 1][5]); fi.w = pack_exact_bf16x2(raw[f & 1][6], raw[f & 1][7]);
#pragma unroll
            for (int pc = 1; pc >= 0; --pc)  // G in its two leading pieces (terms above 2^-16)
              accs[t] = TRANS ? __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(fg.p[pc]), as_bf16x8(fi), accs[t], 0, 0, 0)
                              : __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(fi), as_bf16x8(fg.p[pc]), accs[t], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            continue;
          }
          const Frag3 fa = split_frag(raw[f & 1]);
          const Frag3& L = TRANS ? fg : fa;
          const Frag3& R = TRANS ? fa : fg;
          mfma_split6(accs[t], L, R);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      }
    }
    if (stamp) { t1 = wall_clock64(); d_b += t1 - t0; }
    __syncthreads();
    if (stamp) { t0 = wall_clock64(); d_w2 += t0 - t1; }
    prow0 = row0; pvalid = valid; pseg = seg;
    seg = nseg; row0 = nrow0; valid = nvalid;
    nseg = n2seg; nrow0 = n2row0; nvalid = n2valid;
  }
  store_out(prow0, pvalid, pseg);
  if (!is_dgrad) flush_w(cur_seg);
  if constexpr (DGRAD) {
    if (a.psums != nullptr) {
      flush_psums();
      __syncthreads();
      for (int c = tid; c < 2 * KP; c += NT) {
        const int which = c / KP, col = c - which * KP;
        if (col < a.k_in)
          atomicAdd(a.psums + (size_t)2 * a.k_in * (1 + (blockIdx.x % kBnReplicas)) + (size_t)which * a.k_in + col,
                    stat_s[which][col]);
      }
    }
  }
  if (stamp) {
    unsigned long long* d = a.diag + (wave == 0 ? 0 : 5);
    d[0] = d_a; d[1] = d_w1; d[2] = d_b; d[3] = d_w2; d[4] = (unsigned long long)my_tiles;
  }
}

static bool fused_bwd_on() {
  static const int env = getenv("GCMI_FUSED_BWD") ? atoi(getenv("GCMI_FUSED_BWD")) : 1;
  return env != 0;
}

static std::atomic<int> g_fused_bwd{1};
static std::atomic<int> g_fused_launches{0};
int fused_bwd_launches() { return g_fused_launches.load(std::memory_order_relaxed); }
void set_fused_bwd(int on) { g_fused_bwd.store(on ? 1 : 0, std::memory_order_relaxed); }
int get_fused_bwd() { return g_fused_bwd.load(std::memory_order_relaxed); }
bool fused_bwd_enabled() { return fused_bwd_on() && get_fused_bwd() != 0 && !gemm_exact_mode(); }

template <int NG, int KT, int NOPS, bool TRANS, bool RD, bool DGRAD, bool HB = false, bool GB = false, bool IB = HB>
static int launch_fused(const SegTable& st, int n_tiles, const FusedArgs& a, hipStream_t sm) {
  constexpr int KP = KT * 32;
  size_t shmem = sizeof(float) * kFRows * (NG + 4) + sizeof(float) * (size_t)NOPS * kFRows * (KP + 4);
  if (DGRAD)
    shmem += sizeof(unsigned short) * (size_t)NOPS * 3 * KP * (NG + 8) + sizeof(float) * kFRows * (NOPS * KT * 32 + 8);
  if (RD && !HB) shmem += (size_t)3 * KP * (2 * kFRows + 16);  // the In image of the dense fp32 form
  auto kern = fused_bwd_kernel<NG, KT, NOPS, TRANS, RD, DGRAD, HB, GB, IB>;
  // exactly what is asked for: the kernel also has a few hundred bytes of static LDS (the segment table)
  static LdsLimit lim;  // per instantiation
  if (!raise_lds_limit(lim, reinterpret_cast<const void*>(kern), shmem)) return GCMI_ERR_UNSUPPORTED;
  const int per_cu = DGRAD ? 1 : 2;
  const int grid = std::min(n_tiles, 256 * per_cu);
  static const bool diag_on = getenv("GCMI_FUSED_DIAG") && atoi(getenv("GCMI_FUSED_DIAG")) != 0;
  static unsigned long long* d_diag = nullptr;
  FusedArgs aa = a;
  if (diag_on) {
    if (!d_diag && hipMalloc(&d_diag, 10 * sizeof(unsigned long long)) != hipSuccess) d_diag = nullptr;
    if (d_diag) (void)hipMemsetAsync(d_diag, 0, 10 * sizeof(unsigned long long), sm);
    aa.diag = d_diag;
  }
  hipLaunchKernelGGL(kern, dim3(grid), dim3(DGRAD ? 512 : 256), shmem, sm, st, n_tiles, aa, next_sweep_direction());
  GCMI_CHECK_LAUNCH("fused_bwd");
  if (diag_on && d_diag) {  // serialises the stream: diagnostics only
    unsigned long long h[10];
    if (hipStreamSynchronize(sm) == hipSuccess && hipMemcpy(h, d_diag, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess)
      fprintf(stderr, "fused_bwd<%d,%d,%d> tiles %llu | first wave: G phase %.2f us, wait %.2f, products %.2f, wait %.2f "
                      "| last wave: %.2f %.2f %.2f %.2f (per tile)\n", NG, KT, (int)DGRAD, h[4],
              h[0] * 0.01 / h[4], h[1] * 0.01 / h[4], h[2] * 0.01 / h[4], h[3] * 0.01 / h[4], h[5] * 0.01 / h[4],
              h[6] * 0.01 / h[4], h[7] * 0.01 / h[4], h[8] * 0.01 / h[4]);
  }
  g_fused_launches.fetch_add(1, std::memory_order_relaxed);
  return GCMI_OK;
}

// The narrowing both launchers share: the BlockBackward fields that mean the same for either block
static FusedArgs fused_args(const BlockBackward& b) {
  FusedArgs a;
  memset(&a, 0, sizeof(a));
  a.dy = b.dy; a.lddy = (int32_t)b.lddy; a.x = b.gc; a.ldx = (int32_t)b.ldgc; a.coef = b.coef;
  if (b.rg) { a.membership = b.rg->membership; a.g2 = b.rg->g2; a.ldg2 = (int32_t)b.rg->ldg2; a.arg = b.rg->arg; }
  for (int o = 0; o < 2; ++o) {
    a.in[o] = b.in[o].rows; a.ldin[o] = (int32_t)b.in[o].ld;
    a.dout[o] = b.dout[o].rows; a.lddout[o] = (int32_t)b.dout[o].ld;
  }
  a.k_in = b.k_in; a.w = b.w; a.dw = b.dw; a.db = b.db;
  a.psums = b.dout[0].rows ? b.psums : nullptr;
  return a;
}

// GraphConv block: dW_rel += S^T G, dW_self += X^T G, dbsum += colsum G, and (dout[0] given) dS = G W_rel^T,
// dXs = G W_self^T.  GCMI_ERR_UNSUPPORTED = shape not covered (the caller runs the separate kernels).
int fused_conv_bwd(const BlockBackward& b, hipStream_t sm) {
  const int32_t k_in = b.k_in, act_bf16 = b.act_bf16, in_bf16 = b.in_bf16;
  if (!fused_bwd_enabled() || b.n_seg > kMaxProductSeg || b.width != 64 || b.rg != nullptr) return GCMI_ERR_UNSUPPORTED;
  // (in_bf16 without act_bf16: BlockBackward::in_bf16)
  if (in_bf16 && (act_bf16 || b.dout[0].rows != nullptr || k_in <= 64 || k_in > 96)) return GCMI_ERR_UNSUPPORTED;
  {  // 32-bit element offsets inside the kernel: every array below 2^30 elements
    int64_t rows = 0;
    for (int sgi = 0; sgi < b.n_seg; ++sgi) rows = std::max<int64_t>(rows, b.seg_end[sgi]);
    const int64_t ldmax = std::max(std::max(b.lddy, b.ldgc),
                                   std::max(std::max(b.in[0].ld, b.in[1].ld), std::max(b.dout[0].ld, b.dout[1].ld)));
    if (rows * ldmax >= (int64_t)1 << 30) return GCMI_ERR_UNSUPPORTED;
  }
  if (!aligned16(b.dy) || b.lddy % 4 || !aligned16(b.gc) || b.ldgc % 4) return GCMI_ERR_UNSUPPORTED;
  if (b.coef && !aligned16(b.coef)) return GCMI_ERR_UNSUPPORTED;
  // (act_bf16: gc and in point to bf16 rows, their leading dimensions count elements; 8-byte pieces)
  if ((act_bf16 || in_bf16) && (!aligned16(b.in[0].rows) || b.in[0].ld % 4 || !aligned16(b.in[1].rows) || b.in[1].ld % 4))
    return GCMI_ERR_UNSUPPORTED;
  const bool dgrad = b.dout[0].rows != nullptr;
  SegTable st;
  const int tiles = (int)fill_seg_table(st, b.n_seg, b.seg_begin, b.seg_end, b.w_off[0], b.w_off[1], b.b_off, kFRows);
  if (tiles == 0) return GCMI_OK;
  const FusedArgs a = fused_args(b);
  if (dgrad) {
    if (k_in % 4 || b.dout[0].ld % 4 || b.dout[1].ld % 4 || !aligned16(b.dout[0].rows) || !aligned16(b.dout[1].rows))
      return GCMI_ERR_UNSUPPORTED;
    // (act_bf16 == 2: dy, dS and dXs are bf16 rows too)
    if (k_in > 32 && k_in <= 64)
      return act_bf16 == 2 ? launch_fused<64, 2, 2, false, false, true, true, true>(st, tiles, a, sm)
             : act_bf16    ? launch_fused<64, 2, 2, false, false, true, true>(st, tiles, a, sm)
                           : launch_fused<64, 2, 2, false, false, true>(st, tiles, a, sm);
    return GCMI_ERR_UNSUPPORTED;
  }
  if (k_in > 32 && k_in <= 64)
    return act_bf16 == 2 ? launch_fused<64, 2, 2, false, false, false, true, true>(st, tiles, a, sm)
           : act_bf16    ? launch_fused<64, 2, 2, false, false, false, true>(st, tiles, a, sm)
                         : launch_fused<64, 2, 2, false, false, false>(st, tiles, a, sm);
  if (in_bf16) return launch_fused<64, 3, 2, false, false, false, false, false, true>(st, tiles, a, sm);
  if (k_in > 64 && k_in <= 96)
    return act_bf16 == 2 ? launch_fused<64, 3, 2, false, false, false, true, true>(st, tiles, a, sm)
           : act_bf16    ? launch_fused<64, 3, 2, false, false, false, true>(st, tiles, a, sm)
                         : launch_fused<64, 3, 2, false, false, false>(st, tiles, a, sm);
  return GCMI_ERR_UNSUPPORTED;
}

// Dense layer behind the GraphGather: dy recomputed from the per-molecule gradient, dW (n_out x k_in, nn.Linear
// layout) += G^T P, db += colsum G, dP = G W.  One segment, its rows from 0.
int fused_dense_bwd(const BlockBackward& b, hipStream_t sm) {
  const int32_t k_in = b.k_in, act_bf16 = b.act_bf16;
  if (!fused_bwd_enabled() || b.width != 128 || k_in <= 32 || k_in > 64 || b.coef == nullptr) return GCMI_ERR_UNSUPPORTED;
  if (b.rg == nullptr || b.n_seg != 1 || b.seg_begin[0] != 0) return GCMI_ERR_UNSUPPORTED;
  const ReadoutGrad& rg = *b.rg;
  const int64_t n_rows = b.seg_end[0], ldd = b.ldgc, ldp = b.in[0].ld, lddp = b.dout[0].ld;
  if (!aligned16(rg.g2) || rg.ldg2 % 4 || !aligned16(rg.arg) || !aligned16(b.gc) || ldd % 4 || !aligned16(b.coef))
    return GCMI_ERR_UNSUPPORTED;
  if (n_rows <= 0 || k_in % 4 || lddp % 4 || !aligned16(b.dout[0].rows)) return GCMI_ERR_UNSUPPORTED;
  if (n_rows * std::max<int64_t>(std::max(ldd, rg.ldg2), std::max(ldp, lddp)) >= (int64_t)1 << 30) return GCMI_ERR_UNSUPPORTED;
  SegTable st;
  const int tiles = (int)fill_seg_table(st, 1, b.seg_begin, b.seg_end, b.w_off[0], nullptr, b.b_off, kFRows);
  const FusedArgs a = fused_args(b);
  if (act_bf16) {  // gc and in[0] point to bf16 rows
    if (!aligned16(b.in[0].rows) || ldp % 4) return GCMI_ERR_UNSUPPORTED;
    if (act_bf16 == 2) return launch_fused<128, 2, 1, true, true, true, true, true>(st, tiles, a, sm);  // dout[0]: bf16 rows
    return launch_fused<128, 2, 1, true, true, true, true>(st, tiles, a, sm);
  }
  return launch_fused<128, 2, 1, true, true, true>(st, tiles, a, sm);
}

}  // namespace gcmi

using namespace gcmi;

// The one-pass backward kernels alone: the argument checks, the BlockBackward description, the launcher -- and no
// separate kernels behind a refusal.
static int check_block_backward(const BlockBackward& b, const char* who, bool dense) {
  GCMI_CHECK_ARG(b.n_seg >= 1 && b.n_seg <= kMaxProductSeg, "%s: n_seg %d outside [1,%d]", who, b.n_seg, kMaxProductSeg);
  GCMI_CHECK_ARG(b.seg_begin && b.seg_end && b.w_off[0] && (dense || b.w_off[1]), "%s: NULL segment table", who);
  for (int s = 0; s < b.n_seg; ++s)
    GCMI_CHECK_ARG(b.seg_end[s] >= b.seg_begin[s] && b.seg_begin[s] >= 0, "%s: bad segment %d", who, s);
  GCMI_CHECK_ARG(b.act_bf16 >= 0 && b.act_bf16 <= 2 && (b.in_bf16 == 0 || b.in_bf16 == 1), "%s: bad storage flags", who);
  GCMI_CHECK_ARG(b.gc && b.in[0].rows && (dense || b.in[1].rows) && b.w && b.dw && (dense || b.dy), "%s: NULL buffer", who);
  GCMI_CHECK_ARG(b.db == nullptr || b.b_off != nullptr, "%s: db without offsets", who);
  GCMI_CHECK_ARG(b.k_in > 0 && b.in[0].ld >= b.k_in && (dense || b.in[1].ld >= b.k_in), "%s: ld < k_in in the input rows",
                 who);
  // (fp32 input rows are read as 16-byte pieces; the launchers look at this for bf16 rows only)
  GCMI_CHECK_ARG(b.act_bf16 || b.in_bf16 || (aligned16(b.in[0].rows) && b.in[0].ld % 4 == 0 &&
                                              (dense || (aligned16(b.in[1].rows) && b.in[1].ld % 4 == 0))),
                 "%s: float input rows must be 16-byte aligned with ld %% 4 == 0", who);
  GCMI_CHECK_ARG(b.ldgc >= b.width && (dense || b.lddy >= b.width), "%s: ld < %d in the rows of dy / gc", who, b.width);
  GCMI_CHECK_ARG(dense || (b.dout[0].rows == nullptr) == (b.dout[1].rows == nullptr), "%s: both input gradients or neither",
                 who);
  GCMI_CHECK_ARG(!dense || b.dout[0].rows != nullptr, "%s: NULL input gradient", who);
  GCMI_CHECK_ARG(b.dout[0].rows == nullptr || (b.dout[0].ld >= b.k_in && (dense || b.dout[1].ld >= b.k_in)),
                 "%s: ld < k_in in the input-gradient rows", who);
  GCMI_CHECK_ARG(b.psums == nullptr || b.dout[0].rows != nullptr, "%s: psums without input gradients", who);
  if (dense) {
    const ReadoutGrad& rg = *b.rg;
    GCMI_CHECK_ARG(rg.membership && rg.g2 && rg.arg, "%s: NULL readout gradient", who);
    GCMI_CHECK_ARG(rg.n_mols > 0 && rg.ldg2 >= 2 * (int64_t)b.width, "%s: ldg2 < 2 x %d or no molecules", who, b.width);
  }
  return GCMI_OK;
}

extern "C" {

int gcmi_fused_conv_bwd(int32_t n_seg, const int32_t* seg_begin, const int32_t* seg_end, const int64_t* w_rel_off,
                        const int64_t* w_self_off, const int64_t* b_off, const void* d_dy, int64_t lddy,
                        const void* d_gc, int64_t ldgc, const float* d_coef, const void* d_s, int64_t lds,
                        const void* d_x, int64_t ldx, int32_t k_in, const float* d_w, float* d_dw, float* d_db,
                        void* d_ds, int64_t ldds, void* d_dxs, int64_t lddxs, double* d_psums, int32_t act_bf16,
                        int32_t in_bf16, void* stream) {
  BlockBackward b;
  b.n_seg = n_seg; b.seg_begin = seg_begin; b.seg_end = seg_end;
  b.w_off[0] = w_rel_off; b.w_off[1] = w_self_off; b.b_off = b_off;
  b.dy = static_cast<const float*>(d_dy); b.lddy = lddy;
  b.gc = static_cast<const float*>(d_gc); b.ldgc = ldgc; b.coef = d_coef; b.width = 64;
  b.in[0] = {static_cast<const float*>(d_s), lds}; b.in[1] = {static_cast<const float*>(d_x), ldx};
  b.k_in = k_in; b.w = d_w; b.dw = d_dw; b.db = d_db;
  b.dout[0] = {static_cast<float*>(d_ds), ldds}; b.dout[1] = {static_cast<float*>(d_dxs), lddxs};
  b.psums = d_psums; b.act_bf16 = act_bf16; b.in_bf16 = in_bf16;
  const int rc_args = check_block_backward(b, "fused_conv_bwd", false);
  if (rc_args != GCMI_OK) return rc_args;
  const int rc = fused_conv_bwd(b, (hipStream_t)stream);
  if (rc == GCMI_ERR_UNSUPPORTED)
    set_error("fused_conv_bwd: exact mode, the one-pass kernels switched off, or a shape they do not cover (no other "
              "kernel stands behind this entry)");
  return rc;
}

int gcmi_fused_dense_bwd(int32_t n_seg, const int32_t* seg_begin, const int32_t* seg_end, const int64_t* w_off,
                         const int64_t* b_off, const int32_t* d_membership, const float* d_g2, int64_t ldg2,
                         const int32_t* d_arg, int32_t n_mols, const void* d_gc, int64_t ldgc, const float* d_coef,
                         const void* d_p, int64_t ldp, int32_t k_in, const float* d_w, float* d_dw, float* d_db,
                         void* d_dp, int64_t lddp, double* d_psums, int32_t act_bf16, void* stream) {
  ReadoutGrad rg;
  memset(&rg, 0, sizeof(rg));
  rg.membership = d_membership; rg.g2 = d_g2; rg.ldg2 = ldg2; rg.arg = d_arg; rg.n_mols = n_mols;
  BlockBackward b;
  b.n_seg = n_seg; b.seg_begin = seg_begin; b.seg_end = seg_end;
  b.w_off[0] = w_off; b.b_off = b_off; b.rg = &rg;
  b.gc = static_cast<const float*>(d_gc); b.ldgc = ldgc; b.coef = d_coef; b.width = 128;
  b.in[0] = {static_cast<const float*>(d_p), ldp};
  b.k_in = k_in; b.w = d_w; b.dw = d_dw; b.db = d_db;
  b.dout[0] = {static_cast<float*>(d_dp), lddp};
  b.psums = d_psums; b.act_bf16 = act_bf16;
  const int rc_args = check_block_backward(b, "fused_dense_bwd", true);
  if (rc_args != GCMI_OK) return rc_args;
  const int rc = fused_dense_bwd(b, (hipStream_t)stream);
  if (rc == GCMI_ERR_UNSUPPORTED)
    set_error("fused_dense_bwd: exact mode, the one-pass kernels switched off, or a shape they do not cover (no other "
              "kernel stands behind this entry)");
  return rc;
}

}  // extern "C"
