// LDS-window forms of the three gather kernels: GraphConv.sum_neigh
// (models/torch_models/layers.py:6236-6246), GraphPool.forward (:6319-6367) and its backward.
//
// Every neighbour of an atom belongs to the atom's own molecule.  The collation
// (gcmi_collate_plans) groups consecutive molecules into windows of ~win_cap atoms; because each
// degree block of the batch is sorted by molecule, the atoms of a window are <= 11 CONTIGUOUS row
// ranges (one per degree block).  A persistent workgroup walks windows:
//
//   * the rows of window i+1 stream HBM -> LDS by LDS-DMA (global_load_lds_dwordx4: no VGPRs, the
//     per-lane SOURCE address does the row-range lookup, the LDS image is slot-major and
//     lane-linear) while window i is being computed from the other LDS buffer;
//   * the neighbour lists of the window (uint16 LDS slots, window-major in HBM) arrive the same
//     way, so the compute phase touches HBM only to store results;
//   * the window descriptors (24 ints) are fetched three windows ahead into an LDS ring;
//   * while window i+1 is staged, thread = slot looks up each of its slots' degree and first neighbour entry once
//     and leaves them in a table in LDS (WinSlots): the compute phase reads the table per 16-byte piece and does
//     not search the degree blocks 16 to 32 times per atom.
//
// HBM traffic drops from E*(4F+4) + N*4F (every neighbour row fetched once per edge) to
// N*4F + 2E + N*4F: each row is read ONCE; the (1+E/N)-fold re-reads are served by LDS.  The
// algorithmic figure of SURVEY.md 8d is therefore delivered above the HBM roofline.
#include "common.h"
#include "split_bf16.h"

namespace gcmi {

constexpr int kND = GCMI_MAX_DEG + 1;
constexpr int kLdsPerCU = 160 * 1024;
constexpr int kRingBytes = 320;                 // 3 descriptors of GCMI_WIN_META_INTS ints, 16-byte padded
constexpr int kHeadBytes = kRingBytes + 2048;   // + the per-op constants and the two slot tables
// the 2 048 bytes behind the ring: [scale: 128 floats][shift: 128 floats][slot table of buffer 0][of buffer 1]
// (no window kernel has rows above 128 columns: win_has_width, win_usable_h)
constexpr int kShiftAt = 128;                   // floats
constexpr int kTabSlots = 128;                  // slots of one table: ordinary windows above it search per piece
constexpr int kTabAt = 2 * kShiftAt * 4;        // bytes
static_assert(kTabAt + 2 * kTabSlots * 4 <= 2048, "the slot tables live inside the head");
static_assert(kTabSlots * GCMI_MAX_DEG < (1 << 28), "a table entry is degree | first entry << 4");

typedef __attribute__((address_space(3))) void* lds_ptr_t;

// LDS-DMA: 64 lanes x 16 (4) bytes from per-lane global addresses to LDS [dst, dst + 1024 (256)).
// Written as asm on purpose: for the builtin hipcc (ROCm 7.2) waits vmcnt(0) before EVERY later
// ds_read of the same LDS array (it cannot tell the buffer being filled from the one being read),
// which would serialise the fill of window i+1 with the compute of window i.  The kernel waits
// for these loads itself (wait_dma) before the barrier that publishes a buffer.
__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lds_ptr_t)p);
}
__device__ __forceinline__ void glds16(const void* gsrc, unsigned lds_dst) {
  unsigned keep;
  lds_dst = __builtin_amdgcn_readfirstlane(lds_dst);  // wave-uniform by construction
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ void glds4(const void* gsrc, unsigned lds_dst) {
  unsigned keep;
  lds_dst = __builtin_amdgcn_readfirstlane(lds_dst);
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ void wait_dma() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// The row ranges of one window, read from the LDS ring of window descriptors.
struct WinMeta {
  int rb[kND];      // global row of slot s (degree d) = rb[d] + s
  int sb[kND + 1];  // first slot of degree d; sb[kND] = atoms in the window
  int eoff;         // first entry of the window in win_edges (multiple of 8)
  int ne;           // edge entries of the window
};

__device__ __forceinline__ WinMeta read_meta(const int* ring_slot) {
  WinMeta m;
#pragma unroll
  for (int d = 0; d < kND; ++d) m.rb[d] = ring_slot[d];
  m.sb[0] = 0;
#pragma unroll
  for (int d = 1; d <= kND; ++d) m.sb[d] = ring_slot[kND - 1 + d];
  m.eoff = ring_slot[2 * kND];
  m.ne = ring_slot[2 * kND + 1];
  return m;
}

// slot -> (degree, global row, first entry of its neighbour list inside the window);
// maxd = highest degree present in the batch (uniform)
__device__ __forceinline__ void locate(const WinMeta& m, int maxd, int slot, int& d, int& row, int& eloc) {
  d = 0;
  int rb = m.rb[0], eb = 0, eacc = 0;
#pragma unroll
  for (int k = 1; k < kND; ++k) {
    if (k <= maxd) {
      eacc += (m.sb[k] - m.sb[k - 1]) * (k - 1);  // entries of the degrees below k
      const bool ge = slot >= m.sb[k];
      d = ge ? k : d;
      rb = ge ? m.rb[k] : rb;
      eb = ge ? eacc - m.sb[k] * k : eb;
    }
  }
  row = rb + slot;
  eloc = eb + slot * d;
}

__device__ __forceinline__ int row_of_slot(const WinMeta& m, int maxd, int slot) {
  int rb = m.rb[0];
#pragma unroll
  for (int k = 1; k < kND; ++k)
    if (k <= maxd) rb = slot >= m.sb[k] ? m.rb[k] : rb;
  return rb + slot;
}

// LDS image of one buffer: [tile: alloc*LPR float4][aux: alloc*LPR*4 bytes (optional)][edges]
// tab: every window of this shape has at most kTabSlots slots (the compute phase reads a slot table: WinSlots)
struct Layout {
  int tile_bytes, aux_bytes, edge_bytes, maxd, tab;
  __host__ __device__ int buf_bytes() const { return tile_bytes + aux_bytes + edge_bytes; }
};

// Issue the LDS-DMA of one window: rows of `x` (and of the byte matrix `aux`, F bytes per row)
// and the window's neighbour entries.  Nothing waits here.
// (x: rows of LPR 16-byte pieces -- 4 floats or 8 bf16 each --, ldx in BYTES: the DMA moves bytes, not elements)
// AUX: the byte matrix `aux` (one byte per element) rides along.  Four elements per piece (fp32 rows): one dword per
// piece, aux32[e].  Eight (bf16 rows, EPP 8): two dwords per piece by two DMA instructions, each of which writes 64
// lanes x 4 bytes side by side -- so per 64 pieces the image is [64 low dwords][64 high dwords] (Piece<bf16_t>::arg).
template <int WT, int LPR, bool AUX, int EPP = 4>
__device__ __forceinline__ void stage(char* buf, const Layout& L, const WinMeta& m,
                                      const char* __restrict__ x, int64_t ldx,
                                      const uint8_t* __restrict__ aux,
                                      const uint16_t* __restrict__ edges) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int n16 = m.sb[kND] * LPR;
  const unsigned base = lds_addr(buf);
  for (int e0 = tid - lane; e0 < n16; e0 += WT) {  // e0: wave-uniform first chunk of this piece
    const int e = e0 + lane;
    if (e < n16) {
      const int slot = e / LPR;
      const int c = e - slot * LPR;
      const int row = row_of_slot(m, L.maxd, slot);
      glds16(x + (int64_t)row * ldx + c * 16, base + e0 * 16);
      if constexpr (AUX && EPP == 4) glds4(aux + (int64_t)row * (LPR * 4) + c * 4, base + L.tile_bytes + e0 * 4);
      if constexpr (AUX && EPP == 8) {
        glds4(aux + (int64_t)row * (LPR * 8) + c * 8, base + L.tile_bytes + (e0 >> 6) * 512);
        glds4(aux + (int64_t)row * (LPR * 8) + c * 8 + 4, base + L.tile_bytes + (e0 >> 6) * 512 + 256);
      }
    }
  }
  const int nq = (m.ne + 7) >> 3;  // 16-byte pieces of the neighbour entries
  const uint16_t* src = edges + m.eoff;
  for (int q0 = tid - lane; q0 < nq; q0 += WT) {
    const int q = q0 + lane;
    if (q < nq) glds16(src + (size_t)q * 8, base + L.tile_bytes + L.aux_bytes + q0 * 16);
  }
}

// The rows of a SECOND matrix of the window (same slots, same row pitch in pieces) into a tile of their own: ops whose
// compute phase would otherwise fetch them from HBM -- and wait, one in-order counter, for the next window's DMA with them.
template <int WT, int LPR>
__device__ __forceinline__ void stage_extra(char* dst, const Layout& L, const WinMeta& m, const char* __restrict__ x2,
                                            int64_t ldx2) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int n16 = m.sb[kND] * LPR;
  const unsigned base = lds_addr(dst);
  for (int e0 = tid - lane; e0 < n16; e0 += WT) {
    const int e = e0 + lane;
    if (e < n16) {
      const int slot = e / LPR;
      const int c = e - slot * LPR;
      glds16(x2 + (int64_t)row_of_slot(m, L.maxd, slot) * ldx2 + c * 16, base + e0 * 16);
    }
  }
}

// ---------------------------------------------------------------- one 16-byte piece of a tile row, per element type
// The only place that knows how many elements a piece holds, how they become floats and back, and where the arg-max
// bytes that ride with a piece (stage(), AUX) sit in the LDS image.  Vals / Bytes are indexed v[q]; fp32 keeps the vector types,
// handed on by reference: from a float[4], or a uchar4 by value, hipcc (ROCm 7.2) no longer forms the fp32 ops' packed adds.
template <class T>
struct Piece;

template <>
struct Piece<float> {
  static constexpr int kEPP = 4;  // elements per piece = aux bytes per piece
  using Raw = float4;
  using Vals = float4;   // the piece as floats, v[q]
  using Bytes = uchar4;  // a byte per element, b[q]
  using Arg = uchar4;  // the arg bytes of piece e: one dword, aux32[e]
  static __device__ __forceinline__ void widen(const Raw& r, Vals& v) { v = r; }
  static __device__ __forceinline__ Raw narrow(const Vals& v) { return v; }
  static __device__ __forceinline__ void load_vals(const float* p, Vals& v) { v = *reinterpret_cast<const float4*>(p); }
  static __device__ __forceinline__ Arg arg(const char* aux, int e) { return reinterpret_cast<const uchar4*>(aux)[e]; }
  static __device__ __forceinline__ unsigned char arg_byte(const Arg& a, int q) {
    return q == 0 ? a.x : q == 1 ? a.y : q == 2 ? a.z : a.w;
  }
  static __device__ __forceinline__ void store_arg(uint8_t* p, const Bytes& b) { *reinterpret_cast<uchar4*>(p) = b; }
};

// bf16 rows (gcmi_model_desc.storage >= 1): the LDS-DMA moves bytes, so a bf16 row of 64 is 8 pieces of 8 elements.
// Sums and maxima are formed in fp32 from the widened elements and rounded once (v_cvt_pk_bf16_f32) at the store.
template <>
struct Piece<bf16_t> {
  static constexpr int kEPP = 8;
  using Raw = uint4;
  using Vals = float[8];
  using Bytes = unsigned char[8];
  using Arg = uint2;  // two dwords in the split image stage() writes: per 64 pieces [64 low dwords][64 high dwords]
  static __device__ __forceinline__ void widen(const Raw& r, Vals& v) { widen8(r, v); }
  static __device__ __forceinline__ Raw narrow(const Vals& v) {
    uint4 o;
    o.x = pack_bf16x2(v[0], v[1]); o.y = pack_bf16x2(v[2], v[3]);
    o.z = pack_bf16x2(v[4], v[5]); o.w = pack_bf16x2(v[6], v[7]);
    return o;
  }
  static __device__ __forceinline__ void load_vals(const float* p, Vals& v) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    const float4 b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
  static __device__ __forceinline__ Arg arg(const char* aux, int e) {
    const unsigned* a = reinterpret_cast<const unsigned*>(aux) + (e >> 6) * 128 + (e & 63);
    return make_uint2(a[0], a[64]);
  }
  static __device__ __forceinline__ unsigned char arg_byte(const Arg a, int q) {
    return (unsigned char)((q < 4 ? a.x >> (8 * q) : a.y >> (8 * (q - 4))) & 255u);
  }
  static __device__ __forceinline__ void store_arg(uint8_t* p, const Bytes& b) {
    uint2 av;
    av.x = (unsigned)b[0] | ((unsigned)b[1] << 8) | ((unsigned)b[2] << 16) | ((unsigned)b[3] << 24);
    av.y = (unsigned)b[4] | ((unsigned)b[5] << 8) | ((unsigned)b[6] << 16) | ((unsigned)b[7] << 24);
    *reinterpret_cast<uint2*>(p) = av;
  }
};

template <class T>
__device__ __forceinline__ typename Piece<T>::Raw load_piece(const T* p) {
  return *reinterpret_cast<const typename Piece<T>::Raw*>(p);
}
template <class T>
__device__ __forceinline__ void store_piece(T* p, const typename Piece<T>::Vals& v) {
  *reinterpret_cast<typename Piece<T>::Raw*>(p) = Piece<T>::narrow(v);
}

// One window buffer as a compute phase reads it, and what piece e of it is
template <class P>
struct WinBuf {
  const typename P::Raw* tile;  // [slot][LPR] pieces
  const char* aux;              // the arg-max bytes of the same pieces (ops launched with AUX)
  const uint16_t* ent;          // the window's neighbour entries
  int n16;                      // pieces in the window
};
template <class P, int LPR>
__device__ __forceinline__ WinBuf<P> open_buf(const char* buf, const Layout& L, int n_slots) {
  return {reinterpret_cast<const typename P::Raw*>(buf), buf + L.tile_bytes,
          reinterpret_cast<const uint16_t*>(buf + L.tile_bytes + L.aux_bytes), n_slots * LPR};
}

// What a compute phase knows about the slots of its window.
//   TAB   the window's slot table in LDS: the degree of a slot is looked up ONCE per window, by thread = slot while
//         the window is staged (fill_slot_table), not once per 16-byte piece of its row -- 16 to 32 times per atom;
//   !TAB  the descriptor itself, searched per piece (locate): oversized windows, and ordinary windows of a batch whose
//         largest one has more than kTabSlots atoms (Layout::tab, uniform over the grid).
template <bool TAB>
struct WinSlots;
template <>
struct WinSlots<true> {
  const unsigned* tab;  // [slot] degree | first neighbour entry << 4
  const int* rb;        // the window's descriptor in the ring: row of slot s (degree d) = rb[d] + s
  int n;                // atoms in the window
};
template <>
struct WinSlots<false> {
  WinMeta m;
  int maxd;
  int n;
};

// thread = slot; the barrier that publishes the window's buffer publishes its table
__device__ __forceinline__ void fill_slot_table(unsigned* tab, const WinMeta& m, int maxd) {
  const int slot = threadIdx.x;
  if (slot < m.sb[kND]) {
    int d, row, eloc;
    locate(m, maxd, slot, d, row, eloc);
    tab[slot] = (unsigned)d | ((unsigned)eloc << 4);
  }
}

struct PieceAt {
  int c;            // piece within the row
  int d;            // the atom's degree
  int row;          // its global row
  int eloc;         // first of its d neighbour entries
};
// the single place a compute phase gets (c, d, row, eloc) of piece e from
template <int LPR>
__device__ __forceinline__ PieceAt piece_at(const WinSlots<true>& w, int e) {
  const int slot = e / LPR;
  const unsigned v = w.tab[slot];
  PieceAt a;
  a.c = e - slot * LPR;
  a.d = (int)(v & 15u);
  a.eloc = (int)(v >> 4);
  a.row = w.rb[a.d] + slot;
  return a;
}
template <int LPR>
__device__ __forceinline__ PieceAt piece_at(const WinSlots<false>& w, int e) {
  const int slot = e / LPR;
  PieceAt a;
  a.c = e - slot * LPR;
  locate(w.m, w.maxd, slot, a.d, a.row, a.eloc);
  return a;
}

// ---------------------------------------------------------------- the three inner loops over a piece, each written once
// Piece c of the rows in `tile` ([slot][LPR]); nb: the atom's d neighbour entries.  Every op below -- and both stages of
// the two-stage ops -- forms its sums and comparisons here, so the two-stage pass and the separate passes that take
// its place for oversized windows agree bit for bit by construction.

// acc = sum of the neighbours' pieces, in neighbour order
template <class P, int LPR>
__device__ __forceinline__ void neigh_sum(const typename P::Raw* tile, const uint16_t* nb, int d, int c,
                                          typename P::Vals& acc) {
#pragma unroll
  for (int q = 0; q < P::kEPP; ++q) acc[q] = 0.f;  // lone atoms: zero
  for (int j = 0; j < d; ++j) {
    const int sl = nb[j] & GCMI_WIN_MAX_SLOTS;
    typename P::Vals v;
    P::widen(tile[sl * LPR + c], v);
#pragma unroll
    for (int q = 0; q < P::kEPP; ++q) acc[q] += v[q];
  }
}
template <class P>
__device__ __forceinline__ void add_piece(typename P::Vals& acc, const typename P::Raw& r) {
  typename P::Vals v;
  P::widen(r, v);
#pragma unroll
  for (int q = 0; q < P::kEPP; ++q) acc[q] += v[q];
}

// GraphPool: the maximum over the atom's own piece e and its neighbours', BN: of y = x * scale + shift in fp32 (the
// folded BatchNorm, [scale: 128][shift: 128] floats in LDS); the first maximum wins (self first, then neighbour order).
// ba: 0 = self, j + 1 = neighbour j
template <class P, int LPR, bool BN>
__device__ __forceinline__ void pool_max(const typename P::Raw* tile, const uint16_t* nb, int d, int e, int c,
                                         const float* sh_lds, typename P::Vals& best, typename P::Bytes& ba) {
  typename P::Vals sc, sh;
  if (BN) {
    P::load_vals(sh_lds + c * P::kEPP, sc);
    P::load_vals(sh_lds + kShiftAt + c * P::kEPP, sh);
  }
  P::widen(tile[e], best);  // self first
#pragma unroll
  for (int q = 0; q < P::kEPP; ++q) {
    if (BN) best[q] = fmaf(best[q], sc[q], sh[q]);
    ba[q] = 0;
  }
  for (int j = 0; j < d; ++j) {
    const int sl = nb[j] & GCMI_WIN_MAX_SLOTS;
    typename P::Vals v;
    P::widen(tile[sl * LPR + c], v);
    const unsigned char a = (unsigned char)(j + 1);
#pragma unroll
    for (int q = 0; q < P::kEPP; ++q) {
      if (BN) v[q] = fmaf(v[q], sc[q], sh[q]);
      if (v[q] > best[q]) { best[q] = v[q]; ba[q] = a; }  // strict >: the first maximum wins
    }
  }
}

// GraphPool backward: acc[k] = g[k]*[arg[k]==0] + sum_j g[i_j]*[arg[i_j] == rev_pos(k,j)+1], g = the rows in `tile`,
// arg = the bytes in `aux`; the reverse slot rides in the high bits of a neighbour entry
template <class P, int LPR>
__device__ __forceinline__ void pool_bwd(const typename P::Raw* tile, const char* aux, const uint16_t* nb, int d, int e,
                                         int c, typename P::Vals& acc) {
  typename P::Vals g;
  P::widen(tile[e], g);
  typename P::Arg a = P::arg(aux, e);
#pragma unroll
  for (int q = 0; q < P::kEPP; ++q) acc[q] = P::arg_byte(a, q) == 0 ? g[q] : 0.f;
  for (int j = 0; j < d; ++j) {
    const int en = nb[j];
    const int sl = en & GCMI_WIN_MAX_SLOTS;
    const unsigned char want = (unsigned char)((en >> GCMI_WIN_SLOT_BITS) + 1);
    P::widen(tile[sl * LPR + c], g);
    a = P::arg(aux, sl * LPR + c);
#pragma unroll
    for (int q = 0; q < P::kEPP; ++q) acc[q] += P::arg_byte(a, q) == want ? g[q] : 0.f;
  }
}

// ---------------------------------------------------------------- per-window compute phases
// A body holds an operation's fields and its walk over the pieces of a window, for rows of T; the op types below it
// (the names profiles and bench.py know the kernels by) add what was measured per element type:
//   kThreads  threads per workgroup;
//   kPre      pieces per thread and round.  kPre = 4 (fp32 SumOp and MaxBwdOp): rows the thread also needs from HBM in
//             the compute phase (the old value of an accumulated output) are requested for kPre pieces up front,
//             unconditionally from clamped addresses, and used after the LDS work of all of them: the wait for them is
//             also a wait for the LDS-DMA of the next window (one counter, in order), which the loop would wait for at
//             its top anyway.  kPre = 1: one piece at a time, the old piece loaded before its neighbour loop.


// What a two-stage op keeps behind the two window buffers, in tiles the size of a window tile (Op::kThird):
//   dma_pair  one per window buffer, filled by the LDS-DMA with the window's rows of a second matrix (stage_extra);
//   scratch   one per workgroup, written and read by the compute phase of one window only.
enum class Third { none, dma_pair, scratch };
constexpr int third_tiles(Third k) { return k == Third::dma_pair ? 2 : k == Third::scratch ? 1 : 0; }

// s = (ACC: s +) sum of the neighbours' rows (ACC: the transposed gather of a backward pass onto the self term)
template <class Op, class T, bool ACC>
struct SumBody {
  using P = Piece<T>;
  T* __restrict__ s;
  int64_t lds;
  static constexpr Third kThird = Third::none;
  __device__ __forceinline__ bool skip(int) const { return false; }
  template <int WT>
  __device__ __forceinline__ void init(float*, int) const {}
  template <int WT, int LPR, class S>
  __device__ __forceinline__ void run(const char* buf, const Layout& L, const S& sl, const float*) const {
    constexpr int kPre = Op::kPre;
    const WinBuf<P> w = open_buf<P, LPR>(buf, L, sl.n);
    for (int e0 = threadIdx.x; e0 < w.n16; e0 += kPre * WT) {
      typename P::Raw old[kPre];
      if constexpr (ACC && kPre > 1) {
#pragma unroll
        for (int k = 0; k < kPre; ++k) {
          const int e = e0 + k * WT < w.n16 ? e0 + k * WT : w.n16 - 1;
          const PieceAt at = piece_at<LPR>(sl, e);
          old[k] = load_piece(s + (int64_t)at.row * lds + at.c * P::kEPP);
        }
      }
#pragma unroll
      for (int k = 0; k < kPre; ++k) {
        const int e = e0 + k * WT;
        if (e >= w.n16) break;
        const PieceAt at = piece_at<LPR>(sl, e);
        T* dst = s + (int64_t)at.row * lds + at.c * P::kEPP;
        if constexpr (ACC && kPre == 1) old[0] = load_piece(dst);
        typename P::Vals acc;
        neigh_sum<P, LPR>(w.tile, w.ent + at.eloc, at.d, at.c, acc);
        if constexpr (ACC) add_piece<P>(acc, old[k]);
        store_piece(dst, acc);
      }
    }
  }
};

template <bool ACC>
struct SumOp : SumBody<SumOp<ACC>, float, ACC> {
  static constexpr int kThreads = 512;  // measured (76 columns, us per launch): 179 / 127 / 149 at 256 / 512 / 1 024
  static constexpr int kPre = 4;
};
// GraphConv.sum_neigh over rows stored as bf16 (the pooled rows of the block below): bf16 in, bf16 out
struct SumOpH : SumBody<SumOpH, bf16_t, false> {
  static constexpr int kThreads = 256;  // measured (64 columns, 1.2 M atoms): 58.6 us against 74.4 at 512 and 93.4 at 1 024
  static constexpr int kPre = 1;
};
// s += sum of the neighbours' rows, bf16 in and out (the oversized windows of the two-stage pass over bf16 gradients)
struct SumAccOpH : SumBody<SumAccOpH, bf16_t, true> {
  static constexpr int kThreads = 512;
  static constexpr int kPre = 1;
};

// First GraphConv at bf16 storage: the atom features arrive as fp32 rows (the caller's matrix); the sum of the
// neighbours' rows goes out as bf16, and so does a bf16 copy of the atom's OWN row (it is in LDS anyway), so that the
// product that follows and the backward read two bf16 operands and the fp32 matrix is read exactly once per step.
// Output rows are `ldo` elements; the `pad4` groups of four columns behind the LPR pieces are zeroed (76 -> 80 columns:
// 16-byte rows).
struct SumOpFH {
  using P = Piece<float>;
  bf16_t* __restrict__ s;
  bf16_t* __restrict__ xcopy;
  int64_t ldo;
  int pad4;
  static constexpr Third kThird = Third::none;
  static constexpr int kThreads = 512;
  __device__ __forceinline__ bool skip(int) const { return false; }
  template <int WT>
  __device__ __forceinline__ void init(float*, int) const {}
  template <int WT, int LPR, class S>
  __device__ __forceinline__ void run(const char* buf, const Layout& L, const S& sl, const float*) const {
    const WinBuf<P> w = open_buf<P, LPR>(buf, L, sl.n);
    for (int e = threadIdx.x; e < w.n16; e += WT) {
      const PieceAt at = piece_at<LPR>(sl, e);
      P::Vals acc;
      neigh_sum<P, LPR>(w.tile, w.ent + at.eloc, at.d, at.c, acc);
      const float4 own = w.tile[e];
      bf16_t* srow = s + (int64_t)at.row * ldo + at.c * 4;
      bf16_t* xrow = xcopy + (int64_t)at.row * ldo + at.c * 4;
      *reinterpret_cast<uint2*>(srow) = narrow4(acc[0], acc[1], acc[2], acc[3]);
      *reinterpret_cast<uint2*>(xrow) = narrow4(own.x, own.y, own.z, own.w);
      if (at.c == LPR - 1) {
        for (int z = 1; z <= pad4; ++z) {
          *reinterpret_cast<uint2*>(srow + 4 * z) = make_uint2(0u, 0u);
          *reinterpret_cast<uint2*>(xrow + 4 * z) = make_uint2(0u, 0u);
        }
      }
    }
  }
};

// GraphPool.forward with the folded BatchNorm applied on the fly (BN), the winner stored (bf16: rounded once) with its
// arg-max bytes
template <class T, bool BN>
struct MaxBody {
  using P = Piece<T>;
  const float* __restrict__ scale;
  const float* __restrict__ shift;
  T* __restrict__ out;
  int64_t ldo;
  uint8_t* __restrict__ arg;
  static constexpr Third kThird = Third::none;
  __device__ __forceinline__ bool skip(int) const { return false; }
  // the folded BatchNorm vectors live in LDS: a global load in the compute phase would make the
  // compiler wait for the LDS-DMA in flight as well
  template <int WT>
  __device__ __forceinline__ void init(float* sh_lds, int n_feat) const {
    if (BN)
      for (int i = threadIdx.x; i < n_feat; i += WT) {
        sh_lds[i] = scale[i];
        sh_lds[kShiftAt + i] = shift[i];
      }
  }
  template <int WT, int LPR, class S>
  __device__ __forceinline__ void run(const char* buf, const Layout& L, const S& sl, const float* sh_lds) const {
    const WinBuf<P> w = open_buf<P, LPR>(buf, L, sl.n);
    for (int e = threadIdx.x; e < w.n16; e += WT) {
      const PieceAt at = piece_at<LPR>(sl, e);
      typename P::Vals best;
      typename P::Bytes ba;
      pool_max<P, LPR, BN>(w.tile, w.ent + at.eloc, at.d, e, at.c, sh_lds, best, ba);
      store_piece(out + (int64_t)at.row * ldo + at.c * P::kEPP, best);
      if (arg) P::store_arg(arg + (int64_t)at.row * (LPR * P::kEPP) + at.c * P::kEPP, ba);
    }
  }
};

template <bool BN>
struct MaxOp : MaxBody<float, BN> {
  // measured at 1.2 M atoms, 64 columns (us per launch): 256 threads 131 / 137, 512: 151 / 156, 1 024: 137 / 137 (the
  // gather-sum is the other way round: 179 / 127 / 149 for 76 columns; the GraphPool backward 166 / 126 / 141)
  static constexpr int kThreads = 256;
};
template <bool BN>
struct MaxOpH : MaxBody<bf16_t, BN> {
  static constexpr int kThreads = 512;
};

// GraphPool backward via the reverse slots: tile = dout rows, aux = arg rows of the window
template <class Op, class T>
struct MaxBwdBody {
  using P = Piece<T>;
  T* __restrict__ dx;
  int64_t lddx;
  // optional (bn_bwd_pool_impl): dx is needed only where the pooled BatchNorm sums are ill-conditioned
  const float* __restrict__ only_if_gamma;
  const float* __restrict__ only_if_beta;
  static constexpr Third kThird = Third::none;
  __device__ __forceinline__ bool skip(int n_feat) const {
    return only_if_gamma != nullptr && !bn_pool_ill_conditioned(only_if_gamma, only_if_beta, n_feat);
  }
  template <int WT>
  __device__ __forceinline__ void init(float*, int) const {}
  template <int WT, int LPR, class S>
  __device__ __forceinline__ void run(const char* buf, const Layout& L, const S& sl, const float*) const {
    constexpr int kPre = Op::kPre;
    const WinBuf<P> w = open_buf<P, LPR>(buf, L, sl.n);
    for (int e0 = threadIdx.x; e0 < w.n16; e0 += kPre * WT) {
#pragma unroll
      for (int k = 0; k < kPre; ++k) {
        const int e = e0 + k * WT;
        if (e >= w.n16) break;
        const PieceAt at = piece_at<LPR>(sl, e);
        typename P::Vals acc;
        pool_bwd<P, LPR>(w.tile, w.aux, w.ent + at.eloc, at.d, e, at.c, acc);
        store_piece(dx + (int64_t)at.row * lddx + at.c * P::kEPP, acc);
      }
    }
  }
};

struct MaxBwdOp : MaxBwdBody<MaxBwdOp, float> {
  static constexpr int kThreads = 512;  // measured (us per launch): 166 / 126 / 141 at 256 / 512 / 1 024
  static constexpr int kPre = 4;
};
struct MaxBwdOpH : MaxBwdBody<MaxBwdOpH, bf16_t> {
  static constexpr int kThreads = 256;  // measured: 84.4 us against 92.6 at 512 and 119 at 1 024
  static constexpr int kPre = 1;
};

// The backward between two GraphConv blocks in one window pass:
//   dX[k]  = dXs[k] + sum_j dS[i_j]                 (SumBody<ACC>: the neighbour part onto the self part)
//   dy[k]  = dX[k]*[arg[k]==0] + sum_j dX[i_j]*[arg[i_j] == rev_pos(k,j)+1]       (MaxBwdBody of the block below)
// dX is the gradient of the pooled rows and nothing else reads it, so it lives in a third LDS tile only: it is neither
// written (N*F elements) nor read back (N*F) through HBM.  tile = dS rows, aux = arg rows of the block below.  The
// price is LDS.  Oversized windows are not handled (the launcher refuses).
// The third tile is double-buffered and filled by the LDS-DMA with the window's dXs rows (stage_extra): read from HBM
// in the compute phase they waited, one in-order counter, for the NEXT window's DMA, so that no window's compute
// overlapped the next one's load (281 us at 96-atom windows against 181 at 192-atom ones: a fixed ~3.8 us per window).
// dX is completed IN PLACE in it, in the rows' own element type: over bf16 streams it is rounded to bf16 once, exactly
// what the two separate passes do when they write dX to HBM as a bf16 matrix between them.
template <class T>
struct SumAccMaxBwdBody {
  using P = Piece<T>;
  const T* __restrict__ dxs;  // self part of dX (global rows)
  int64_t lddxs;
  T* __restrict__ dy;
  int64_t lddy;
  static constexpr Third kThird = Third::dma_pair;
  __device__ __forceinline__ const char* extra_src() const { return reinterpret_cast<const char*>(dxs); }
  __device__ __forceinline__ int64_t extra_ld_bytes() const { return lddxs * (int64_t)sizeof(T); }
  __device__ __forceinline__ bool skip(int) const { return false; }
  template <int WT>
  __device__ __forceinline__ void init(float*, int) const {}
  // extra: the third tile of the window being computed, [slot][LPR] pieces, the dXs rows on entry
  template <int WT, int LPR, class S>
  __device__ __forceinline__ void run(const char* buf, const Layout& L, const S& sl, char* extra) const {
    const WinBuf<P> w = open_buf<P, LPR>(buf, L, sl.n);
    typename P::Raw* t2 = reinterpret_cast<typename P::Raw*>(extra);
    // ---- stage 1: dX of the window = gather(dS) + dXs, in place in the third tile
    for (int e = threadIdx.x; e < w.n16; e += WT) {
      const PieceAt at = piece_at<LPR>(sl, e);
      typename P::Vals acc;
      neigh_sum<P, LPR>(w.tile, w.ent + at.eloc, at.d, at.c, acc);
      add_piece<P>(acc, t2[e]);
      t2[e] = P::narrow(acc);
    }
    __syncthreads();
    // ---- stage 2: the GraphPool backward over it
    for (int e = threadIdx.x; e < w.n16; e += WT) {
      const PieceAt at = piece_at<LPR>(sl, e);
      typename P::Vals acc;
      pool_bwd<P, LPR>(t2, w.aux, w.ent + at.eloc, at.d, e, at.c, acc);
      store_piece(dy + (int64_t)at.row * lddy + at.c * P::kEPP, acc);
    }
    // (the walker's barrier at the top of the next window comes before the third tile is written again)
  }
};

// fp32 tiles hold one workgroup per CU by LDS, so make it a full one (1 024 threads: 292 us against 346 at 512)
struct SumAccMaxBwdOp : SumAccMaxBwdBody<float> {
  static constexpr int kThreads = 1024;
};
// bf16 tiles are half the size and two 512-thread workgroups share a CU (288 us against 367 at 1 024; two of 1 024
// would not fit a CU's thread limit)
struct SumAccMaxBwdOpH : SumAccMaxBwdBody<bf16_t> {
  static constexpr int kThreads = 512;
};

// The forward between two GraphConv blocks in one window pass: GraphPool of the block below (MaxBody), then the
// neighbour sum of the block above (SumBody) over the pooled rows of the window.
//   P[k] = max(y[k], y[i_j])   -> out (+ arg bytes),  and, as stored (narrow), into the third tile
//   S[k] = sum_j P[i_j]        -> s
// The pooled rows are still written (the product above and the backward read them) but not read back: the second
// launch's N*F elements from HBM, its neighbour entries and its window walk go.  The third tile is one scratch tile per
// workgroup: the DMA never touches it, and the walker's barrier at the top of the next window separates stage 2 of
// this window from stage 1 of the next.  Both stages call the loops the separate ops call, on the same values, so the
// pass equals MaxOp followed by SumOp bit for bit.  Oversized windows are not handled (the launcher refuses).
template <class T, bool BN>
struct MaxSumBody {
  using P = Piece<T>;
  MaxBody<T, BN> pool;  // scale, shift, out, ldo, arg
  T* __restrict__ s;
  int64_t lds;
  static constexpr Third kThird = Third::scratch;
  __device__ __forceinline__ bool skip(int) const { return false; }
  template <int WT>
  __device__ __forceinline__ void init(float* sh_lds, int n_feat) const { pool.template init<WT>(sh_lds, n_feat); }
  template <int WT, int LPR, class S>
  __device__ __forceinline__ void run(const char* buf, const Layout& L, const S& sl, const float* sh_lds,
                                      char* extra) const {
    const WinBuf<P> w = open_buf<P, LPR>(buf, L, sl.n);
    typename P::Raw* t2 = reinterpret_cast<typename P::Raw*>(extra);
    // ---- stage 1: the GraphPool of the window, to HBM and into the third tile
    for (int e = threadIdx.x; e < w.n16; e += WT) {
      const PieceAt at = piece_at<LPR>(sl, e);
      typename P::Vals best;
      typename P::Bytes ba;
      pool_max<P, LPR, BN>(w.tile, w.ent + at.eloc, at.d, e, at.c, sh_lds, best, ba);
      store_piece(pool.out + (int64_t)at.row * pool.ldo + at.c * P::kEPP, best);
      if (pool.arg) P::store_arg(pool.arg + (int64_t)at.row * (LPR * P::kEPP) + at.c * P::kEPP, ba);
      t2[e] = P::narrow(best);
    }
    __syncthreads();
    // ---- stage 2: the neighbour sum over the pooled rows
    for (int e = threadIdx.x; e < w.n16; e += WT) {
      const PieceAt at = piece_at<LPR>(sl, e);
      typename P::Vals acc;
      neigh_sum<P, LPR>(t2, w.ent + at.eloc, at.d, at.c, acc);
      store_piece(s + (int64_t)at.row * lds + at.c * P::kEPP, acc);
    }
  }
};

// measured at 1.2 M atoms (us per launch, with arg bytes; MaxOp + SumOp on the same rows: 248 and 752):
//   64 columns (two workgroups per CU by LDS):  253 / 186 / 206 at 256 / 512 / 1 024 threads
//   128 columns (one workgroup per CU by LDS):  846 / 477 / 378
// so the launcher picks WT by the width (max_sum below)
template <bool BN, int WT>
struct MaxSumOp : MaxSumBody<float, BN> {
  static constexpr int kThreads = WT;
};

// ---------------------------------------------------------------- the persistent window walker
// Workgroups [0, g_norm) walk the ordinary windows double-buffered; workgroups [g_norm, gridDim)
// walk the oversized windows (one big molecule each) using both buffers as one.
template <int WT, int LPR, bool AUX, class Op>
__global__ void __launch_bounds__(WT)
win_kernel(const int32_t* __restrict__ meta, const uint16_t* __restrict__ edges, int n_norm, int n_win,
           int g_norm, Layout L, Layout Lbig, const char* __restrict__ x, int64_t ldx,
           const uint8_t* __restrict__ aux, Op op, int rev) {
  // ALL LDS is one array (a second __shared__ object beside an LDS-DMA target makes hipcc wait
  // vmcnt(0) before every ds_read): [window descriptors: it, it+1, it+2][op constants, 2 slot tables][2 buffers][third tiles]
  extern __shared__ __attribute__((aligned(16))) char smem_all[];
  int(*ring)[GCMI_WIN_META_INTS] = reinterpret_cast<int(*)[GCMI_WIN_META_INTS]>(smem_all);
  float* op_lds = reinterpret_cast<float*>(smem_all + kRingBytes);
  char* smem = smem_all + kHeadBytes;
  constexpr int kEPP = Op::P::kEPP;
  constexpr bool kXT = Op::kThird == Third::dma_pair;  // a third tile per window buffer, DMA-filled with the window
  constexpr bool kScratch = Op::kThird == Third::scratch;  // one third tile, the compute phase's own
  if (op.skip(LPR * kEPP)) return;  // uniform over the grid
  op.template init<WT>(op_lds, LPR * kEPP);
  // the compute phase of one window: ops with a third tile get it, the others the op constants (scratch: both)
  auto compute = [&](const char* buf, const Layout& l, const auto& sl, char* extra) {
    if constexpr (kXT) op.template run<WT, LPR>(buf, l, sl, extra);
    else if constexpr (kScratch) op.template run<WT, LPR>(buf, l, sl, op_lds, extra);
    else op.template run<WT, LPR>(buf, l, sl, op_lds);
  };
  const int t = threadIdx.x;
  if ((int)blockIdx.x >= g_norm) {  // oversized windows: stage, wait, compute
    const int G = gridDim.x - g_norm;
    for (int w = n_norm + (int)blockIdx.x - g_norm; w < n_win; w += G) {
      if (t < GCMI_WIN_META_INTS) ring[0][t] = meta[(size_t)w * GCMI_WIN_META_INTS + t];
      __syncthreads();
      const WinMeta m = read_meta(ring[0]);
      stage<WT, LPR, AUX, kEPP>(smem, Lbig, m, x, ldx, aux, edges);
      wait_dma();
      __syncthreads();
      // (no launcher sends a two-stage op here)
      compute(smem, Lbig, WinSlots<false>{m, Lbig.maxd, m.sb[kND]}, smem + 2 * L.buf_bytes());
      __syncthreads();
    }
    return;
  }
  const int G = g_norm;
  int w = blockIdx.x;  // < n_norm by construction of the grid
  // on alternate launches the ordinary windows are walked from the last one (next_sweep_direction, core.cpp): the
  // rows the previous kernel wrote last are the ones still in the Infinity Cache
  auto widx = [&](int v) { return (size_t)(rev ? n_norm - 1 - v : v); };
  const int bb = L.buf_bytes();
  unsigned* tabs = reinterpret_cast<unsigned*>(smem_all + kRingBytes + kTabAt);  // [buffer][kTabSlots]
  // everything a window needs before its compute phase: the DMA of its rows and entries, and its slot table
  auto prepare = [&](int slot3, int b) {
    const WinMeta m = read_meta(ring[slot3]);
    stage<WT, LPR, AUX, kEPP>(smem + b * bb, L, m, x, ldx, aux, edges);
    if constexpr (kXT) stage_extra<WT, LPR>(smem + 2 * bb + b * L.tile_bytes, L, m, op.extra_src(), op.extra_ld_bytes());
    if (L.tab) fill_slot_table(tabs + b * kTabSlots, m, L.maxd);
  };
  int metareg = 0;
  if (t < GCMI_WIN_META_INTS) {
    ring[0][t] = meta[widx(w) * GCMI_WIN_META_INTS + t];
    if (w + G < n_norm) ring[1][t] = meta[widx(w + G) * GCMI_WIN_META_INTS + t];
    if (w + 2 * G < n_norm) metareg = meta[widx(w + 2 * G) * GCMI_WIN_META_INTS + t];
  }
  __syncthreads();
  prepare(0, 0);
  int it = 0;
  for (;;) {
    wait_dma();
    __syncthreads();  // buffer it&1 and its slot table have landed, the other pair is free
    const bool has_next = w + G < n_norm;
    if (t < GCMI_WIN_META_INTS) {
      ring[(it + 2) % 3][t] = metareg;  // read from the next round on
      if (w + 3 * G < n_norm) metareg = meta[widx(w + 3 * G) * GCMI_WIN_META_INTS + t];
    }
    if (has_next) prepare((it + 1) % 3, (it + 1) & 1);
    const int* desc = ring[it % 3];
    char* extra = smem + 2 * bb + (kXT ? (it & 1) * L.tile_bytes : 0);
    if (L.tab)  // the compute phase reads the atom count of the descriptor and nothing else of it
      compute(smem + (it & 1) * bb, L, WinSlots<true>{tabs + (it & 1) * kTabSlots, desc, desc[2 * kND - 1]}, extra);
    else
      compute(smem + (it & 1) * bb, L, WinSlots<false>{read_meta(desc), L.maxd, desc[2 * kND - 1]}, extra);
    if (!has_next) break;
    w += G;
    ++it;
  }
}

// ------------------------------------------------------------------ host-side dispatch helpers
static bool windows_disabled() {
  static int v = -1;
  if (v < 0) v = getenv("GCMI_NO_WINDOWS") != nullptr ? 1 : 0;
  return v == 1;
}

// (n_feat counts FLOATS per tile row: a bf16 row of n elements is a tile row of n / 2 "floats")
// aux: 0 none, 4 / 8 = aux bytes per 16-byte piece (fp32 / bf16 rows; stage())
static Layout make_layout(int alloc, int ecap, int maxd, int n_feat, int aux) {
  Layout L;
  L.tile_bytes = alloc * n_feat * 4;
  L.aux_bytes = aux == 4 ? (alloc * n_feat + 15) / 16 * 16 : aux == 8 ? (alloc * (n_feat / 4) + 63) / 64 * 512 : 0;
  L.edge_bytes = (ecap > 8 ? ecap : 8) * 2;
  L.maxd = maxd;
  L.tab = 0;
  return L;
}

struct WinPlan {
  Layout L, Lbig;
  size_t shmem;
  bool ok;
};

// LDS shapes: the two buffers of the ordinary windows must also hold one oversized window.
static WinPlan make_plan(const gcmi_graph* g, int n_feat, int aux) {
  int maxd = 0;
  for (int d = 1; d <= g->max_deg; ++d)
    if (g->deg_start[d + 1] > g->deg_start[d]) maxd = d;
  WinPlan p;
  p.Lbig = make_layout(g->win_alloc_big, g->win_ecap_big, maxd, n_feat, aux);
  int alloc = std::max(g->win_alloc, 1);
  p.L = make_layout(alloc, g->win_ecap, maxd, n_feat, aux);
  if (g->n_win_big > 0) {
    while (2 * p.L.buf_bytes() < p.Lbig.buf_bytes()) {
      alloc += 8;
      p.L = make_layout(alloc, g->win_ecap, maxd, n_feat, aux);
    }
  }
  p.L.tab = g->win_alloc <= kTabSlots ? 1 : 0;  // by the largest WINDOW: the buffers may have grown beyond it
  p.shmem = 2 * (size_t)p.L.buf_bytes() + kHeadBytes;
  p.ok = p.shmem <= (size_t)kLdsPerCU;
  return p;
}

// the batch has window plans and a tile row of n_floats floats (+ aux) fits the LDS
static bool plan_fits(const gcmi_graph* g, int n_floats, int aux) {
  if (windows_disabled() || g->d_win_meta == nullptr || g->n_win <= 0) return false;
  if (g->d_win_edges == nullptr || g->n_win_big < 0 || g->n_win_big > g->n_win) return false;
  return make_plan(g, n_floats, aux).ok;
}
// ... and so do the third tiles of a two-stage pass
static bool third_tiles_fit(const gcmi_graph* g, int n_floats, int aux, Third kind) {
  const WinPlan p = make_plan(g, n_floats, aux);
  return p.shmem + (size_t)third_tiles(kind) * p.L.tile_bytes <= (size_t)kLdsPerCU;
}

// which: 0 all windows, 1 ordinary, 2 oversized only
template <int LPR, bool AUX, class Op>
static int launch_lpr(const gcmi_graph* g, const WinPlan& p, const char* x, int64_t ldx, const uint8_t* aux,
                      const Op& op, hipStream_t st, const char* what, int which) {
  constexpr int WT = Op::kThreads;
  auto kern = win_kernel<WT, LPR, AUX, Op>;
  static LdsLimit lim;  // per instantiation
  if (!raise_lds_limit(lim, reinterpret_cast<const void*>(kern), kLdsPerCU)) {
    set_error("%s: cannot raise the dynamic LDS limit", what);
    return GCMI_ERR_LAUNCH;
  }
  const int n_norm = g->n_win - g->n_win_big;
  size_t shmem = p.shmem;
  if constexpr (Op::kThird != Third::none) {
    if (which != 1) {
      set_error("%s: oversized windows are not handled by the two-stage form", what);
      return GCMI_ERR_UNSUPPORTED;
    }
    shmem += (size_t)p.L.tile_bytes * third_tiles(Op::kThird);
    if (shmem > (size_t)kLdsPerCU) return GCMI_ERR_UNSUPPORTED;
  }
  const int by_lds = (int)((size_t)kLdsPerCU / shmem);
  const int by_threads = 2048 / WT;
  const int per_cu = std::max(1, std::min(8, std::min(by_lds, by_threads)));
  const int g_norm = which == 2 ? 0 : std::min(n_norm, 256 * per_cu);
  const int g_big = which == 1 ? 0 : std::min(g->n_win_big, 64);
  if (g_norm + g_big == 0) return GCMI_OK;
  const int rev = next_sweep_direction();
  // The forward two-stage pass stands where two launches stood and takes both their turns (it walks in the first one's
  // direction, from the end its producer finished at): every later kernel keeps the direction, and with it the order
  // of its partial sums, that it has after the two separate launches.  Measured against taking one turn: §34.
  if constexpr (Op::kThird == Third::scratch) (void)next_sweep_direction();
  hipLaunchKernelGGL(kern, dim3(g_norm + g_big), dim3(WT), shmem, st, g->d_win_meta, g->d_win_edges, n_norm,
                     g->n_win, g_norm, p.L, p.Lbig, x, ldx, aux, op, rev);
  GCMI_CHECK_LAUNCH(what);
  return GCMI_OK;
}

// Rows of T, n_feat elements = n_feat / kEPP pieces each (fp32: 64 -> 16, 76 -> 19, 128 -> 32; bf16: 64 -> 8, 80 -> 10,
// 128 -> 16); AUX: the byte matrix `aux` (one byte per element) rides along.  The DMA moves bytes, so the leading
// dimension goes down in bytes and the plan counts a tile row in floats.
template <bool AUX, class T, class Op>
static int launch(const gcmi_graph* g, int n_feat, const T* x, int64_t ldx, const uint8_t* aux, const Op& op,
                  hipStream_t st, const char* what, int which = 0) {
  using P = Piece<T>;
  constexpr bool kH = P::kEPP == 8;
  const WinPlan p = make_plan(g, n_feat * (int)sizeof(T) / 4, AUX ? P::kEPP : 0);
  const char* xb = reinterpret_cast<const char*>(x);
  const int64_t ldb = ldx * (int64_t)sizeof(T);
  switch (n_feat / P::kEPP) {
    case 8: if constexpr (kH) return launch_lpr<8, AUX, Op>(g, p, xb, ldb, aux, op, st, what, which); break;
    case 10: if constexpr (kH) return launch_lpr<10, AUX, Op>(g, p, xb, ldb, aux, op, st, what, which); break;
    case 16: return launch_lpr<16, AUX, Op>(g, p, xb, ldb, aux, op, st, what, which);
    case 19: if constexpr (!kH) return launch_lpr<19, AUX, Op>(g, p, xb, ldb, aux, op, st, what, which); break;
    case 32: if constexpr (!kH) return launch_lpr<32, AUX, Op>(g, p, xb, ldb, aux, op, st, what, which); break;
    default: break;
  }
  set_error(kH ? "%s: no bf16 window kernel for %d features" : "%s: no window kernel for %d features", what, n_feat);
  return GCMI_ERR_UNSUPPORTED;
}

// d_dxs holds the self part of dX on entry; on return d_dy holds the GraphPool backward of the complete dX.  The
// ordinary windows take the two-stage pass (dX in LDS only); the few oversized ones (a molecule above the window cap
// each) take the two separate passes over their own rows, which completes d_dxs there.  GCMI_ERR_UNSUPPORTED: no LDS
// for the third tiles.  what: the names of the three launches
template <class TwoStage, class SumAcc, class Bwd, class T>
static int sumacc_max_bwd(const gcmi_graph* g, const T* d_ds, int64_t ldds, int n_feat, T* d_dxs, int64_t lddxs,
                          const uint8_t* d_arg, T* d_dy, int64_t lddy, hipStream_t st, const char* const (&what)[3]) {
  TwoStage op{{d_dxs, lddxs, d_dy, lddy}};
  int rc = launch<true>(g, n_feat, d_ds, ldds, d_arg, op, st, what[0], 1);
  if (rc || g->n_win_big == 0) return rc;
  SumAcc acc{{d_dxs, lddxs}};
  rc = launch<false>(g, n_feat, d_ds, ldds, nullptr, acc, st, what[1], 2);
  if (rc) return rc;
  Bwd mb{{d_dy, lddy, nullptr, nullptr}};
  return launch<true>(g, n_feat, d_dxs, lddxs, d_arg, mb, st, what[2], 2);
}

// ------------------------------------------------------------------ entry points (common.h)
bool win_has_width(int n_feat) { return n_feat == 64 || n_feat == 76 || n_feat == 128; }

bool win_usable(const gcmi_graph* g, int n_feat, bool aux) {
  if (n_feat % 4 != 0 || n_feat > 256) return false;
  return plan_fits(g, n_feat, aux ? 4 : 0);
}

int win_gather_sum(const gcmi_graph* g, const float* d_x, int64_t ldx, int n_feat, float* d_s,
                   int64_t lds, hipStream_t st, bool accumulate) {
  if (accumulate) {
    SumOp<true> op{{d_s, lds}};
    return launch<false>(g, n_feat, d_x, ldx, nullptr, op, st, "win_gather_sum (accumulate)");
  }
  SumOp<false> op{{d_s, lds}};
  return launch<false>(g, n_feat, d_x, ldx, nullptr, op, st, "win_gather_sum");
}

int win_gather_max(const gcmi_graph* g, const float* d_x, int64_t ldx, int n_feat, const float* d_scale,
                   const float* d_shift, float* d_out, int64_t ldo, uint8_t* d_arg, hipStream_t st) {
  if (d_scale) {
    MaxOp<true> op{{d_scale, d_shift, d_out, ldo, d_arg}};
    return launch<false>(g, n_feat, d_x, ldx, nullptr, op, st, "win_gather_max");
  }
  MaxOp<false> op{{nullptr, nullptr, d_out, ldo, d_arg}};
  return launch<false>(g, n_feat, d_x, ldx, nullptr, op, st, "win_gather_max");
}

int win_gather_max_bwd(const gcmi_graph* g, const float* d_dout, int64_t lddo, int n_feat,
                       const uint8_t* d_arg, float* d_dx, int64_t lddx, hipStream_t st) {
  MaxBwdOp op{{d_dx, lddx, nullptr, nullptr}};
  return launch<true>(g, n_feat, d_dout, lddo, d_arg, op, st, "win_gather_max_bwd");
}

int win_gather_max_bwd_if_ill(const gcmi_graph* g, const float* d_dout, int64_t lddo, int n_feat, const uint8_t* d_arg,
                              float* d_dx, int64_t lddx, const float* d_gamma, const float* d_beta, hipStream_t st) {
  MaxBwdOp op{{d_dx, lddx, d_gamma, d_beta}};
  return launch<true>(g, n_feat, d_dout, lddo, d_arg, op, st, "win_gather_max_bwd (conditional)");
}

bool win_two_stage_usable(const gcmi_graph* g, int n_feat) {
  return win_has_width(n_feat) && win_usable(g, n_feat, true) && third_tiles_fit(g, n_feat, 4, Third::dma_pair);
}

int win_gather_sumacc_max_bwd(const gcmi_graph* g, const float* d_ds, int64_t ldds, int n_feat, float* d_dxs,
                              int64_t lddxs, const uint8_t* d_arg, float* d_dy, int64_t lddy, hipStream_t st) {
  return sumacc_max_bwd<SumAccMaxBwdOp, SumOp<true>, MaxBwdOp>(
      g, d_ds, ldds, n_feat, d_dxs, lddxs, d_arg, d_dy, lddy, st,
      {"win_gather_sumacc_max_bwd", "win_gather_sum (accumulate, oversized windows)",
       "win_gather_max_bwd (oversized windows)"});
}

bool win_max_sum_usable(const gcmi_graph* g, int n_feat) {
  return win_has_width(n_feat) && (n_feat == 64 || n_feat == 128) && win_usable(g, n_feat, false) &&
         third_tiles_fit(g, n_feat, 0, Third::scratch);
}

static std::atomic<int> g_max_sum_launches{0};
int max_sum_launches() { return g_max_sum_launches.load(std::memory_order_relaxed); }

// the two-stage pass over the ordinary windows
template <bool BN>
static int max_sum(const gcmi_graph* g, const float* d_y, int64_t ldy, int n_feat, const MaxBody<float, BN>& pool,
                   float* d_s, int64_t lds, hipStream_t st) {
  // (launch_lpr directly: two widths, a thread count each -- launch<> would instantiate both for every piece count)
  const WinPlan p = make_plan(g, n_feat, 0);
  const char* yb = reinterpret_cast<const char*>(d_y);
  const int64_t ldb = ldy * (int64_t)sizeof(float);
  if (n_feat == 128) {  // one workgroup per CU by LDS: a full one
    MaxSumOp<BN, 1024> op{{pool, d_s, lds}};
    return launch_lpr<32, false>(g, p, yb, ldb, nullptr, op, st, "win_gather_max_sum", 1);
  }
  if (n_feat == 64) {
    MaxSumOp<BN, 512> op{{pool, d_s, lds}};
    return launch_lpr<16, false>(g, p, yb, ldb, nullptr, op, st, "win_gather_max_sum", 1);
  }
  set_error("win_gather_max_sum: no window kernel for %d features", n_feat);
  return GCMI_ERR_UNSUPPORTED;
}

// d_pool = GraphPool of the rows of d_y (+ arg bytes), d_s = the neighbour sums of d_pool.  The ordinary windows take
// the two-stage pass; the few oversized ones the two separate passes over their own rows.
int win_gather_max_sum(const gcmi_graph* g, const float* d_y, int64_t ldy, int n_feat, const float* d_scale,
                       const float* d_shift, float* d_pool, int64_t ldp, uint8_t* d_arg, float* d_s, int64_t lds,
                       hipStream_t st) {
  int rc = d_scale ? max_sum<true>(g, d_y, ldy, n_feat, {d_scale, d_shift, d_pool, ldp, d_arg}, d_s, lds, st)
                   : max_sum<false>(g, d_y, ldy, n_feat, {nullptr, nullptr, d_pool, ldp, d_arg}, d_s, lds, st);
  if (rc) return rc;
  if (g->n_win > g->n_win_big) g_max_sum_launches.fetch_add(1, std::memory_order_relaxed);
  if (g->n_win_big == 0) return rc;
  if (d_scale) {
    MaxOp<true> mx{{d_scale, d_shift, d_pool, ldp, d_arg}};
    rc = launch<false>(g, n_feat, d_y, ldy, nullptr, mx, st, "win_gather_max (oversized windows)", 2);
  } else {
    MaxOp<false> mx{{nullptr, nullptr, d_pool, ldp, d_arg}};
    rc = launch<false>(g, n_feat, d_y, ldy, nullptr, mx, st, "win_gather_max (oversized windows)", 2);
  }
  if (rc) return rc;
  SumOp<false> sm{{d_s, lds}};
  return launch<false>(g, n_feat, d_pool, ldp, nullptr, sm, st, "win_gather_sum (oversized windows)", 2);
}

// ---- bf16 activation storage (storage >= 1)
bool win_usable_h(const gcmi_graph* g, int n_feat) {
  if (n_feat != 64 && n_feat != 80 && n_feat != 128) return false;
  return plan_fits(g, n_feat / 2, 0);
}

// fp32 rows of n_feat (76) columns -> bf16 neighbour sums and a bf16 copy of the rows, both `ldo` (80) wide
int win_gather_sum_fh(const gcmi_graph* g, const float* d_x, int64_t ldx, int n_feat, bf16_t* d_s, bf16_t* d_xcopy,
                      int64_t ldo, hipStream_t st) {
  if (n_feat % 4 != 0 || ldo < n_feat || (ldo - n_feat) % 4 != 0 || ldo % 8 != 0 || !aligned16(d_s) || !aligned16(d_xcopy)) {
    set_error("win_gather_sum (fp32 -> bf16): bad shape (n_feat %d, ldo %lld)", n_feat, (long long)ldo);
    return GCMI_ERR_UNSUPPORTED;
  }
  SumOpFH op{d_s, d_xcopy, ldo, (int)((ldo - n_feat) / 4)};
  return launch<false>(g, n_feat, d_x, ldx, nullptr, op, st, "win_gather_sum (fp32 -> bf16)");
}

int win_gather_sum_h(const gcmi_graph* g, const bf16_t* d_x, int64_t ldx, int n_feat, bf16_t* d_s, int64_t lds,
                     hipStream_t st, bool accumulate) {
  if (accumulate) {  // SumAccOpH over all windows (the two-stage backward runs it over the oversized ones only)
    SumAccOpH op{{d_s, lds}};
    return launch<false>(g, n_feat, d_x, ldx, nullptr, op, st, "win_gather_sum (bf16, accumulate)");
  }
  SumOpH op{{d_s, lds}};
  return launch<false>(g, n_feat, d_x, ldx, nullptr, op, st, "win_gather_sum (bf16)");
}

int win_gather_max_h(const gcmi_graph* g, const bf16_t* d_x, int64_t ldx, int n_feat, const float* d_scale,
                     const float* d_shift, bf16_t* d_out, int64_t ldo, uint8_t* d_arg, hipStream_t st) {
  if (d_scale) {
    MaxOpH<true> op{{d_scale, d_shift, d_out, ldo, d_arg}};
    return launch<false>(g, n_feat, d_x, ldx, nullptr, op, st, "win_gather_max (bf16)");
  }
  MaxOpH<false> op{{nullptr, nullptr, d_out, ldo, d_arg}};
  return launch<false>(g, n_feat, d_x, ldx, nullptr, op, st, "win_gather_max (bf16)");
}

// ---- gradient streams in bf16 (storage == 2): dpool, dy, dS and dXs travel between kernels as bf16 rows
bool win_usable_gh(const gcmi_graph* g, int n_feat) { return n_feat == 64 && plan_fits(g, n_feat / 2, 8); }

int win_gather_max_bwd_h(const gcmi_graph* g, const bf16_t* d_dout, int64_t lddo, int n_feat, const uint8_t* d_arg,
                         bf16_t* d_dx, int64_t lddx, const float* only_if_gamma, const float* only_if_beta, hipStream_t st) {
  MaxBwdOpH op{{d_dx, lddx, only_if_gamma, only_if_beta}};
  return launch<true>(g, n_feat, d_dout, lddo, d_arg, op, st, "win_gather_max_bwd (bf16)");
}

bool win_two_stage_usable_h(const gcmi_graph* g, int n_feat) {
  return win_usable_gh(g, n_feat) && third_tiles_fit(g, n_feat / 2, 8, Third::dma_pair);
}

// The same two questions for every width launch<> has a bf16 kernel with arg bytes for (the model step keeps its bf16
// gradient streams at 64 columns: win_usable_gh): the operation-level entry points of gather.hip
bool win_usable_bwd_h(const gcmi_graph* g, int n_feat) {
  if (n_feat != 64 && n_feat != 80 && n_feat != 128) return false;
  return plan_fits(g, n_feat / 2, 8);
}
bool win_two_stage_usable_bwd_h(const gcmi_graph* g, int n_feat) {
  return win_usable_bwd_h(g, n_feat) && third_tiles_fit(g, n_feat / 2, 8, Third::dma_pair);
}

int win_gather_sumacc_max_bwd_h(const gcmi_graph* g, const bf16_t* d_ds, int64_t ldds, int n_feat, bf16_t* d_dxs,
                                int64_t lddxs, const uint8_t* d_arg, bf16_t* d_dy, int64_t lddy, hipStream_t st) {
  return sumacc_max_bwd<SumAccMaxBwdOpH, SumAccOpH, MaxBwdOpH>(
      g, d_ds, ldds, n_feat, d_dxs, lddxs, d_arg, d_dy, lddy, st,
      {"win_gather_sumacc_max_bwd (bf16)", "win_gather_sum (bf16, accumulate, oversized windows)",
       "win_gather_max_bwd (bf16, oversized windows)"});
}

}  // namespace gcmi
