// Batch collation from a resident graph set: what dmpnn_collate.hip and megnet_collate.hip share.
//
// A set holds the flat arrays of M items (molecules, graphs) with two int64 offset arrays of M + 1 entries each (atoms
// and bonds, nodes and edges: "a" and "b" below).  The plan of a batch of n items, int32 words made by the host in O(n):
// [idx (n) ; off_a (n + 1) ; off_b (n + 1)], the offsets being the exclusive prefix sums of the selected items' counts
// with the totals last.  The buffer is a row of blocks of 4-byte words, every block at a 16-byte boundary, the pad words
// behind a block zero.
//
// One workgroup of kCollateThreads threads per selected item (collate_item): item m of the batch owns its entries of
// the per-item blocks and the rows [off_a[m], off_a[m + 1]) and [off_b[m], off_b[m + 1]); the LAST workgroup also writes
// what no item owns (collate_tail): the closing entries of the offset lists and the pad words.  So every word of the
// buffer is written exactly once, without atomics, without a dependence between workgroups and without LDS.  Whatever
// is contiguous in the set AND in the batch is one flat copy, thread t taking word t, t + 256, ...: consecutive lanes,
// consecutive dwords on both sides (rows of 5, 33 or 133 floats are only 4-byte aligned, so dwords, not 16-byte
// pieces; never one lane per row).
//
// A file states its args (a struct derived from CollateBatch), collate_item and collate_tail; collate_set_kernel and
// collate_set_host run them, the host with one "thread", so that the layout is testable without a GPU.
#pragma once
#include "common.h"

namespace gcmi {

constexpr int kCollateThreads = 256;

// The batch side of the args: the plan, the totals and where the N blocks lie
template <int N>
struct CollateBatch {
  const int32_t* plan;
  int32_t n, n_a, n_b;  // items, and the totals the plan ends with
  int32_t* out;
  int64_t at[N];    // word offset of every block, -1: the mode lacks it
  int64_t size[N];  // its words before padding
  int64_t end;
};

// at[0..n_blocks): where each block starts (-1 where `lacks` says so) and sizes: its words before padding (0 likewise);
// lacks, at and sizes may be NULL.  Returns the words of the buffer
inline int64_t place_blocks(int n_blocks, const int64_t* size, const bool* lacks, int64_t* at, int64_t* sizes) {
  int64_t end = 0;
  for (int k = 0; k < n_blocks; ++k) {
    const bool absent = lacks && lacks[k];
    if (at) at[k] = absent ? -1 : end;
    if (sizes) sizes[k] = absent ? 0 : size[k];
    if (!absent) end += up4(size[k]);
  }
  return end;
}

// The (at most three) zero words behind every block.  4 slots per block: slot q of block b is the q-th word behind the
// block's data, if the block has that many pad words
template <int N>
__host__ __device__ inline void write_pads(const CollateBatch<N>& p, int tid, int n_threads) {
  for (int t = tid; t < 4 * N; t += n_threads) {
    const int b = t / 4, q = t % 4;
    if (p.at[b] >= 0 && q < (4 - p.size[b] % 4) % 4) p.out[p.at[b] + p.size[b] + q] = 0;
  }
}

// Entry m of a plan: the item idx of the set, its rows [ap, ap + na) and [bp, bp + nb) there and where they go in the
// batch, a0 and b0.  fits: the item is one of the set's M and its rows lie inside the totals; an entry that does not fit
// is skipped without reading through it (the Python side refuses such a batch before any launch)
struct PlanEntry {
  int64_t idx;
  int a0, b0;
  int64_t ap, bp, na, nb;
  bool fits;
};

__host__ __device__ inline PlanEntry plan_entry(const int32_t* plan, int n, int m, const int64_t* ptr_a,
                                                const int64_t* ptr_b, int64_t M, int64_t total_a, int64_t total_b) {
  PlanEntry e;
  e.idx = plan[m];
  e.a0 = plan[n + m];
  e.b0 = plan[2 * n + 1 + m];
  const bool known = e.idx >= 0 && e.idx < M;
  e.ap = known ? ptr_a[e.idx] : 0, e.bp = known ? ptr_b[e.idx] : 0;
  e.na = known ? ptr_a[e.idx + 1] - e.ap : 0, e.nb = known ? ptr_b[e.idx + 1] - e.bp : 0;
  e.fits = known && e.ap >= 0 && e.bp >= 0 && e.na >= 0 && e.nb >= 0 && e.a0 >= 0 && e.b0 >= 0 &&
           e.a0 + e.na <= total_a && e.b0 + e.nb <= total_b;
  return e;
}

// dst[w] = src[w] + add over `words` words, thread tid of n_threads taking every n_threads-th
__host__ __device__ inline void copy_add(int32_t* dst, const int32_t* src, int64_t words, int32_t add, int tid,
                                         int n_threads) {
  for (int64_t w = tid; w < words; w += n_threads) dst[w] = src[w] + add;
}

__host__ __device__ inline void copy_rows(float* dst, const float* src, int64_t words, int tid, int n_threads) {
  for (int64_t w = tid; w < words; w += n_threads) dst[w] = src[w];
}

__host__ __device__ inline void fill_words(int32_t* dst, int64_t words, int32_t value, int tid, int n_threads) {
  for (int64_t w = tid; w < words; w += n_threads) dst[w] = value;
}

// collate_item and collate_tail are the including file's, found through the args type
template <class Args>
__global__ __launch_bounds__(kCollateThreads) void collate_set_kernel(const Args p) {
  const int m = blockIdx.x, tid = threadIdx.x;
  if (m == (int)gridDim.x - 1) collate_tail(p, tid, kCollateThreads);
  if (m < p.n) collate_item(p, m, tid, kCollateThreads);
}

template <class Args>
int collate_set_launch(const Args& p, int workgroups, void* stream, const char* what) {
  hipLaunchKernelGGL(collate_set_kernel<Args>, dim3(workgroups), dim3(kCollateThreads), 0,
                     static_cast<hipStream_t>(stream), p);
  GCMI_CHECK_LAUNCH(what);
  return GCMI_OK;
}

template <class Args>
int collate_set_host(const Args& p) {
  collate_tail(p, 0, 1);
  for (int m = 0; m < p.n; ++m) collate_item(p, m, 0, 1);
  return GCMI_OK;
}

}  // namespace gcmi
