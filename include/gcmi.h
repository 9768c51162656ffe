/*
 * gcmi.h -- C ABI of libgcmi.so: the MI355X (gfx950) graph-convolution hot path.
 *
 * The reference (DeepChem, pure Python) has no FFI for this path; its boundary
 * is a Python class contract.  These entry points are what the
 * reference's layers would bind if they had one -- one per reference function
 * on the hot path -- and what deepchem_amd's host-side mirror calls through
 * ctypes.  Reference citations are relative to /root/reference/deepchem/.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch / STL types.
 *   - every pointer named d_* is DEVICE memory, borrowed for the call; all
 *     other pointers are host memory.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  All
 *     work is enqueued on it; nothing synchronises, allocates or frees, so
 *     every entry point can be captured into a hipGraph.
 *   - return 0 on success, a negative gcmi_status otherwise; the message of
 *     the last failure on the calling thread: gcmi_last_error().
 *   - feature matrices are row-major float32 with an explicit leading
 *     dimension (ld, in floats).  When ld % 4 == 0 and the base is 16-byte
 *     aligned the kernels move 16 B per lane; otherwise 4 B per lane.
 *   - thread-compatible: no global mutable state except the per-thread error
 *     string.
 */
#ifndef GCMI_H
#define GCMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GCMI_VERSION 100 /* 0.1.0 */
#define GCMI_MAX_DEG 10  /* degrees 0..10: ConvMol default, feat/mol_graphs.py:48 */

typedef enum gcmi_status {
  GCMI_OK = 0,
  GCMI_ERR_ARG = -1,    /* bad argument (null pointer, negative size, shape mismatch) */
  GCMI_ERR_LAUNCH = -2, /* HIP launch / runtime error */
  GCMI_ERR_UNSUPPORTED = -3
} gcmi_status;

/*
 * One collated batch of molecules in the layout ConvMol.agglomerate_mols
 * produces (feat/mol_graphs.py:256-349): atoms sorted by (degree, molecule),
 * so the atoms of degree d are the contiguous rows
 * [deg_start[d], deg_start[d+1]) and each of them has exactly d neighbours.
 * The per-degree (n_d, d) int32 tables deg_adj_lists[1..max_deg] are stored
 * back to back in ONE array d_col_idx; the table of degree d starts at
 * edge_start[d].  That is a CSR whose row pointer is implicit:
 *   row_ptr(i) = edge_start[d] + (i - deg_start[d]) * d.
 */
#define GCMI_WIN_META_INTS 24
#define GCMI_WIN_SLOT_BITS 12
#define GCMI_WIN_MAX_SLOTS 4095

typedef struct gcmi_graph {
  int32_t n_atoms;                      /* N                                        */
  int32_t n_edges;                      /* E = sum_d d * n_d  (directed)            */
  int32_t n_mols;                       /* B: rows GraphGather emits (batch_size)   */
  int32_t max_deg;                      /* <= GCMI_MAX_DEG                          */
  int32_t deg_start[GCMI_MAX_DEG + 2];  /* [max_deg+1] = N                          */
  int32_t edge_start[GCMI_MAX_DEG + 2]; /* [max_deg+1] = E                          */
  const int32_t* d_col_idx;             /* E neighbour rows                         */
  const int32_t* d_membership;          /* N: molecule of every atom, ascending
                                           inside every degree block               */
  const int32_t* d_mol_runs;            /* n_mols*(max_deg+1)*2: per molecule and
                                           degree the row range [begin,end) of its
                                           atoms; built by gcmi_build_mol_runs     */
  const uint8_t* d_rev_pos;             /* E (may be NULL): for the edge slot (k, j)
                                           with i = col_idx[row_ptr(k)+j], the slot of
                                           k in i's own neighbour list; exists when
                                           every bond is listed from both ends; built
                                           by gcmi_build_rev_pos or gcmi_collate    */
  /* Molecule windows (optional; produced by gcmi_collate_plans): consecutive molecules grouped
   * so that a window holds <= win_cap atoms (a larger molecule gets a window of its own; those
   * oversized windows come last in d_win_meta).
   * Because every degree block is sorted by molecule, the atoms of a window are <= max_deg+1
   * CONTIGUOUS row ranges, one per degree block.  A workgroup streams those ranges into LDS
   * once ("slots", numbered degree block by degree block) and serves every neighbour read of
   * the window from LDS: all neighbours of an atom belong to its own molecule, hence to its
   * window.
   *   d_win_meta[w][GCMI_WIN_META_INTS]:
   *     [0..10]  row_of_slot_base[d] = first row of the window in degree block d - slot_start[d]
   *              (global row of slot s of degree d = base[d] + s)
   *     [11..21] slot_start[1..11]  (slot_start[0] = 0, slot_start[11] = atoms in the window)
   *     [22]     first entry of the window in d_win_edges (a multiple of 8)
   *     [23]     edge entries of the window (unpadded)
   *   d_win_edges: the neighbour lists window by window, inside a window in (degree, row, j)
   *     order, every window padded to a multiple of 8 entries; entry = LDS slot of the
   *     neighbour | rev_pos << 12 (rev_pos = 15: no partner).                                */
  int32_t n_win;                        /* all windows: ordinary ones first, then     */
  int32_t n_win_big;                    /* the oversized ones (one molecule > win_cap) */
  int32_t win_alloc;                    /* atoms of the largest ordinary window       */
  int32_t win_ecap;                     /* its padded edge entries (largest)          */
  int32_t win_alloc_big;                /* the same for the oversized windows         */
  int32_t win_ecap_big;
  int32_t win_reserved[2];              /* [0]: molecules with at least one atom among the collated ones (filled by
                                           gcmi_collate / gcmi_collate_plans with the windows; 0 = unknown): when it
                                           equals n_mols every molecule lies in some window; [1]: 0 */
  const int32_t* d_win_meta;            /* n_win * GCMI_WIN_META_INTS                */
  const uint16_t* d_win_edges;          /* <= E + 8 * n_win                          */
} gcmi_graph;

int gcmi_version(void);
/* Process-wide options.  GCMI_OPT_GEMM_EXACT: 1 = all matrix products on the exact-fp32 MFMA (the
 * reference's summation order: training trajectories track the reference to ~1e-5); 0 (default) =
 * the split-bf16 kernels (fp32-accurate per product, ~1.25x faster, own rounding).  Also settable
 * by the environment variable GCMI_GEMM_EXACT=1 before the library is loaded.                   */
enum {
  GCMI_OPT_GEMM_EXACT = 1,
  /* 1 (default): the training forward of the whole-model entry points takes the BatchNorm column sums from the
   * epilogue of the producing product; 0: separate column-sum launches (same statistics up to summation order) */
  GCMI_OPT_FUSED_BN_STATS = 2,
  /* 1 (default): the whole-model backward forms the gradient of a block's pre-activation in LDS and computes the
   * weight gradients and the input gradients from it in one pass over the rows (bwd_fused.hip; split-bf16 mode,
   * default widths); 0: separate BatchNorm-backward, weight-gradient and input-gradient launches (same arithmetic
   * up to summation order).  Environment: GCMI_FUSED_BWD=0 before the library is loaded.                        */
  GCMI_OPT_FUSED_BWD = 3,
  /* read-only (gcmi_get_option): launches of the one-pass backward kernel in this process so far */
  GCMI_OPT_FUSED_BWD_LAUNCHES = 4,
  /* 1 (default): gcmi_readout_fwd and the whole-model forward walk a molecule's rows as one sequence of four-row
   * rounds with two rounds in flight and the run bounds held in registers (readout.hip); 0: run by run, one round
   * at a time.  Same rows in the same order: the results are bit-identical.  Environment: GCMI_READOUT_PRE=0
   * before the library is loaded.                                                                              */
  GCMI_OPT_READOUT_PIPELINED = 5,
  /* read-only (gcmi_get_option): launches so far of the first GraphConv block's one-piece kernels (forward product and
   * backward each count one), taken when gcmi_model_io.features_small_int holds                                  */
  GCMI_OPT_ONE_PIECE_LAUNCHES = 6,
  /* read-only (gcmi_get_option): launches so far of the window pass that forms a GraphPool and the neighbour sums of
   * its output together (gcmi_gather_max_sum_fwd, and the model forward between two GraphConv blocks)              */
  GCMI_OPT_MAX_SUM_LAUNCHES = 7
};
int gcmi_set_option(int32_t option, int32_t value);
int gcmi_get_option(int32_t option, int32_t* value);
const char* gcmi_last_error(void);

/* ---------------------------------------------------------------- host side
 * gcmi_collate: ConvMol.agglomerate_mols (feat/mol_graphs.py:256-349) over a
 * packed molecule set, plus the flattening the kernels want.  Host only.
 *   in : atom_features [A x n_feat] (molecule-major), atom_ptr [n_set+1],
 *        adj_ptr [A+1], adj_idx [nnz] (molecule-local ids), sel [n_sel]
 *        molecules to collate, in order (repeats allowed = pad_batch tiling,
 *        data/datasets.py:204-216).
 *   out: out_features [N x out_ld] (rows in batch order, columns >= n_feat
 *        zero), out_membership [N], out_col_idx [E], out_mol_runs
 *        [n_sel*(max_deg+1)*2], *graph (counts and offsets filled, device
 *        pointers left NULL).  Capacities are checked.
 */
int gcmi_collate_sizes(const int64_t* atom_ptr, const int64_t* adj_ptr, const int64_t* sel,
                       int64_t n_sel, int64_t* out_n_atoms, int64_t* out_n_edges);
int gcmi_collate(const float* atom_features, int64_t n_feat, const int64_t* atom_ptr,
                 const int64_t* adj_ptr, const int32_t* adj_idx, const int64_t* sel,
                 int64_t n_sel, int32_t max_deg, float* out_features, int64_t out_ld,
                 int64_t cap_atoms, int32_t* out_membership, int32_t* out_col_idx,
                 int64_t cap_edges, int32_t* out_mol_runs, gcmi_graph* graph);
/* The same plus the plans of the LDS-window kernels and of the gather-form backwards, all
 * optional (NULL = skip):
 *   out_rev_pos   [E]  uint8; *out_symmetric = 0 when some bond is not listed from both ends
 *                      (the table is then unusable);
 *   win_cap > 0:   out_win_meta [<= n_sel*GCMI_WIN_META_INTS], out_win_edges
 *                  [<= E + 8*n_sel] uint16; graph->n_win, n_win_big, win_alloc*, win_ecap* are filled
 *                  (n_win = 0 when a molecule exceeds GCMI_WIN_MAX_SLOTS atoms).               */
int gcmi_collate_plans(const float* atom_features, int64_t n_feat, const int64_t* atom_ptr,
                       const int64_t* adj_ptr, const int32_t* adj_idx, const int64_t* sel,
                       int64_t n_sel, int32_t max_deg, float* out_features, int64_t out_ld,
                       int64_t cap_atoms, int32_t* out_membership, int32_t* out_col_idx,
                       int64_t cap_edges, int32_t* out_mol_runs, uint8_t* out_rev_pos,
                       int32_t* out_symmetric, int32_t win_cap, int32_t* out_win_meta,
                       uint16_t* out_win_edges, gcmi_graph* graph);
/* The same, and *out_small_int = 1 when every feature element of the batch is an integer with
 * |x| <= 256 / max(1, max_deg) (gcmi_model_io.features_small_int; tested while a row is copied, no second pass), else 0.
 * atom_codes != 0: the rows are 8-byte atom codes (n_feat = 2 "floats"; gcmi_expand_atom_codes) and the test is made on
 * what they expand to: one-hot columns are 0 / 1, so it is the three value bytes -- formal charge (int8), radical
 * electrons, aromatic flag -- that must be within the limit.                                                        */
int gcmi_collate_plans_p(const float* atom_features, int64_t n_feat, const int64_t* atom_ptr,
                         const int64_t* adj_ptr, const int32_t* adj_idx, const int64_t* sel,
                         int64_t n_sel, int32_t max_deg, float* out_features, int64_t out_ld,
                         int64_t cap_atoms, int32_t* out_membership, int32_t* out_col_idx,
                         int64_t cap_edges, int32_t* out_mol_runs, uint8_t* out_rev_pos,
                         int32_t* out_symmetric, int32_t win_cap, int32_t* out_win_meta,
                         uint16_t* out_win_edges, gcmi_graph* graph, int32_t atom_codes, int32_t* out_small_int);

/* ---------------------------------------------------------------- collation on the device
 * The same batches (ConvMol.agglomerate_mols, feat/mol_graphs.py:256-349; the arena gcmi_collate_plans
 * writes, byte for byte) built by the GPU from a molecule set that stays in HBM, so that an epoch of
 * shuffled batches (DiskDataset.iterbatches, data/datasets.py:1518-1623) moves a few MB of row bases per
 * batch over PCIe instead of the whole batch.
 *
 * gcmi_molset_tables (host, once per set): out_mol_hist [n_mols x 11] atoms per degree, out_rank [A] an
 *   atom's rank among the atoms of its degree in its molecule, out_rev [nnz] the reverse slot of every
 *   neighbour entry (15 = none; *out_symmetric = 0 then).  Fails on a degree above max_deg or a
 *   neighbour id outside its molecule, like gcmi_collate_plans.
 * gcmi_collate_plan (host, per batch): the serial part -- row bases of every molecule in every degree
 *   block, windows -- into `staging` (int32 words, >= gcmi_collate_plan_words(n_sel); only the first
 *   out_offsets[6] words are used and need copying).  out_offsets[8]: word offsets of
 *   base, mol_win, atom_off, atom0 (int64), win_meta (what graph->d_win_meta must point at on the
 *   device), window descriptors; [6] words used; [7] uint16 entries of the window edge array.
 *   *graph is filled as by gcmi_collate_plans.
 * gcmi_collate_rows (device, per batch): one thread per atom writes features (n_feat floats per atom of
 *   the resident set; 2 for 8-byte atom codes), membership, col_idx, rev_pos (NULL = skip), window
 *   entries; a second launch writes mol_runs (NULL = skip).  d_staging is the device copy of the plan.
 *   d_src_atom (NULL, or n_atoms int64 of scratch): with it the per-atom threads only note their source
 *   atom and a further launch copies the feature rows with consecutive lanes on consecutive columns
 *   (wide float rows); without it every thread copies its own row (8-byte atom codes).
 * gcmi_collate_rows_host: the same routine run by host loops over host buffers, for tests without a GPU. */
#define GCMI_COLLATE_WIN_DESC_INTS 36
int gcmi_molset_tables(const int64_t* atom_ptr, const int64_t* adj_ptr, const int32_t* adj_idx, int64_t n_mols,
                       int32_t max_deg, int32_t* out_mol_hist, int32_t* out_rank, uint8_t* out_rev,
                       int32_t* out_symmetric, int32_t n_threads);
int64_t gcmi_collate_plan_words(int64_t n_sel);
int gcmi_collate_plan(const int32_t* mol_hist, const int64_t* atom_ptr, const int64_t* sel, int64_t n_sel,
                      int32_t max_deg, int32_t win_cap, int32_t* staging, int64_t staging_words,
                      int64_t* out_offsets, gcmi_graph* graph);
int gcmi_collate_rows(const void* d_features, int64_t n_feat, const int64_t* d_adj_ptr, const int32_t* d_adj_idx,
                      const int32_t* d_rank, const uint8_t* d_rev, const int32_t* d_staging,
                      const int64_t* offsets, const gcmi_graph* plan, float* d_out_features, int64_t out_ld,
                      int32_t* d_membership, int32_t* d_col_idx, int32_t* d_mol_runs, uint8_t* d_rev_pos,
                      uint16_t* d_win_edges, int64_t* d_src_atom, void* stream);
int gcmi_collate_rows_host(const void* features, int64_t n_feat, const int64_t* adj_ptr, const int32_t* adj_idx,
                           const int32_t* rank, const uint8_t* rev, const int32_t* staging, const int64_t* offsets,
                           const gcmi_graph* plan, float* out_features, int64_t out_ld, int32_t* membership,
                           int32_t* col_idx, int32_t* mol_runs, uint8_t* rev_pos, uint16_t* win_edges);

/* ---------------------------------------------------------------- graph plan
 * d_mol_runs from d_membership (device).  d_flag (1 int, device) is set to 1
 * when membership is NOT ascending inside a degree block or out of range.   */
int gcmi_build_mol_runs(const gcmi_graph* g, int32_t* d_mol_runs, int32_t* d_flag, void* stream);
/* d_rev_pos from d_col_idx (device).  d_flag is set to 1 when some edge has no
 * partner (the adjacency is not symmetric): the table is then unusable and the
 * scatter (atomic) backward kernels must be used.                              */
int gcmi_build_rev_pos(const gcmi_graph* g, uint8_t* d_rev_pos, int32_t* d_flag, void* stream);

/* ---------------------------------------------------------------- K1 gather-sum
 * GraphConv.sum_neigh (models/torch_models/layers.py:6236-6246):
 *   s[i,:] = sum_{j<deg(i)} x[col_idx[row_ptr(i)+j], :]   (degree-0 rows: 0)
 * Backward of the gather (dx[k,:] += ds[i,:] for every edge i->k) as
 * gcmi_scatter_add (float atomics; any adjacency).  For a symmetric adjacency
 * (every bond listed from both ends: ConvMol) the same result is
 * gcmi_gather_sum_fwd applied to ds -- deterministic, no atomics.             */
int gcmi_gather_sum_fwd(const gcmi_graph* g, const float* d_x, int64_t ldx, int32_t n_feat,
                        float* d_s, int64_t lds, int32_t accumulate /* s += instead of s = */,
                        void* stream);
int gcmi_scatter_add(const gcmi_graph* g, const float* d_ds, int64_t ldds, int32_t n_feat,
                     float* d_dx, int64_t lddx, void* stream);

/* ---------------------------------------------------------------- K3 gather-max
 * GraphPool.forward (layers.py:6319-6367): out[i,:] = max over {x[i], x[nbrs]}
 * with candidates ordered self, nbr_0, nbr_1, ... and the FIRST maximum winning
 * (torch.max(dim) tie rule).  d_arg[i,f] (uint8, ld = n_feat) records the
 * winner: 0 = self, j+1 = neighbour j.  If d_scale/d_shift are non-NULL the
 * candidates are x*scale[f]+shift[f] (the preceding BatchNorm1d folded in).
 * Backward: dx[winner row, f] += dout[i,f].  With g->d_rev_pos the transposed
 * (gather) form runs -- every dx row is written once, no atomics, deterministic;
 * without it float atomics into a dx the caller pre-zeroed.                    */
int gcmi_gather_max_fwd(const gcmi_graph* g, const float* d_x, int64_t ldx, int32_t n_feat,
                        const float* d_scale, const float* d_shift, float* d_out, int64_t ldo,
                        uint8_t* d_arg, void* stream);
int gcmi_gather_max_bwd(const gcmi_graph* g, const float* d_dout, int64_t lddo, int32_t n_feat,
                        const uint8_t* d_arg, float* d_dx, int64_t lddx, void* stream);
/* GraphPool followed by GraphConv.sum_neigh of its output (the forward between two GraphConv blocks):
 *   d_pool, d_arg = gcmi_gather_max_fwd(d_y, scale, shift);   d_s = gcmi_gather_sum_fwd(d_pool)
 * bit for bit.  Where the batch has molecule windows and n_feat is 64 or 128 (16-byte addressable rows) both are
 * formed in one pass over d_y, the pooled rows of a window held in LDS between the two; otherwise the two calls
 * above run one after the other.  d_arg may be NULL (evaluation).                                              */
int gcmi_gather_max_sum_fwd(const gcmi_graph* g, const float* d_y, int64_t ldy, int32_t n_feat,
                            const float* d_scale, const float* d_shift, float* d_pool, int64_t ldp,
                            uint8_t* d_arg, float* d_s, int64_t lds, void* stream);

/* ---------------------------------------------------------------- the molecule-window passes, one operation each
 * The operations the whole-model entry points run over the molecule windows of a batch (gcmi_collate_plans), callable
 * alone: for tests and for a caller that keeps bf16 activations itself.  bf16 rows are raw 16-bit patterns (uint16_t),
 * leading dimensions count elements.  Every row pointer must be 16-byte aligned with a leading dimension of whole
 * 16-byte pieces (ld % 4 == 0 for float rows, ld % 8 == 0 for bf16 rows), arg rows are n_feat bytes at a 4-byte
 * aligned pointer, and the backward forms need g->d_rev_pos (or n_edges == 0): else GCMI_ERR_ARG.  NO other kernel
 * stands behind these: a batch without window plan, a width without window kernel (float rows: 64, 76, 128; bf16
 * rows: 64, 80, 128) or windows too large for the LDS give GCMI_ERR_UNSUPPORTED with an error text and no launch.
 * Sums and comparisons are formed in fp32 in neighbour order; a bf16 result is rounded once (to nearest even) where it
 * is stored.
 *   gcmi_win_sum_h            s = (accumulate: s +) sum of the neighbours' rows; bf16 in, bf16 out
 *   gcmi_win_sum_fh           float rows in; d_s = their neighbour sums and d_xcopy = the rows themselves, both bf16
 *                             with ldo columns per row (ldo % 8 == 0, (ldo - n_feat) % 4 == 0), columns >= n_feat zero
 *   gcmi_win_max_h            gcmi_gather_max_fwd over bf16 rows (scale/shift float, optional; d_arg optional)
 *   gcmi_win_max_bwd_h        the gather form of gcmi_gather_max_bwd over bf16 rows.  With d_gamma/d_beta (both or
 *                             neither) nothing is written unless some column has |beta| > 64 |gamma|
 *   gcmi_win_max_bwd_if_ill   the same over float rows, d_gamma/d_beta required
 *   gcmi_win_sumacc_max_bwd   the backward between two GraphConv blocks: with dX = d_dxs + neighbour sums of d_ds,
 *     (_h: bf16 rows)         d_dy = GraphPool backward of dX by d_arg.  dX of an ordinary window exists in LDS only
 *                             (bf16: rounded once there): d_dxs is left as it was on the rows of ordinary windows and
 *                             holds the complete dX on the rows of oversized windows, which take the two separate
 *                             passes.                                                                              */
int gcmi_win_sum_h(const gcmi_graph* g, const uint16_t* d_x, int64_t ldx, int32_t n_feat, uint16_t* d_s, int64_t lds,
                   int32_t accumulate, void* stream);
int gcmi_win_sum_fh(const gcmi_graph* g, const float* d_x, int64_t ldx, int32_t n_feat, uint16_t* d_s,
                    uint16_t* d_xcopy, int64_t ldo, void* stream);
int gcmi_win_max_h(const gcmi_graph* g, const uint16_t* d_x, int64_t ldx, int32_t n_feat, const float* d_scale,
                   const float* d_shift, uint16_t* d_out, int64_t ldo, uint8_t* d_arg, void* stream);
int gcmi_win_max_bwd_h(const gcmi_graph* g, const uint16_t* d_dout, int64_t lddo, int32_t n_feat, const uint8_t* d_arg,
                       uint16_t* d_dx, int64_t lddx, const float* d_gamma, const float* d_beta, void* stream);
int gcmi_win_max_bwd_if_ill(const gcmi_graph* g, const float* d_dout, int64_t lddo, int32_t n_feat,
                            const uint8_t* d_arg, float* d_dx, int64_t lddx, const float* d_gamma,
                            const float* d_beta, void* stream);
int gcmi_win_sumacc_max_bwd(const gcmi_graph* g, const float* d_ds, int64_t ldds, int32_t n_feat, float* d_dxs,
                            int64_t lddxs, const uint8_t* d_arg, float* d_dy, int64_t lddy, void* stream);
int gcmi_win_sumacc_max_bwd_h(const gcmi_graph* g, const uint16_t* d_ds, int64_t ldds, int32_t n_feat, uint16_t* d_dxs,
                              int64_t lddxs, const uint8_t* d_arg, uint16_t* d_dy, int64_t lddy, void* stream);

/* ---------------------------------------------------------------- K4 readout
 * GraphGather.forward (layers.py:6450-6479) = unsorted_segment_sum
 * (utils/pytorch_utils.py:20-74) ++ unsorted_segment_max (:473-528) (+tanh):
 *   out[b, 0:F]  = act(sum_{i in mol b} x[i,:]),  out[b, F:2F] = act(max ...)
 * n_mols rows always; an empty molecule gives (0, -inf) -> tanh -> (0, -1).
 * Optional folded BatchNorm (scale/shift) as above.  act: 0 none, 1 tanh.
 * d_arg [n_mols x F] int32: row of the first maximum (-1 for empty).
 * Backward: dx[i,:] = dsum[b,:] + (i == arg[b,:]) * dmax[b,:], with the tanh
 * derivative taken from the saved output.                                     */
int gcmi_readout_fwd(const gcmi_graph* g, const float* d_x, int64_t ldx, int32_t n_feat,
                     const float* d_scale, const float* d_shift, int32_t act, float* d_out,
                     int64_t ldo, int32_t* d_arg, void* stream);
int gcmi_readout_bwd(const gcmi_graph* g, const float* d_dout, int64_t lddo, const float* d_out,
                     int64_t ldo, int32_t n_feat, int32_t act, const int32_t* d_arg,
                     float* d_dx, int64_t lddx, void* stream);

/* ---------------------------------------------------------------- K2 batch norm
 * nn.BatchNorm1d(F, eps=1e-3, momentum=0.99) over the atom rows
 * (models/torch_models/graphconvmodel.py:150-165, applied :215-216, :224-225).
 * gcmi_bn_stats: training statistics of x[n_rows x F] -> d_mean, d_invstd,
 *   folded d_scale = gamma*invstd, d_shift = beta - mean*scale; running stats
 *   updated with torch semantics (running = (1-m)*running + m*batch; unbiased
 *   variance into running_var).  d_acc: GCMI_BN_ACC_DOUBLES(F) doubles of scratch
 *   (column sums are accumulated in 32 replicas to keep fp64 atomics uncontended).
 * gcmi_bn_fold_eval: scale/shift from the running statistics (eval mode).
 * gcmi_bn_apply: y = x*scale + shift (only when the consumer cannot fold it).
 * gcmi_bn_bwd: given dy, x and the saved mean/invstd: dgamma, dbeta and
 *   (if d_dx) dx = gamma*invstd*(dy - dbeta/n - xhat*dgamma/n).  relu_mask != 0:
 *   x is the output of a ReLU and dx is wanted w.r.t. its input: dx *= (x > 0).  */
#define GCMI_BN_ACC_DOUBLES(F) (66 * (F))
int gcmi_bn_stats(const float* d_x, int64_t ldx, int64_t n_rows, int32_t n_feat,
                  const float* d_gamma, const float* d_beta, float eps, float momentum,
                  float* d_running_mean, float* d_running_var, float* d_mean, float* d_invstd,
                  float* d_scale, float* d_shift, double* d_acc, void* stream);
int gcmi_bn_fold_eval(const float* d_gamma, const float* d_beta, const float* d_running_mean,
                      const float* d_running_var, float eps, int32_t n_feat, float* d_scale,
                      float* d_shift, void* stream);
int gcmi_bn_apply(const float* d_x, int64_t ldx, int64_t n_rows, int32_t n_feat,
                  const float* d_scale, const float* d_shift, float* d_y, int64_t ldy,
                  void* stream);
int gcmi_bn_bwd(const float* d_dy, int64_t lddy, const float* d_x, int64_t ldx, int64_t n_rows,
                int32_t n_feat, const float* d_gamma, const float* d_mean,
                const float* d_invstd, float* d_dgamma, float* d_dbeta, float* d_dx,
                int64_t lddx, int32_t relu_mask, double* d_acc, void* stream);

/* ---------------------------------------------------------------- GEMMs (MFMA, exact fp32)
 * Row-segmented affine map on v_mfma_f32_32x32x2_f32:
 *   for every segment s (rows [seg_begin[s], seg_end[s])), s < n_seg <= 16:
 *     out[rows,:] = act( a1[rows,:k1] . W1_s + a2[rows,:k2] . W2_s + bias_s )
 * W1_s is the k1 x n_out row-major block at d_w1 + w1_off[s] (floats); a
 * negative offset drops that term for the segment.  a2/w2 may be NULL.
 * bias_s = d_bias + bias_off[s] (n_out floats; negative offset: none).
 * act: 0 none, 1 relu, 2 accumulate (out += the result; no activation).  trans_w != 0: the blocks are stored n_out x k
 * (nn.Linear layout, or the transposed product of a backward pass).
 * seg_begin, seg_end, *_off are HOST arrays of n_seg entries.
 *
 * Uses: GraphConv (layers.py:6202-6231: per degree S_d.W_rel + X_d.W_self + both
 * biases, relu; 11 segments, degree 0 without the S term), the atom-level
 * dense layer (graphconvmodel.py:222-223), the task heads
 * (graphconvmodel.py:230-247), and every data-gradient product of the
 * backward pass (dA = dOut . W^T is the same map with trans_w flipped).       */
int gcmi_seg_gemm(int32_t n_seg, const int32_t* seg_begin, const int32_t* seg_end,
                  const float* d_a1, int64_t lda1, int32_t k1, const float* d_w1,
                  const int64_t* w1_off, const float* d_a2, int64_t lda2, int32_t k2,
                  const float* d_w2, const int64_t* w2_off, const float* d_bias,
                  const int64_t* bias_off, int32_t n_out, int32_t trans_w, int32_t act,
                  float* d_out, int64_t ldo, void* stream);
/* dW_s += a[rows_s,:k]^T . g[rows_s,:n]  (block at d_dw + dw_off[s], k x n, or
 * n x k when trans_w) and dbias_s += column sums of g[rows_s] (d_dbias may be
 * NULL).  Accumulates with float atomics into caller-zeroed buffers.          */
int gcmi_seg_gemm_wgrad(int32_t n_seg, const int32_t* seg_begin, const int32_t* seg_end,
                        const float* d_a, int64_t lda, int32_t k, const float* d_g, int64_t ldg,
                        int32_t n, float* d_dw, const int64_t* dw_off, float* d_dbias,
                        const int64_t* dbias_off, int32_t trans_w, void* stream);
/* ---------------------------------------------------------------- the persistent block kernels, one operation each
 * The kernels the large-batch model step runs for a GraphConv / dense block (fwd_fused.hip, fwd_bf16.hip,
 * bwd_fused.hip), callable alone: for tests.  NO other kernel stands behind these: exact mode
 * (GCMI_OPT_GEMM_EXACT), GCMI_OPT_FUSED_BWD off or a shape outside the ones below give GCMI_ERR_UNSUPPORTED with an
 * error text, launch nothing and write nothing.  bf16 rows are raw 16-bit patterns, leading dimensions count elements.
 *
 * gcmi_fwd_fused_gemm: gcmi_seg_gemm's arguments and contract (act 0 / 1) for
 *   two operands of 33..64 columns -> 64 outputs (128-row tiles), one operand of 33..64 columns -> 128 outputs in
 *   nn.Linear layout (trans_w), two operands of 65..80 columns -> 64 outputs (needs d_wimg_scratch:
 *   gcmi_fwd_fused_scratch_floats() floats, 16-byte aligned); k1 == k2, rows 16-byte aligned with ld % 4 == 0,
 *   ldo % 4 == 0.  Rows narrower than the kernel's padded width (64 / 80) are fine: columns >= k are masked.
 *   d_stats (optional): GCMI_BN_ACC_DOUBLES(n_out) doubles; the column sums of out and out^2 are ADDED into its 32
 *   replicas [2 n_out + r * 2 n_out, ...) as [sum | sum of squares]; the first 2 n_out doubles are not touched.
 * gcmi_fwd_fused_gemm_h: the same over bf16 operand rows (ld % 8 == 0; columns [k, min(ld, 64 / 80)) must be ZERO; the
 *   rows of an operand whose weight offset is < 0 in a segment must be finite), bf16 output rows (ldo % 8 == 0) rounded
 *   once, sums of the rounded values; out_f32 = 1: float output rows and sums of the unrounded values, the 65..80
 *   column shape only (operands that hold their values exactly).  The scratch is required.
 * gcmi_fused_conv_bwd: the backward of a GraphConv block of 64 columns in one pass over its rows,
 *     G = (gc > 0) * (A dy + B gc + C)   ([A | B | C] = d_coef, 3 x 64 floats; NULL: G = (gc > 0) * dy)
 *     dW_rel[s] += S^T G, dW_self[s] += X^T G (k_in x 64 blocks at d_dw + w_rel_off[s] / w_self_off[s]; the same offsets
 *     address the weights in d_w), db[s] += column sums of G (d_db + b_off[s]; optional),
 *     dS = G W_rel[s]^T, dXs = G W_self[s]^T (both or neither; an offset < 0: that term is absent, its input-gradient
 *     rows are written as zeros).
 *   d_psums (optional, with the input gradients): GCMI_BN_ACC_DOUBLES(k_in) doubles in the layout above; ADDED per input
 *   column: sum over the rows of (s * dS + dXs) and of (dS * S + dXs * X), where s is the SEGMENT INDEX of the row --
 *   the segment is the degree block, and a row of dS is gathered by `degree` neighbours -- so a caller's table must
 *   list degree d as segment d.  act_bf16 1: gc, S and X are bf16 rows; 2: dy, dS and dXs too (the sums then describe
 *   the rounded values).  in_bf16 1 (act_bf16 0, no input gradients, 65..96 columns): S and X alone are bf16 rows.
 *   k_in 33..64 (with input gradients: a multiple of 4), or 65..96 without input gradients.
 * gcmi_fused_dense_bwd: the dense block (128 columns, nn.Linear layout) behind the readout, one segment from row 0:
 *     dy[r, f] = g2[mol(r), f] + (arg[mol(r), f] == r) * g2[mol(r), 128 + f]  recomputed from the readout gradient,
 *     G as above (d_coef required), dW += G^T P (128 x k_in), db += column sums of G, dP = G W; d_psums: sum dP,
 *     sum dP * P.  k_in 33..64, a multiple of 4.
 * GCMI_OPT_FUSED_BWD_LAUNCHES counts the launches of the two backward entries.                                       */
int64_t gcmi_fwd_fused_scratch_floats(void);
int gcmi_fwd_fused_gemm(int32_t n_seg, const int32_t* seg_begin, const int32_t* seg_end,
                        const float* d_a1, int64_t lda1, int32_t k1, const float* d_w1,
                        const int64_t* w1_off, const float* d_a2, int64_t lda2, int32_t k2,
                        const float* d_w2, const int64_t* w2_off, const float* d_bias,
                        const int64_t* bias_off, int32_t n_out, int32_t trans_w, int32_t act,
                        float* d_out, int64_t ldo, double* d_stats, float* d_wimg_scratch, void* stream);
int gcmi_fwd_fused_gemm_h(int32_t n_seg, const int32_t* seg_begin, const int32_t* seg_end,
                          const uint16_t* d_a1, int64_t lda1, int32_t k1, const float* d_w1,
                          const int64_t* w1_off, const uint16_t* d_a2, int64_t lda2, int32_t k2,
                          const float* d_w2, const int64_t* w2_off, const float* d_bias,
                          const int64_t* bias_off, int32_t n_out, int32_t trans_w, int32_t act,
                          void* d_out, int64_t ldo, int32_t out_f32, double* d_stats, float* d_wimg_scratch,
                          void* stream);
int gcmi_fused_conv_bwd(int32_t n_seg, const int32_t* seg_begin, const int32_t* seg_end, const int64_t* w_rel_off,
                        const int64_t* w_self_off, const int64_t* b_off, const void* d_dy, int64_t lddy,
                        const void* d_gc, int64_t ldgc, const float* d_coef, const void* d_s, int64_t lds,
                        const void* d_x, int64_t ldx, int32_t k_in, const float* d_w, float* d_dw, float* d_db,
                        void* d_ds, int64_t ldds, void* d_dxs, int64_t lddxs, double* d_psums, int32_t act_bf16,
                        int32_t in_bf16, void* stream);
int gcmi_fused_dense_bwd(int32_t n_seg, const int32_t* seg_begin, const int32_t* seg_end, const int64_t* w_off,
                         const int64_t* b_off, const int32_t* d_membership, const float* d_g2, int64_t ldg2,
                         const int32_t* d_arg, int32_t n_mols, const void* d_gc, int64_t ldgc, const float* d_coef,
                         const void* d_p, int64_t ldp, int32_t k_in, const float* d_w, float* d_dw, float* d_db,
                         void* d_dp, int64_t lddp, double* d_psums, int32_t act_bf16, void* stream);

/* The task head's forward product as the whole-model path runs it (graphconvmodel.py:177-179, :230-236:
 * logits = fingerprint . W^T + b with nn.Linear's (n_out x 256) weight).  With 33..256 outputs -- PCBA: 128 tasks x 2 --
 * the head matrix is first split once into fragment images in d_img_scratch (gcmi_task_head_scratch_floats() floats; the
 * model keeps them in its workspace for the backward) and the product runs from those; other shapes, or
 * d_img_scratch == NULL, are gcmi_seg_gemm with trans_w = 1.                                                    */
int64_t gcmi_task_head_scratch_floats(void);
int gcmi_task_head_forward(const float* d_fingerprint, int64_t ld, int64_t n_rows, int32_t k, const float* d_w,
                           const float* d_bias, int32_t n_out, float* d_img_scratch, float* d_out, int64_t ldo,
                           void* stream);
/* The per-molecule head backward kernels of the large-batch model step (head_bwd.hip), callable alone: for tests.  NO
 * other kernel stands behind this entry: exact mode (GCMI_OPT_GEMM_EXACT) with more than 32 outputs, GCMI_OPT_FUSED_BWD
 * off, more than 256 outputs, 33..256 outputs without both scratches or with ldfp % 4 != 0, and d_sums without its
 * inputs give GCMI_ERR_UNSUPPORTED with an error text, launch nothing and write nothing.
 *   outputs = n_tasks x n_classes (kind 0, softmax cross-entropy over the classes of a task) or n_tasks (kind 1, L2);
 *   logits / labels: n_rows x outputs, weights: n_rows x n_tasks or NULL (all ones).  The first n_rows of the n_mols
 *   molecules carry a loss, 1 <= n_rows <= n_mols; the others are padding with a zero gradient (their fingerprint rows
 *   are still read and must be finite).
 *     loss = sum w l / (n_rows n_tasks): the SUM w l is ADDED into the 16 doubles at d_loss_acc (any of them; their sum
 *       is the value) and returned raw -- the caller divides
 *     dl   = d loss / d logits; on route 1 written to d_dl_scratch (n_mols x outputs, zeros in the padding rows)
 *     dW  += dl^T fp (outputs x 256, nn.Linear layout), db += column sums of dl (d_db may be NULL)
 *     g2   = (dl W) * (1 - fp^2): written for all n_mols rows of d_g2 (ldg2 >= 256), fp = the tanh output (ldfp >= 256)
 *   d_sums (optional): GCMI_BN_ACC_DOUBLES(128) doubles in the layout of gcmi_fwd_fused_gemm's d_stats; ADDED per
 *   column f of the dense BatchNorm (mean, invstd: 128 floats): the sums over the atom rows of dy and of dy * xhat for
 *   the dy of gcmi_fused_dense_bwd, taken from per-molecule data -- with n = the atoms of the molecule (d_runs:
 *   n_mols x n_deg x 2 row runs [begin, end), 1 <= n_deg <= GCMI_MAX_DEG + 1), d_rawsum (n_mols x 256) = [sum over the
 *   molecule's rows | the arg-max row's value] of the BatchNorm input and d_arg (n_mols x 128; < 0: no atoms, that
 *   entry of d_rawsum is not used):
 *     sum dy        = sum over molecules of n g2[f] + (arg[f] >= 0) g2[128 + f]
 *     sum dy * xhat = sum of g2[f] (rawsum[f] - n mean) invstd + (arg[f] >= 0) g2[128 + f] (rawsum[128 + f] - mean) invstd
 *   d_dl_scratch (n_mols x outputs floats), d_img_scratch (gcmi_task_head_scratch_floats() floats): both needed for
 *   33..256 outputs, written there; what they held before does not matter.
 *   *route (host): 0 = head_bwd_kernel (at most 32 outputs), 1 = head_prep + head_bwd_wide + head_wgrad_wide.
 *   logits, labels, d_dl_scratch, d_rawsum, d_arg, d_runs: 16-byte aligned.                                         */
int gcmi_head_backward(int32_t kind, const float* d_logits, const float* d_labels, const float* d_weights,
                       int64_t n_rows, int32_t n_tasks, int32_t n_classes, const float* d_fp, int64_t ldfp,
                       int32_t n_mols, const float* d_w, float* d_dw, float* d_db, float* d_g2, int64_t ldg2,
                       double* d_loss_acc, double* d_sums, const int32_t* d_runs, int32_t n_deg, const int32_t* d_arg,
                       const float* d_rawsum, const float* d_mean, const float* d_invstd, float* d_dl_scratch,
                       float* d_img_scratch, int32_t* route, void* stream);
/* elementwise g *= (y > 0): ReLU derivative, in place on g. */
int gcmi_relu_bwd(float* d_g, int64_t ldg, const float* d_y, int64_t ldy, int64_t n_rows,
                  int32_t n_feat, void* stream);

/* ---------------------------------------------------------------- Weave (pair-feature convolution)
 * The index-driven parts of WeaveLayer.forward (models/torch_models/layers.py:4327-4429) and
 * WeaveGather.forward (:4547-4648); the dense products go through gcmi_seg_gemm.  All BatchNorm
 * layers of this path run in eval mode in the reference (layers.py:4361, :4369, :4390, ...):
 * gcmi_fold_affine folds them into the neighbouring weights,
 *     W' = W * diag(scale),  b' = b * scale + shift      (W: k x n row-major, n x k if trans_w)
 * with scale/shift from gcmi_bn_fold_eval.
 *
 * gcmi_weave_pair_to_atom (layers.py:4366-4387): PA = relu(Pf . W + b) summed over the pairs of
 *   every source atom; d_pair_src [n_pairs] int32 = pair_split (ascending: pairs are listed source
 *   by source).  out [n_atoms x n_hidden] (zeroed here, float atomics, one per column and atom).
 * gcmi_weave_pair_features (layers.py:4397-4424): per ordered pair p = (i, j)
 *     z[p, 0:Hap]       = relu(U[i] + V[j] + b_ap) + relu(U[j] + V[i] + b_ap)
 *     z[p, Hap:Hap+Hpp] = relu(Pf[p] . W_pp + b_pp)
 *   where U = A . W_AP[:Fa], V = A . W_AP[Fa:] (n_atoms x Hap, computed per atom by the caller):
 *   the reference's gathered P x 2Fa matmuls, re-associated.  d_atom_to_pair [n_pairs x 2] int32.
 * gcmi_weave_gather (layers.py:4566-4648): per molecule (atoms [mol_ptr[m], mol_ptr[m+1])) the sum
 *   of the atom rows, after the 11-bin Gaussian-histogram expansion when gaussian_expand != 0
 *   (out [n_mols x 11*n_feat], column f*11 + bin) or of the raw rows (out [n_mols x n_feat]).
 * gcmi_tanh_: in-place tanh (final_conv_activation_fn of the Weave model).                      */
int gcmi_fold_affine(const float* d_w, const float* d_b, const float* d_scale, const float* d_shift, int32_t k,
                     int32_t n, int32_t trans_w, float* d_w_out, float* d_b_out, void* stream);
int gcmi_weave_pair_to_atom(const float* d_pair_feat, int64_t ldp, int32_t n_pair_feat, const int32_t* d_pair_src,
                            int64_t n_pairs, int32_t n_atoms, const float* d_w, const float* d_b, int32_t n_hidden,
                            float* d_out, int64_t ldo, void* stream);
int gcmi_weave_pair_features(const float* d_u, const float* d_v, int64_t lduv, int32_t n_hidden_ap,
                             const float* d_b_ap, const float* d_pair_feat, int64_t ldp, int32_t n_pair_feat,
                             const float* d_w_pp, const float* d_b_pp, int32_t n_hidden_pp,
                             const int32_t* d_atom_to_pair, int64_t n_pairs, float* d_z, int64_t ldz,
                             void* stream);
int gcmi_weave_gather(const float* d_x, int64_t ldx, int32_t n_feat, const int32_t* d_mol_ptr, int32_t n_mols,
                      int32_t gaussian_expand, float* d_out, int64_t ldo, void* stream);
int gcmi_tanh_(float* d_x, int64_t ldx, int64_t n_rows, int32_t n_feat, void* stream);

/* ---------------------------------------------------------------- message passing (MPNN sub-layers)
 * gcmi_edge_network_sum: EdgeNetwork.forward (models/torch_models/layers.py:4060-4088) after the
 *   re-association  (reshape(Pf[p].W + b) . h_j)[r] = sum_k Pf[p,k] G[j][k*d+r] + G[j][K*d+r]  with
 *   G = h . [W_0^T | ... | W_{K-1}^T | B^T]  (N x (K+1)d, one gcmi_seg_gemm over the atoms, W read in
 *   place as a (K*d) x d matrix in transposed layout):  out[i] = sum over the pairs p whose first
 *   atom is i (pairs sorted by it; d_dst_ptr [n_dst+1] is that CSR) of the message from d_src[p].
 * gcmi_gru_gates / gcmi_gru_out: the elementwise parts of GatedRecurrentUnit.forward (:2903-2913):
 *   z <- sigmoid(z), r <- sigmoid(r), hr = h*r;   out = (1-z) tanh(hpre) + z x   (contiguous, n floats).
 * gcmi_set2set_attend: one attention step of SetGather.forward (:3047-3064): per molecule
 *   e_a = <x_a, h_m>, a = softmax over its atoms, q_star[m] = [h_m | sum_a a_a x_a].
 * gcmi_lstm_cell: SetGather._LSTMStep (:3066-3092) after z = q_star.U + b: gate order i, f, o, g.  */
int gcmi_edge_network_sum(const float* d_g, int64_t ldg, int32_t n_hidden, int32_t n_pair_feat,
                          const float* d_pair_feat, int64_t ldp, const int32_t* d_dst_ptr, const int32_t* d_src,
                          int32_t n_dst, float* d_out, int64_t ldo, void* stream);
/* gcmi_edge_network_moments: the same message with the weights applied last,
 *   T[i, k*d + c] = sum_p pf[p,k] h[src_p, c] (k < K),  T[i, K*d + c] = sum_p h[src_p, c]   (d <= 128, K <= 16),
 *   message = T . [W_0 | ... | W_{K-1} | B]^T by one gcmi_seg_gemm: a 4d-byte gather per pair instead of 4(K+1)d. */
int gcmi_edge_network_moments(const float* d_h, int64_t ldh, int32_t n_hidden, int32_t n_pair_feat,
                              const float* d_pair_feat, int64_t ldp, const int32_t* d_dst_ptr, const int32_t* d_src,
                              int32_t n_dst, float* d_t, int64_t ldt, void* stream);
/* ... with the molecules of the batch given (d_mol_ptr [n_mols + 1]: atoms of molecule m are the rows
 *   [d_mol_ptr[m], d_mol_ptr[m+1]) -- the CSR of default_generator's atom_split, graph_models.py:1197-1247): a
 *   molecule's state rows are staged once in LDS and serve all its pairs.  Same T; pairs that leave their molecule are
 *   still right (read from memory).  max_mol_atoms: atoms of the largest molecule if the caller knows it (sizes the
 *   LDS: more workgroups per CU), else 0.  d_mol_ptr == NULL: gcmi_edge_network_moments.                          */
int gcmi_edge_network_moments_mol(const float* d_h, int64_t ldh, int32_t n_hidden, int32_t n_pair_feat,
                                  const float* d_pair_feat, int64_t ldp, const int32_t* d_dst_ptr, const int32_t* d_src,
                                  int32_t n_dst, const int32_t* d_mol_ptr, int32_t n_mols, int32_t max_mol_atoms,
                                  float* d_t, int64_t ldt, void* stream);
/* Backward of the same pieces (the training step of MPNNModel, models/graph_models.py:1045-1247; forward
 * formulas models/layers.py:3755-3887).  gru_gates_bwd: dzp = dz z(1-z), drp = dhr h r(1-r), dh = dhr r;
 * gru_out_bwd: dz = dout (x - tanh hpre), dhpre = dout (1-z)(1-tanh^2), dx = dout z; lstm_cell_bwd: dz (rows x 4H,
 * gate order i, f, o, g) and dc of the incoming cell state from dh', dc' (NULL = 0); set2set_attend_bwd: dx (written,
 * or added to when accumulate != 0) and dh from dq = [dh | dr], softmax recomputed.                          */
int gcmi_gru_gates_bwd(const float* d_z, const float* d_r, const float* d_h, const float* d_dz, const float* d_dhr,
                       float* d_dzp, float* d_drp, float* d_dh, int64_t n, void* stream);
int gcmi_gru_out_bwd(const float* d_z, const float* d_hpre, const float* d_x, const float* d_dout, float* d_dz,
                     float* d_dhpre, float* d_dx, int64_t n, void* stream);
int gcmi_lstm_cell_bwd(const float* d_z, int64_t ldz, int32_t n_hidden, int64_t n_rows, const float* d_c_prev,
                       const float* d_dh, const float* d_dc_next, float* d_dz, float* d_dc_prev, void* stream);
int gcmi_set2set_attend_bwd(const float* d_x, int64_t ldx, int32_t n_feat, const int32_t* d_mol_ptr, int32_t n_mols,
                            const float* d_h, int64_t ldh, const float* d_dq, int64_t lddq, float* d_dx, int64_t lddx,
                            int32_t accumulate, float* d_dh, int64_t lddh, void* stream);
int gcmi_gru_gates(float* d_z, float* d_r, const float* d_h, float* d_hr, int64_t n, void* stream);
int gcmi_gru_out(const float* d_z, const float* d_hpre, const float* d_x, float* d_out, int64_t n, void* stream);
int gcmi_set2set_attend(const float* d_x, int64_t ldx, int32_t n_feat, const int32_t* d_mol_ptr, int32_t n_mols,
                        const float* d_h, int64_t ldh, float* d_qstar, int64_t ldq, void* stream);
int gcmi_lstm_cell(const float* d_z, int64_t ldz, int32_t n_hidden, int64_t n_rows, float* d_c, int64_t ldc,
                   float* d_h, int64_t ldh, void* stream);

/* ---------------------------------------------------------------- atom codes
 * The 75-column rows of atom_features (feat/graph_features.py:282-391) are five one-hot blocks, two small integers
 * and a flag.  Code row (8 bytes): symbol column, degree, implicit-valence column, formal charge (int8), radical
 * electrons, hybridisation column, aromatic, total-H column.  Collation and the host-to-device copy move codes
 * (gcmi_collate_plans with n_feat = 2 "floats"); this writes the float rows on the device:
 * out[r, 0:75] as the reference lays them out, out[r, 75:ldo] = 0.                                            */
int gcmi_expand_atom_codes(const uint8_t* d_codes, int64_t ldc_bytes, int64_t n_atoms, float* d_out, int64_t ldo,
                           void* stream);

/* ---------------------------------------------------------------- SMILES featurization (host)
 * What the reference computes in Python per rdkit Mol, for SMILES input:
 *   atom_features feat/graph_features.py:282-391 (75 columns), bond_features :394-459 (6), pair_features +
 *   find_distance :532-695 (14, all pairs), ConvMolFeaturizer._featurize :845-914, WeaveFeaturizer._featurize
 *   :1037-1078; a molecule that cannot be read is skipped like MolecularFeaturizer.featurize does
 *   (feat/base_classes.py:254-330).  Atoms keep their order of appearance in the SMILES.
 * Two passes so that the caller owns all memory:
 *   gcmi_smiles_sizes      n_atoms[i] / n_bonds[i] of every molecule; n_atoms[i] = -1 when it cannot be read.
 *   gcmi_smiles_featurize  atom_off/bond_off (n+1 prefix sums of those sizes, 0 for rejected molecules) and,
 *                          when pair_features is given, pair_off (prefix sums of n_atoms^2).  Every output may
 *                          be NULL:  atom_features [A][75], adj_degree [A], adj_idx [2B] (neighbours LOCAL to
 *                          the molecule, per atom in bond order: together with adj_degree the CSR the collation
 *                          entry points read), bond_atoms [B][2], bond_features [B][6], pair_features
 *                          [sum n^2][14] (row a1*n+a2), atom_props [A][8] = atomic number, degree, implicit H,
 *                          explicit H, charge, radical electrons, hybridisation (0 unspecified, 1 S, 2 SP,
 *                          3 SP2, 4 SP3, 5 SP3D, 6 SP3D2), aromatic.
 *   gcmi_smiles_check      NULL when the SMILES can be read, else a static reason string.
 * n_threads worker threads; results do not depend on it.                                                   */
#define GCMI_ATOM_FEATURES 75
#define GCMI_BOND_FEATURES 6
#define GCMI_PAIR_FEATURES 14
int gcmi_smiles_sizes(const char* const* smiles, int64_t n, int32_t* n_atoms, int32_t* n_bonds, int n_threads);
int gcmi_smiles_featurize(const char* const* smiles, int64_t n, const int64_t* atom_off, const int64_t* bond_off,
                          const int64_t* pair_off, float* atom_features, int32_t* adj_degree, int32_t* adj_idx,
                          int32_t* bond_atoms, float* bond_features, float* pair_features, int32_t* atom_props,
                          int n_threads);
const char* gcmi_smiles_check(const char* smiles);

/* ---------------------------------------------------------------- loss
 * SoftmaxCrossEntropy (models/losses.py:251-259) / L2Loss (:85-94) through
 * _StandardLoss (models/torch_models/torch_model.py:1275-1294):
 *   loss = mean over (n_rows, n_tasks) of  w[b,t] * l[b,t]
 *   kind 0: l = -sum_c y[b,t,c] * log_softmax(logits[b,t,:])[c]
 *   kind 1: l = (out[b,t] - y[b,t])^2
 * Writes *d_loss (float, device) and d_dlogits (same shape as logits).
 * d_probs (may be NULL): softmax(logits) (the model's 'prediction' output,
 * graphconvmodel.py:235).  d_acc: 1 double of scratch.                        */
int gcmi_loss_fwd_bwd(int32_t kind, const float* d_logits, const float* d_labels,
                      const float* d_weights, int64_t n_rows, int32_t n_tasks,
                      int32_t n_classes, float* d_loss, float* d_dlogits, float* d_probs,
                      double* d_acc, void* stream);
int gcmi_softmax(const float* d_logits, int64_t n_rows_tasks, int32_t n_classes, float* d_probs,
                 void* stream);

/* ---------------------------------------------------------------- metrics (metrics.hip)
 * Per-task scores of n rows x n_tasks predictions where they sit in HBM (deepchem/metrics/metric.py:568-727: no row is
 * dropped; weights enter only as sample weights, NULL = none).  Element (row, task) of a prediction array is at
 * d_x[row * row_stride + task * elem_stride] (strides in floats: the class-1 probability of an (n, T, 2) tensor has
 * row_stride 2T, elem_stride 2).  d_labels (fp64) and d_weights (fp32) are contiguous n x n_tasks.
 *
 * gcmi_metric_rank: ROC-AUC or the trapezoid area under the precision-recall curve of every task: a stable LSD radix
 * sort of (score image, row) per task, then one scan over the tie groups.  A row is positive when its label equals
 * `positive`.  d_out[t]: the score; d_status[t]: 0 ok, or the bitwise OR of 1 one class (or no weight on one class), 2 a NaN
 * score, 4 an infinite score, each flag once however many rows raise it (sklearn rejects those; they are ranked all the same, NaN is not and d_out[t] is then meaningless).  Unweighted ROC-AUC is computed in integers up to one final division.  d_workspace:
 * gcmi_metrics_workspace_bytes(n, n_tasks) bytes, 16-byte aligned.
 *
 * gcmi_metric_moments: GCMI_METRIC_MOMENT_DOUBLES sums per task in one pass, shifted by the first row's values
 * (y0, p0) so that variances come out of small numbers.  With p = (double)pred * scale[t] + shift[t] (NULL: 1, 0),
 * dy = y - y0, dp = p - p0:  [0] sum w, [1] sum w dy, [2] sum w dp, [3] sum w dy^2, [4] sum w dp^2, [5] sum w dy dp,
 * [6] sum w |y - p|, [7] sum w (y - p)^2, [8] y0, [9] p0, [10] (which = ACCURACY only) sum w [argmax_c pred == y],
 * first maximum on ties, pred then being n_classes consecutive floats per element, [11] 0.                         */
enum {
  GCMI_METRIC_ROC_AUC = 0,
  GCMI_METRIC_PRC_AUC = 1,
  GCMI_METRIC_MOMENTS = 0,
  GCMI_METRIC_ACCURACY = 1
};
#define GCMI_METRIC_MOMENT_DOUBLES 12
int64_t gcmi_metrics_workspace_bytes(int64_t n, int32_t n_tasks);
int gcmi_metric_rank(int32_t which, const float* d_scores, int64_t row_stride, int64_t elem_stride,
                     const double* d_labels, int32_t positive, const float* d_weights, int64_t n, int32_t n_tasks,
                     double* d_out, int32_t* d_status, void* d_workspace, void* stream);
int gcmi_metric_moments(int32_t which, const float* d_pred, int64_t row_stride, int64_t elem_stride, int32_t n_classes,
                        const double* d_labels, const float* d_weights, const double* d_scale, const double* d_shift,
                        int64_t n, int32_t n_tasks, double* d_out, void* stream);

/* ---------------------------------------------------------------- optimizer
 * torch.optim.Adam(lr, betas, eps, weight_decay=0) (models/optimizers.py:231-241)
 * on one flat range.  step = 1-based step count after this update.            */
int gcmi_adam_step(float* d_param, const float* d_grad, float* d_m, float* d_v, int64_t n,
                   float lr, float beta1, float beta2, float eps, int64_t step, void* stream);

/* The other optimizers of models/optimizers.py on flat ranges (csrc/optim.hip).
 * gcmi_opt_desc: rule + its hyper-parameters (the ones a rule does not use are ignored):
 *   GCMI_RULE_SGD      p -= lr g                                                   (torch.optim.SGD, :482-488)
 *   GCMI_RULE_ADAGRAD  sum += g^2; p -= lr g / (sqrt(sum) + eps)                   (torch.optim.Adagrad, :160-170;
 *                      state1 = sum, which the caller starts at initial_accumulator_value)
 *   GCMI_RULE_RMSPROP  sq = alpha sq + (1 - alpha) g^2; avg = sqrt(sq) + eps; momentum != 0: buf = momentum buf + g / avg,
 *                      p -= lr buf; else p -= lr g / avg                           (torch.optim.RMSprop, :427-437;
 *                      state1 = square_avg, state2 = momentum_buffer, NULL allowed without momentum)
 *   GCMI_RULE_ADAM_L2  g += weight_decay p, then Adam                              (torch.optim.Adam, :231-241;
 *                      state1 = exp_avg, state2 = exp_avg_sq; weight_decay == 0 IS the adam step above, bit for bit)
 *   GCMI_RULE_ADAMW    p *= 1 - lr weight_decay, then Adam (no amsgrad)            (torch.optim.AdamW, :360-367)
 *   GCMI_RULE_LAMB     the Lamb step below only
 * each in the operation order of torch's single-tensor implementation.  step = 1-based count after this update.
 * Any n >= 0; 16-byte accesses when every pointer is 16-byte aligned, scalar otherwise; no atomics.          */
enum {
  GCMI_RULE_SGD = 0,
  GCMI_RULE_ADAGRAD = 1,
  GCMI_RULE_RMSPROP = 2,
  GCMI_RULE_ADAM_L2 = 3,
  GCMI_RULE_ADAMW = 4,
  GCMI_RULE_LAMB = 5
};
typedef struct gcmi_opt_desc {
  int32_t rule;
  float beta1, beta2, eps, weight_decay, alpha, momentum;
} gcmi_opt_desc;
int gcmi_opt_step(const gcmi_opt_desc* desc, float* d_param, const float* d_grad, float* d_state1, float* d_state2,
                  int64_t n, float lr, int64_t step, void* stream);
/* LambOptimizer (utils/optimizer_utils.py:91-163 as models/optimizers.py:872-881 configures it: debias=False,
 * adam=False, clamp_value=10) over arenas of n floats.  d_segments: n_segments pairs (offset, numel) of int64 in
 * DEVICE memory, one per parameter tensor; floats between segments belong to none and are left alone, and a pair that
 * does not lie inside [0, n) is skipped.  Two launches: moments + update u = m / (sqrt(v) + eps) + weight_decay p +
 * per-chunk fp64 sums of p^2 and u^2, then per segment trust = min(||p||, 10) / ||u|| (1 when either norm is 0) and
 * p -= lr trust u.  The sums are combined in a fixed order (no floating-point atomics): equal inputs, equal bits.
 * d_norms (may be NULL): n_segments x 3 floats [weight_norm, adam_norm, trust_ratio] of this step.
 * d_scratch: gcmi_lamb_scratch_floats(n, n_segments) floats (negative: bad arguments), 16-byte aligned.      */
int64_t gcmi_lamb_scratch_floats(int64_t n, int64_t n_segments);
int gcmi_lamb_step(const gcmi_opt_desc* desc, float* d_param, const float* d_grad, float* d_m, float* d_v,
                   float* d_scratch, const int64_t* d_segments, int32_t n_segments, int64_t n, float* d_norms, float lr,
                   void* stream);

/* ---------------------------------------------------------------- whole-model sequencing
 * _GraphConvTorchModel.forward (models/torch_models/graphconvmodel.py:188-249) and the
 * loss + backward of one fit_generator step (models/torch_models/torch_model.py:436-442)
 * as ONE call each: the library enqueues every kernel back to back on `stream`, so a
 * training step costs three C calls (forward, loss_backward, gcmi_adam_step on the flat
 * gradient range) instead of ~150 Python-driven launches.  Nothing here allocates: the
 * caller owns the parameter arena, the gradient arena and the workspace.
 *
 * Parameters live in ONE flat fp32 arena in nn.Module.parameters() order; the offsets
 * below (in floats) locate each block.  GraphConv layer l: 2*max_deg+1 weight blocks
 * (K_l x width_l each) in the reference order rel_1, self_1, ..., self_0, then the
 * 2*max_deg+1 bias vectors.  nn.Linear blocks are (out, in).  The gradient arena has
 * the same layout.
 */
#define GCMI_MAX_CONV_LAYERS 4
typedef struct gcmi_model_desc {
  int32_t n_layers;                      /* GraphConv layers, <= GCMI_MAX_CONV_LAYERS        */
  int32_t max_deg;                       /* 10                                               */
  int32_t n_feat_in;                     /* atom feature width (75)                          */
  int32_t conv_width[GCMI_MAX_CONV_LAYERS];
  int32_t dense_width;                   /* 128                                              */
  int32_t n_tasks;
  int32_t n_classes;                     /* classification: >= 2; regression: 1              */
  int32_t mode;                          /* 0 classification, 1 regression                   */
  int32_t batch_norm;                    /* 0 / 1                                            */
  int32_t grad_mode;                     /* 0 reference (autograd cut at GraphConv), 1 full  */
  float bn_eps, bn_momentum;
  int64_t off_conv_w[GCMI_MAX_CONV_LAYERS], off_conv_b[GCMI_MAX_CONV_LAYERS];
  int64_t off_bn_gamma[GCMI_MAX_CONV_LAYERS + 1], off_bn_beta[GCMI_MAX_CONV_LAYERS + 1];
  int64_t off_dense_w, off_dense_b, off_head_w, off_head_b;
  int64_t n_params;
  int32_t storage;                       /* what a step writes and reads back: 0 fp32; 1 the activations as bfloat16 (a
                                            copy of the atom features, neighbour sums, GraphConv outputs, pooled rows,
                                            the dense output: one rounding per stored element); 2 also the gradient
                                            STREAMS between kernels (dpool, dy, dS, dXs).  fp32 arithmetic and
                                            accumulation, fp64 BatchNorm sums of the rounded values, fp32 parameters,
                                            parameter gradients and Adam state in every mode.  gcmi_small_*: 1 and 2 are
                                            the same (its gradients never leave L2).  gcmi_model_*: the default shapes
                                            only (widths 64 over 73..76 features, dense 128, BatchNorm on), else
                                            GCMI_ERR_UNSUPPORTED                                                   */
  int32_t reserved_;
} gcmi_model_desc;

typedef struct gcmi_model_io {
  const float* d_atom_features;          /* N x ld_features                                  */
  int64_t ld_features;
  float* d_workspace;                    /* gcmi_model_workspace_floats() floats             */
  float* d_bn_running_mean[GCMI_MAX_CONV_LAYERS + 1];
  float* d_bn_running_var[GCMI_MAX_CONV_LAYERS + 1];
  int64_t* d_bn_batches_tracked[GCMI_MAX_CONV_LAYERS + 1]; /* may be NULL                    */
  /* outputs, all g->n_mols rows (TrimGraphOutput is a view the caller takes):               */
  float* d_logits;                       /* n_mols x (n_tasks*n_classes)  (regression: n_tasks) */
  float* d_probs;                        /* classification softmax; may be NULL              */
  float* d_fingerprint;                  /* n_mols x 2*dense_width                           */
  float* d_loss;                         /* 1 float (loss_backward)                          */
  int32_t features_small_int;            /* a PROMISE about d_atom_features (0 = none): every element, pad columns
                                            included, is an integer with |x| <= 256 / max(1, max_deg) -- 25 for
                                            max_deg 10; what ConvMolFeaturizer rows (one-hot blocks, small counts)
                                            are.  Such elements and their neighbour sums (< 256) are exact in bf16,
                                            and gcmi_model_forward / _loss_backward (storage 0, fast product mode,
                                            BatchNorm, widths 64 over 73..76 features, window plans and reverse slots
                                            on the graph) then run the first GraphConv block on one-piece bf16
                                            operands: the same terms, half the matrix work.  Established where the
                                            batch is made (gcmi_collate_plans_p, gcmi_count_not_small_int); a false
                                            promise gives rounded features without notice.  gcmi_small_*: ignored. */
  int32_t reserved_;
} gcmi_model_io;

/* How many elements of the n_rows x n_cols device matrix d_x (row stride ld) are NOT integers with
 * |x| <= 256 / max(1, max_deg) (NaN and infinities count) -> *d_count (device, one int64), one pass on `stream`.
 * 0 = the features_small_int promise may be made.  For tests and for sets that live on the device; no step launches it. */
int gcmi_count_not_small_int(const float* d_x, int64_t ld, int64_t n_rows, int32_t n_cols, int32_t max_deg,
                             int64_t* d_count, void* stream);

/* floats of workspace needed for a batch of n_atoms / n_mols (forward + backward). */
int64_t gcmi_model_workspace_floats(const gcmi_model_desc* m, int64_t n_atoms, int64_t n_mols);
/* training != 0: BatchNorm uses batch statistics and updates the running ones. The
 * graph needs d_mol_runs; the backward additionally uses d_rev_pos when present.            */
int gcmi_model_forward(const gcmi_model_desc* m, const gcmi_graph* g, const float* d_params,
                       const gcmi_model_io* io, int32_t training, void* stream);
/* After a training-mode gcmi_model_forward on the same workspace: loss over the first
 * n_rows molecules (SoftmaxCrossEntropy / L2Loss through _StandardLoss) -> io->d_loss, then
 * the backward pass; gradients are WRITTEN (not accumulated) into d_grads for every
 * parameter the gradient mode trains; [*grad_lo, *grad_hi) returns that range (floats).     */
int gcmi_model_loss_backward(const gcmi_model_desc* m, const gcmi_graph* g, const float* d_params,
                             float* d_grads, const gcmi_model_io* io, const float* d_labels,
                             const float* d_weights, int64_t n_rows, int64_t* grad_lo,
                             int64_t* grad_hi, void* stream);
/* Data-parallel form with SYNCHRONISED BatchNorm: exactly the two calls above, with every training
 * BatchNorm of the step normalising over the GLOBAL batch.  Between "column sums complete" and "finalise" of each
 * BatchNorm point the library calls, on the calling thread,
 *     sync(ctx, d_buf, n_doubles, stream)
 * with d_buf = [sum a (F) | sum b (F) | rows of this rank] as doubles (n_doubles = 2 F + 1, inside io->d_workspace,
 * 16-byte aligned; F = the width of that BatchNorm).  Contract as gcmi_grad_sync_fn: it must ENQUEUE, in order on
 * `stream`, a SUM all-reduce of those doubles over the ranks and return 0; a non-zero return aborts the call with
 * GCMI_ERR_LAUNCH; the library makes no RCCL call itself.  Forward (training): n_layers + 1 calls, a = x, b = x^2;
 * mean, biased variance, the folded scale / shift and the running statistics (unbiased factor N_g / (N_g - 1)) come
 * from the global sums and the global row count N_g; num_batches_tracked moves once per rank.  Backward: n_layers + 1
 * calls in full gradient mode, 2 in reference mode, a = dy, b = dy * xhat; dgamma / dbeta are THIS rank's sums (torch
 * SyncBatchNorm: the gradient average over the ranks follows), the dx coefficients come from the global sums and N_g.
 * Every rank makes the same calls in the same order, a rank whose batch has no atoms included (zero sums, count 0).
 * The model must have BatchNorm (else GCMI_ERR_ARG).  sync == NULL: gcmi_model_forward / _loss_backward; the
 * eval-mode forward never calls sync.                                                                           */
typedef int (*gcmi_stat_sync_fn)(void* ctx, double* d_buf, int64_t n_doubles, void* stream);
int gcmi_model_forward_dp(const gcmi_model_desc* m, const gcmi_graph* g, const float* d_params,
                          const gcmi_model_io* io, int32_t training, gcmi_stat_sync_fn sync, void* sync_ctx,
                          void* stream);
int gcmi_model_loss_backward_dp(const gcmi_model_desc* m, const gcmi_graph* g, const float* d_params,
                                float* d_grads, const gcmi_model_io* io, const float* d_labels,
                                const float* d_weights, int64_t n_rows, int64_t* grad_lo, int64_t* grad_hi,
                                gcmi_stat_sync_fn sync, void* sync_ctx, void* stream);
/* The pieces of a synchronised BatchNorm for callers that sequence their own step.  d_xbuf: 2 F + 1 doubles.
 * gcmi_bn_sync_sums: column sums of x and x^2 and the row count of THIS rank -> d_xbuf (d_acc: GCMI_BN_ACC_DOUBLES(F)
 *   doubles of scratch, left zero behind its first 2 F doubles).  Sum d_xbuf over the ranks, then
 * gcmi_bn_sync_finalize: what gcmi_bn_stats leaves, from the summed buffer.
 * gcmi_bn_sync_bwd_sums: sums of dy and dy * xhat -> d_xbuf; d_dgamma / d_dbeta (may be NULL) = this rank's sums.
 * gcmi_bn_sync_bwd_pool: the same buffer and gradients from accumulators the caller's kernels filled (both in the
 *   GCMI_BN_ACC_DOUBLES layout, both left zero behind their first 2 F doubles): d_psums holds the POOLED sums of a
 *   one-pass block backward, sum dP and sum dP * P with P = gamma * xhat + beta, so that sum dy * xhat =
 *   (sum dP * P - beta * sum dP) / gamma; d_acc holds the direct sums, which are used instead when some column has
 *   |beta| > 64 |gamma| (the pooled form is ill-conditioned there).
 * gcmi_bn_sync_bwd_coef: from the summed buffer the 3 F floats [A | B | C] with dx = A dy + B x + C (gcmi_bn_bwd).   */
int gcmi_bn_sync_sums(const float* d_x, int64_t ldx, int64_t n_rows, int32_t n_feat, double* d_acc, double* d_xbuf,
                      void* stream);
int gcmi_bn_sync_finalize(const double* d_xbuf, int32_t n_feat, const float* d_gamma, const float* d_beta, float eps,
                          float momentum, float* d_running_mean, float* d_running_var, float* d_mean, float* d_invstd,
                          float* d_scale, float* d_shift, int64_t* d_batches_tracked, void* stream);
int gcmi_bn_sync_bwd_sums(const float* d_dy, int64_t lddy, const float* d_x, int64_t ldx, int64_t n_rows, int32_t n_feat,
                          const float* d_gamma, const float* d_mean, const float* d_invstd, float* d_dgamma,
                          float* d_dbeta, double* d_acc, double* d_xbuf, void* stream);
int gcmi_bn_sync_bwd_pool(double* d_psums, double* d_acc, int64_t n_rows, int32_t n_feat, const float* d_gamma,
                          const float* d_beta, float* d_dgamma, float* d_dbeta, double* d_xbuf, void* stream);
int gcmi_bn_sync_bwd_coef(const double* d_xbuf, int32_t n_feat, const float* d_gamma, const float* d_mean,
                          const float* d_invstd, float* d_coef, void* stream);

/* ---------------------------------------------------------------- small-batch engine
 * The same model step for batches whose activations live in L2 (the reference's default batch of 100
 * molecules, MolNet's 64: graphconvmodel.py:292, molnet/preset_hyper_parameters.py:49-56), over MANY batches
 * per call: the loop of TorchModel.fit_generator (torch_model.py:423-445) -- forward, loss, backward, Adam,
 * running statistics -- runs inside the library, 8 launches per step in reference gradient mode and 12 in
 * full mode, on 16-row degree tiles (csrc/smallstep.hip).  Same arithmetic contract as gcmi_model_*: fp32
 * operands and accumulation on v_mfma_f32_16x16x4_f32, BatchNorm statistics in fp64.
 *
 * gcmi_small_batch: one collated batch; every pointer is device memory.  graph needs d_col_idx, d_membership,
 *   d_mol_runs, and for gcmi_small_fit d_rev_pos (GCMI_ERR_UNSUPPORTED without: use gcmi_model_*).  Atom
 *   feature rows must be 16-byte aligned (ld_features % 4 == 0, >= n_feat_in rounded up to 4; pad columns 0).
 * gcmi_small_fit: for i in [0, n_batches): one optimizer step on batches[i] (labels (B, T, C) one-hot for
 *   classification / (B, T) for regression; weights (B, T) or NULL; loss over the first n_rows molecules,
 *   _StandardLoss, torch_model.py:1275-1294); Adam step number first_step + i (1-based; torch.optim.Adam as
 *   optimizers.py:231-241 configures it) on the trained range [*grad_lo, *grad_hi) of the flat arenas;
 *   d_losses[i] = that step's loss; BatchNorm running statistics and counters updated per step.
 *   d_grads: scratch arena of n_params floats (left zero on the trained range).  The workspace
 *   (io->d_workspace) holds gcmi_small_workspace_floats(m, ws_atoms, ws_mols) floats; every batch must fit.
 * gcmi_small_predict: eval-mode forward of every batch into its d_logits (B x T*C), d_probs (classification;
 *   may be NULL) and d_fingerprint (B x 2*dense_width).
 * Widths: GraphConv and dense widths multiples of 64 up to 256 (else GCMI_ERR_UNSUPPORTED).              */
typedef struct gcmi_small_batch {
  gcmi_graph graph;
  const float* d_atom_features;
  int64_t ld_features;
  const float* d_labels;
  const float* d_weights;
  int64_t n_rows;
  float* d_logits;
  float* d_probs;
  float* d_fingerprint;
} gcmi_small_batch;
int64_t gcmi_small_workspace_floats(const gcmi_model_desc* m, int64_t max_atoms, int64_t max_mols);
int gcmi_small_fit(const gcmi_model_desc* m, float* d_params, float* d_grads, float* d_adam_m, float* d_adam_v,
                   const gcmi_model_io* io, const gcmi_small_batch* batches, int64_t n_batches, int64_t ws_atoms,
                   int64_t ws_mols, float lr, float beta1, float beta2, float eps, int64_t first_step,
                   float* d_losses, int64_t* grad_lo, int64_t* grad_hi, void* stream);
/* Data-parallel form (molecules sharded by rank, ONE flat-bucket all-reduce per step; the reference
 * shards disk shards by rank, data/pytorch_datasets.py:104-113, and leaves the gradient exchange to torch DDP):
 * exactly gcmi_small_fit, with `sync` called once per optimizer step between the backward launches and the Adam
 * launch of that step, on the calling thread:
 *     sync(ctx, d_grads + *grad_lo, *grad_hi - *grad_lo, stream)
 * It must ENQUEUE, in order on `stream`, a sum all-reduce over the ranks of that range (and whatever scaling the
 * caller's mean needs) and return 0; a non-zero return aborts the call with GCMI_ERR_LAUNCH.  The library makes no
 * RCCL call itself: the host side owns the communicator (torch.distributed's "nccl" backend = RCCL over xGMI), and
 * the callback is the only thing it has to provide.  sync == NULL: gcmi_small_fit.  BatchNorm statistics stay per
 * rank.  In reference gradient mode the GraphConv stacks of the next steps still run ahead on the second stream:
 * nothing they read is trained, so nothing they read is exchanged.                                         */
typedef int (*gcmi_grad_sync_fn)(void* ctx, float* d_grad_range, int64_t n_floats, void* stream);
int gcmi_small_fit_dp(const gcmi_model_desc* m, float* d_params, float* d_grads, float* d_adam_m, float* d_adam_v,
                      const gcmi_model_io* io, const gcmi_small_batch* batches, int64_t n_batches, int64_t ws_atoms,
                      int64_t ws_mols, float lr, float beta1, float beta2, float eps, int64_t first_step,
                      float* d_losses, int64_t* grad_lo, int64_t* grad_hi, gcmi_grad_sync_fn sync, void* sync_ctx,
                      void* stream);
/* The same loop under any elementwise rule and a learning rate per step: gcmi_small_fit_dp with the four Adam scalars
 * replaced by the description, d_state1 / d_state2 by the rule's state arenas (gcmi_opt_step; one the rule does not
 * use may be NULL) and lr by lr_per_step, a HOST array of n_batches values read while the call enqueues.  Step
 * i runs under lr_per_step[i] as step number first_step + i.  gcmi_small_fit and gcmi_small_fit_dp are this call
 * with GCMI_RULE_ADAM_L2, weight_decay 0 and a constant array.  GCMI_RULE_LAMB is not an elementwise rule.   */
int gcmi_small_fit_opt(const gcmi_model_desc* m, float* d_params, float* d_grads, float* d_state1, float* d_state2,
                       const gcmi_model_io* io, const gcmi_small_batch* batches, int64_t n_batches, int64_t ws_atoms,
                       int64_t ws_mols, const gcmi_opt_desc* opt, const float* lr_per_step, int64_t first_step,
                       float* d_losses, int64_t* grad_lo, int64_t* grad_hi, gcmi_grad_sync_fn sync, void* sync_ctx,
                       void* stream);
int gcmi_small_predict(const gcmi_model_desc* m, const float* d_params, const gcmi_model_io* io,
                       const gcmi_small_batch* batches, int64_t n_batches, int64_t ws_atoms, int64_t ws_mols,
                       void* stream);

/* Host side of the small-batch engine: every batch of a chunk of an epoch collated by ONE call into ONE arena
 * (one H2D copy), worker threads taking whole batches; per batch the output is what gcmi_collate_plans writes
 * (ConvMol.agglomerate_mols, feat/mol_graphs.py:256-349; no LDS windows).
 *   sel [batch_ptr[n_batches]] molecule indices, batch b = sel[batch_ptr[b] : batch_ptr[b+1]] (repeats = pad_batch
 *   tiling); mols_out > 0: every batch's graph says mols_out molecules, the ones beyond its selection empty
 *   (GraphGather always emits batch_size rows, layers.py:6469-6479).
 * gcmi_collate_batches_layout -> arena size in 4-byte words (negative: error); out_parts [n_batches x 5] word
 *   offsets of features, membership, col_idx, mol_runs, rev_pos; out_counts [n_batches x 3] atoms, edges, first
 *   feature row.  The feature rows of all batches form ONE contiguous [rows x ld] array at the start of the arena
 *   (every batch padded to an even row count), so 8-byte atom codes (ld = 2) expand in one launch.
 * gcmi_collate_batches fills the arena and graphs[n_batches] (device pointers NULL); out_symmetric[b] = 0 when a
 *   bond of batch b is listed from one end only.
 * gcmi_small_bind turns that into the gcmi_small_batch array once the arena is on the device.               */
int64_t gcmi_collate_batches_layout(const int64_t* atom_ptr, const int64_t* adj_ptr, const int64_t* sel,
                                    const int64_t* batch_ptr, int64_t n_batches, int64_t ld, int32_t max_deg,
                                    int64_t mols_out, int64_t* out_parts, int64_t* out_counts);
int gcmi_collate_batches(const float* atom_features, int64_t n_feat, const int64_t* atom_ptr, const int64_t* adj_ptr,
                         const int32_t* adj_idx, const int64_t* sel, const int64_t* batch_ptr, int64_t n_batches,
                         int32_t max_deg, int64_t ld, int64_t mols_out, float* arena, const int64_t* parts,
                         const int64_t* counts, gcmi_graph* graphs, int32_t* out_symmetric, int32_t n_threads);
int gcmi_small_bind(gcmi_small_batch* out, const gcmi_graph* graphs, const int64_t* parts, const int64_t* counts,
                    int64_t n_batches, const float* d_arena, const float* d_features, int64_t feature_ld,
                    int64_t mols_out, const int64_t* n_rows, const float* d_labels, int64_t label_stride,
                    const float* d_weights, int64_t weight_stride, float* d_logits, float* d_probs,
                    int64_t logit_stride, float* d_fingerprint, int64_t fp_stride);

/* ---------------------------------------------------------------- DTNN (csrc/dtnn.hip)
 * gcmi_dtnn_pair_fwd: the fused pair interaction of DTNNStep (models/torch_models/layers.py:3844-3881 of the
 *   reference, without its self term and residual).  For n_pairs pairs sorted by first atom (d_mem_i non-decreasing,
 *   d_mem_j; both inside [0, n_atoms): the CALLER validates them, the kernel only clamps) and atom rows
 *   d_ah [n_atoms x n_hidden] = C . W_cf + b_cf:
 *       y[i] = sum over pairs p with mem_i[p] = i of tanh(((g_p . W_df + b_df) (.) ah[mem_j[p]]) . W_fc)
 *   from_distance != 0: d_src holds one distance per pair and g_p[k] = exp(-(d - distance_min - k step)^2 / (2 step^2))
 *   is generated in registers; else d_src is the n_pairs x n_distance Gaussian matrix (leading dimension ld_src).
 *   d_w_df [n_distance x n_hidden], d_b_df [n_hidden], d_w_fc [n_hidden x n_embedding], contiguous.  y
 *   [n_atoms x n_embedding] is cleared here (float atomics: a run of pairs adds once per 32-pair tile it touches).
 *   n_embedding <= 64, n_hidden <= 64, n_distance <= 128, else GCMI_ERR_ARG.  Nothing of size n_pairs is written.
 * gcmi_dtnn_pair_bwd: given d_dy [n_atoms x n_embedding], recomputes the forward from the same inputs and writes
 *   d_dah [n_atoms x n_hidden] (cleared here, atomics by mem_j) and ADDS dW_df, db_df, dW_fc into their buffers.
 * gcmi_dtnn_collate: a batch from a resident set (d_z_all [n_mols_all x max_atoms] atom numbers, d_dist_all
 *   [n_mols_all x max_atoms x max_atoms] distances, d_n_atoms_all [n_mols_all]; max_atoms <= 64): for the molecules
 *   d_mol_idx [n_batch], atom and pair offsets [n_batch + 1], atom numbers [n_atoms], and per pair, in row-major (i, j)
 *   order per molecule, the distance and both memberships.  n_atoms / n_pairs: the sizes of the outputs (the caller
 *   knows the atom counts); a molecule that would not fit them is left out.                                        */
int gcmi_dtnn_pair_fwd(const float* d_src, int64_t ld_src, int32_t from_distance, const int32_t* d_mem_i,
                       const int32_t* d_mem_j, int64_t n_pairs, int32_t n_atoms, const float* d_ah, int64_t ldah,
                       int32_t n_hidden, const float* d_w_df, const float* d_b_df, int32_t n_distance,
                       const float* d_w_fc, int32_t n_embedding, double distance_min, double step, float* d_y,
                       int64_t ldy, void* stream);
int gcmi_dtnn_pair_bwd(const float* d_src, int64_t ld_src, int32_t from_distance, const int32_t* d_mem_i,
                       const int32_t* d_mem_j, int64_t n_pairs, int32_t n_atoms, const float* d_ah, int64_t ldah,
                       int32_t n_hidden, const float* d_w_df, const float* d_b_df, int32_t n_distance,
                       const float* d_w_fc, int32_t n_embedding, double distance_min, double step, const float* d_dy,
                       int64_t lddy, float* d_dah, int64_t lddah, float* d_dw_df, float* d_db_df, float* d_dw_fc,
                       void* stream);
int gcmi_dtnn_collate(const int32_t* d_z_all, const float* d_dist_all, const int32_t* d_n_atoms_all,
                      int32_t n_mols_all, int32_t max_atoms, const int32_t* d_mol_idx, int32_t n_batch,
                      int32_t n_atoms, int64_t n_pairs, int32_t* d_atom_off, int32_t* d_pair_off, int32_t* d_z,
                      float* d_d, int32_t* d_mem_i, int32_t* d_mem_j, void* stream);

/* ---------------------------------------------------------------- Molecule Attention Transformer (mat.hip)
 * A pad-free batch: the atoms of its n_mols molecules concatenated, atom offsets [n_mols + 1] strictly increasing from
 * 0, and per molecule a row-major n x n block of pair data at pair offsets [n_mols + 1] (the exclusive sums of n^2).
 * The offsets are passed TWICE: h_atom_off / h_pair_off on the HOST, which every entry validates before any launch
 * (and sizes its grid and LDS from), and d_atom_off / d_pair_off, the same numbers on the device, which the kernels
 * read and trust only inside the bounds the host copy gives.
 * gcmi_mat_bias: d_bias[p] = lambda_distance * g(D)[p] + lambda_adjacency * A[p] / (row sum of A + eps), g = the row
 *   softmax of -D (GCMI_MAT_DIST_SOFTMAX; the row minimum is subtracted, so a row of equal distances is uniform and a
 *   distance 1e6 above the row minimum gives an exact 0) or exp(-D) (GCMI_MAT_DIST_EXP).  Any molecule size.
 * gcmi_mat_attention_fwd: O = (lambda_attention * softmax(Q K^T / sqrt(d_k)) + bias) V per (molecule, head); d_q, d_k,
 *   d_v (they may be equal) are rows of ld floats with head h in columns [h d_k, (h + 1) d_k), d_o rows of ldo floats in
 *   the same layout.  Columns past n_heads * d_k are neither read nor written.  Nothing of size n x n is written.
 * gcmi_mat_attention_bwd: from the same inputs and d_do (rows of lddo floats) writes d_dq, d_dk, d_dv (rows of ldg
 *   floats); shared != 0 (then d_q == d_k == d_v is required): their SUM into d_dq, d_dk / d_dv unused.  The attention
 *   matrix is recomputed; no atomics, so two calls agree bit for bit.
 * d_k a multiple of 4 up to 64 and molecules of at most GCMI_MAT_MAX_ATOMS atoms, else GCMI_ERR_UNSUPPORTED; NULL
 * pointers, ld < n_heads * d_k, rows that are not 16-byte addressable (pointer or ld % 4), atoms x ld >= 2^31 (rows are
 * indexed with 32-bit element offsets), n_mols <= 0, offsets that do not increase and, without shared, gradient
 * buffers that are not three distinct ones are GCMI_ERR_ARG.                                                       */
#define GCMI_MAT_MAX_ATOMS 128
#define GCMI_MAT_DIST_SOFTMAX 0
#define GCMI_MAT_DIST_EXP 1
int gcmi_mat_bias(const float* d_adj, const float* d_dist, const int32_t* h_atom_off, const int32_t* h_pair_off,
                  const int32_t* d_atom_off, const int32_t* d_pair_off, int32_t n_mols, int32_t dist_kernel,
                  float lambda_distance, float lambda_adjacency, float eps, float* d_bias, void* stream);
int gcmi_mat_attention_fwd(const float* d_q, const float* d_k, const float* d_v, int64_t ld, const float* d_bias,
                           const int32_t* h_atom_off, const int32_t* h_pair_off, const int32_t* d_atom_off,
                           const int32_t* d_pair_off, int32_t n_mols, int32_t n_heads, int32_t head_dim,
                           float lambda_attention, float* d_o, int64_t ldo, void* stream);
int gcmi_mat_attention_bwd(const float* d_q, const float* d_k, const float* d_v, int64_t ld, const float* d_bias,
                           const int32_t* h_atom_off, const int32_t* h_pair_off, const int32_t* d_atom_off,
                           const int32_t* d_pair_off, int32_t n_mols, int32_t n_heads, int32_t head_dim,
                           float lambda_attention, const float* d_do, int64_t lddo, float* d_dq, float* d_dk, float* d_dv,
                           int64_t ldg, int32_t shared, void* stream);

/* ---------------------------------------------------------------- graph-network block of MEGNet (megnet.hip)
 * A batch of n_graphs graphs: their n_nodes nodes concatenated (node_ptr [n_graphs + 1], node_graph [n_nodes]), their
 * n_edges edges src[e] -> dst[e] concatenated in the same graph order (edge_ptr [n_graphs + 1]; both ends of an edge in
 * one graph), and per node the incidence list inc(v) = inc_edge / inc_other [inc_ptr[v], inc_ptr[v + 1]): (edge, other
 * end) of every directed edge ARRIVING at v.  undirected = 1: every edge counts in both directions, so it stands in
 * the lists of both its ends (a self-loop twice in one list) and n_inc = 2 n_edges; undirected = 0: in the list of its
 * destination only, n_inc = n_edges, and out_ptr / out_edge / out_other list the edges LEAVING each node the same way
 * (NULL when undirected).  All int32.  The kernel entries take a description whose arrays are on the DEVICE and check
 * sizes and pointers only; the kernels compare every index they read with those sizes before using it.
 * gcmi_gn_graph_check follows a description whose arrays are on the HOST and validates everything above: call it once
 * per batch on the arrays that are uploaded.
 * Rows (Ps, Pd: n_nodes; Q: n_edges; R: n_graphs; and what the entries write) are GCMI_GN_WIDTH = 32 floats with a
 * leading dimension that is a multiple of 4, 16-byte aligned; Ps and Pd share ldp (two column blocks of one product).
 *   gcmi_gn_edge_fwd   Hs[e] = Q[e] + R[g] + (Ps[s] + Pd[d])  (directed),
 *                      Hs[e] = Q[e] + R[g] + ((Ps[s] + Pd[d]) + (Ps[d] + Pd[s])) / 2  (undirected)
 *   gcmi_gn_node_fwd   Mh[v] = Pd[v] + R[g] + (sum over inc(v) of (Ps[other] + Q[edge])) / |inc(v)|, a zero row where
 *                      inc(v) is empty
 *   gcmi_gn_edge_bwd   from dHs: dPs, dPd (two distinct buffers, every row written) and dR; dQ is dHs itself
 *   gcmi_gn_node_bwd   from dMh (rows of nodes with an empty list are ignored): dQ, dPs, dPd, dR, every row written
 *   gcmi_gn_seg_reduce out[s] = the sum (mean = 0) or mean (mean = 1) of rows [ptr[s], ptr[s + 1]) of x, any width
 *                      >= 1; a zero row for an empty range
 *   gcmi_gn_seg_spread its transpose: out[r] = x[s] (mean = 1: / count) for the rows r of range s; ptr must cover
 *                      [0, n_rows] for every row to be written
 * No atomics: two calls agree bit for bit.  n_edges = 0 is allowed (edge rows and lists may then be NULL).        */
#define GCMI_GN_WIDTH 32
#define GCMI_GN_ROWS_PER_WG 32
typedef struct gcmi_gn_graph {
  int32_t n_nodes, n_edges, n_graphs, undirected, n_inc;
  const int32_t *src, *dst;              /* [n_edges] */
  const int32_t* node_graph;             /* [n_nodes] */
  const int32_t *node_ptr, *edge_ptr;    /* [n_graphs + 1] */
  const int32_t *inc_ptr;                /* [n_nodes + 1] */
  const int32_t *inc_edge, *inc_other;   /* [n_inc] */
  const int32_t *out_ptr;                /* [n_nodes + 1], directed only */
  const int32_t *out_edge, *out_other;   /* [n_edges], directed only */
} gcmi_gn_graph;
int gcmi_gn_graph_check(const gcmi_gn_graph* host_graph);
int gcmi_gn_edge_fwd(const gcmi_gn_graph* g, const float* d_ps, const float* d_pd, int64_t ldp, const float* d_q, int64_t ldq,
                     const float* d_r, int64_t ldr, float* d_hs, int64_t ldh, void* stream);
int gcmi_gn_node_fwd(const gcmi_gn_graph* g, const float* d_ps, const float* d_pd, int64_t ldp, const float* d_q, int64_t ldq,
                     const float* d_r, int64_t ldr, float* d_mh, int64_t ldm, void* stream);
int gcmi_gn_edge_bwd(const gcmi_gn_graph* g, const float* d_dhs, int64_t ldh, float* d_dps, float* d_dpd, int64_t ldp,
                     float* d_dr, int64_t ldr, void* stream);
int gcmi_gn_node_bwd(const gcmi_gn_graph* g, const float* d_dmh, int64_t ldm, float* d_dq, int64_t ldq, float* d_dps,
                     float* d_dpd, int64_t ldp, float* d_dr, int64_t ldr, void* stream);
int gcmi_gn_seg_reduce(const int32_t* d_ptr, int32_t n_seg, int32_t n_rows, int32_t width, int32_t mean, const float* d_x,
                       int64_t ldx, float* d_out, int64_t ldo, void* stream);
int gcmi_gn_seg_spread(const int32_t* d_ptr, int32_t n_seg, int32_t n_rows, int32_t width, int32_t mean, const float* d_x,
                       int64_t ldx, float* d_out, int64_t ldo, void* stream);

/* ---------------------------------------------------------------- D-MPNN (dmpnn.hip)
 * The message aggregation of the directed message-passing network (deepchem/models/torch_models/layers.py:1629,
 * `message[mapping].sum(1)`, and :1539, `h_message[atom_to_incoming_bonds].sum(1)`) over a batch whose directed bonds
 * are sorted by SOURCE atom.  d_out_ptr [n_atoms + 1]: the outgoing bonds of atom a are the run
 * R(a) = [out_ptr[a], out_ptr[a+1]); d_rev [n_bonds]: the position of the reverse bond, an involution without fixed
 * points (the bonds arriving at a are rev[b], b in R(a)).  Both must have been validated by the caller; the kernel skips
 * rows outside [0, n_bonds).  Rows are float32 with ld >= d, any d >= 1 (16-byte aligned rows of whole 16-byte pieces
 * take the vector path, anything 4-byte aligned the scalar one).
 *   transposed = 0:  S[a] = sum_{b in R(a)} x[rev[b]]  -> d_s [n_atoms x d] (optional);
 *                    q[b] = S[a] - x[rev[b]]           -> d_q [n_bonds x d] (optional).  d_add must be NULL.
 *   transposed = 1:  the adjoint.  T[a] = sum_{b in R(a)} x[b] -> d_s (optional);
 *                    q[rev[b]] = T[a] - x[b] + add[a]  -> d_q (optional): every bond row is written exactly once, no
 *                    atomics.  d_x (the gradient of q) or d_add (the gradient of S, [n_atoms x d]) may be NULL = zeros.
 * d_q must not be d_x.  An atom without bonds gets a zero d_s row and nothing else; n_bonds == 0 launches no kernel
 * (d_s is cleared).  NULL pointers, ld < d and buffers off a 4-byte boundary: GCMI_ERR_ARG before any launch.  */
int gcmi_dmpnn_message(int32_t transposed, const float* d_x, int64_t ldx, int32_t d, const int32_t* d_out_ptr,
                       const int32_t* d_rev, int32_t n_atoms, int32_t n_bonds, const float* d_add, int64_t ldadd,
                       float* d_s, int64_t lds, float* d_q, int64_t ldq, void* stream);
/* The fused bond update of a message-passing round, forward only:
 *     h[b] = act( input[b] + (S[a] - x[rev[b]]) . W^T ),   a = d_bond_src[b], act 0 none / 1 ReLU,
 * with d_w [d_hidden x d_hidden] in nn.Linear layout (out x in, leading dimension ldw).  The aggregated rows are built
 * in LDS as the A operand of the product and never written to memory; the product is the six-product split-bf16 on
 * v_mfma_f32_32x32x16_bf16, float32 accuracy.  1 <= d_hidden <= 320 (zero-padded to the tile); above: GCMI_ERR_UNSUPPORTED
 * with an error text -- no other kernel stands behind this entry.  d_bond_src [n_bonds]: the source atom of every bond
 * (non-decreasing, consistent with d_out_ptr); every atom's degree must be at most 32 (validated by the caller).
 * d_img_scratch: 16-byte aligned, scratch_floats >= ceil(d/16) * ceil(d/32) * 768 floats; it receives the split image of
 * d_w, rebuilt by every call.  d_h may be d_input, not d_x.  NULL pointers, ld < d_hidden, misaligned buffers and a short
 * scratch: GCMI_ERR_ARG before any launch; n_bonds == 0 launches nothing.                                             */
int gcmi_dmpnn_update_fwd(const float* d_x, int64_t ldx, const float* d_input, int64_t ldi, const float* d_w, int64_t ldw,
                          int32_t d_hidden, int32_t act, const int32_t* d_out_ptr, const int32_t* d_rev,
                          const int32_t* d_bond_src, int32_t n_atoms, int32_t n_bonds, float* d_img_scratch,
                          int64_t scratch_floats, float* d_h, int64_t ldh, void* stream);

/* ---------------------------------------------------------------- D-MPNN batch collation (dmpnn_collate.hip)
 * A batch of the D-MPNN kernels above, gathered on the device from a graph set that stays in device memory.  The set,
 * M = n_mols_all molecules with A atoms and B directed bonds in all: d_atom_ptr, d_bond_ptr [M + 1]; d_atom_features
 * [A x atom_fdim]; d_bond_features [B x bond_fdim] with the bonds of every molecule stably sorted by source atom;
 * d_sorted_src [B] the source atom and d_sorted_rev [B] the position of the reverse bond, both local to the molecule;
 * d_out_start [A]: where the atom's run of outgoing bonds begins, relative to the molecule's first bond;
 * d_global_features [M x global_fdim].  d_plan: int32 words [mol_idx (n_mols) ; atom_off (n_mols + 1) ; bond_off
 * (n_mols + 1)], the offsets being the exclusive prefix sums of the selected molecules' atom and bond counts, totals
 * last (= n_atoms, n_bonds).
 * d_out receives nine blocks of 4-byte words, each starting at a 16-byte boundary, pad words zero:
 *   mol_ptr (n_mols + 1), out_ptr (n_atoms + 1), bond_src (n_bonds), rev (n_bonds), atom_membership (n_atoms),
 *   atoms_per_mol (n_mols, float), atom_features (n_atoms x atom_fdim), f_ini_atoms_bonds (n_bonds x (atom_fdim +
 *   bond_fdim): [features of the source atom ; bond features]), global_features (n_mols x global_fdim).
 * gcmi_dmpnn_collate_words returns the words of that buffer and, with offsets != NULL, the nine block offsets (-1: a
 * negative size).  Every word is written exactly once, pad words included; no atomics.  A molecule index outside
 * [0, M), or a molecule that would not fit the totals, is skipped and not read through (its words stay unwritten: the
 * caller validates the indices).  NULL pointers, negative sizes, misaligned buffers and out_words below the layout's:
 * GCMI_ERR_ARG before any launch.
 * gcmi_dmpnn_collate_host: the same routine run by host loops over host buffers, for tests without a GPU.           */
int64_t gcmi_dmpnn_collate_words(int32_t n_mols, int32_t n_atoms, int32_t n_bonds, int32_t atom_fdim, int32_t bond_fdim,
                                 int32_t global_fdim, int64_t* offsets);
int gcmi_dmpnn_collate(const int64_t* d_atom_ptr, const int64_t* d_bond_ptr, const float* d_atom_features,
                       const float* d_bond_features, const int32_t* d_sorted_src, const int32_t* d_sorted_rev,
                       const int32_t* d_out_start, const float* d_global_features, int64_t n_mols_all,
                       int32_t atom_fdim, int32_t bond_fdim, int32_t global_fdim, const int32_t* d_plan, int32_t n_mols,
                       int32_t n_atoms, int32_t n_bonds, int32_t* d_out, int64_t out_words, void* stream);
int gcmi_dmpnn_collate_host(const int64_t* atom_ptr, const int64_t* bond_ptr, const float* atom_features,
                            const float* bond_features, const int32_t* sorted_src, const int32_t* sorted_rev,
                            const int32_t* out_start, const float* global_features, int64_t n_mols_all, int32_t atom_fdim,
                            int32_t bond_fdim, int32_t global_fdim, const int32_t* plan, int32_t n_mols, int32_t n_atoms,
                            int32_t n_bonds, int32_t* out, int64_t out_words);

/* ---------------------------------------------------------------- MEGNet batch collation (megnet_collate.hip)
 * A batch of the graph-network kernels above (the int32 lists of gcmi_gn_graph plus the three feature arrays), gathered
 * on the device from a graph set that stays in device memory.  The set, n_graphs = M graphs with N nodes and E edges in
 * all, k = 2 (undirected) or 1: node_ptr, edge_ptr [M + 1]; node_features [N x fn]; edge_features [E x fe];
 * global_features [M x fg]; src, dst [E] LOCAL to the graph; inc_start [N]: where the node's incidence list begins,
 * relative to the graph's first entry; inc_edge, inc_other [k E] local, the entries of graph g at [k edge_ptr[g],
 * k edge_ptr[g + 1]); directed only: out_start [N], out_edge, out_other [E], the same for the edges LEAVING a node.
 * d_plan: int32 words [graph_idx (n_graphs) ; node_off (n_graphs + 1) ; edge_off (n_graphs + 1)], the offsets being the
 * exclusive prefix sums of the selected graphs' node and edge counts, totals last (= n_nodes, n_edges).
 * d_out receives blocks of 4-byte words, each starting at a 16-byte boundary, pad words zero: the int32 blocks src, dst
 * (n_edges), node_graph (n_nodes), node_ptr, edge_ptr (n_graphs + 1), inc_ptr (n_nodes + 1), inc_edge, inc_other
 * (k n_edges), directed only out_ptr (n_nodes + 1), out_edge, out_other (n_edges), then the float blocks x (n_nodes x
 * fn), edge_attr (n_edges x fe), global_features (n_graphs x fg).
 * gcmi_gn_collate_words returns the words of that buffer and, with offsets != NULL, the GCMI_GN_COLLATE_BLOCKS block
 * offsets in that order, -1 for a block the mode lacks (-1 returned: a negative size).  Every word is written exactly
 * once, pad words included; no atomics.  A graph index outside [0, M), or a graph that would not fit the totals, is
 * skipped and not read through (its words stay unwritten: the caller validates the indices).  NULL pointers, negative
 * sizes, n_graphs < 1, misaligned buffers, an output that is not 16-byte aligned and out_words other than the layout's:
 * GCMI_ERR_ARG before any launch.
 * gcmi_gn_collate_host: the same routine run by host loops over host buffers, for tests without a GPU.             */
#define GCMI_GN_COLLATE_BLOCKS 14
typedef struct gcmi_gn_set {
  int64_t n_graphs;
  int32_t undirected, fn, fe, fg;
  const int64_t *node_ptr, *edge_ptr;
  const float *node_features, *edge_features, *global_features;
  const int32_t *src, *dst, *inc_start, *inc_edge, *inc_other;
  const int32_t *out_start, *out_edge, *out_other; /* directed only */
} gcmi_gn_set;
int64_t gcmi_gn_collate_words(int32_t n_graphs, int32_t n_nodes, int32_t n_edges, int32_t undirected, int32_t fn,
                              int32_t fe, int32_t fg, int64_t* offsets);
int gcmi_gn_collate(const gcmi_gn_set* set, const int32_t* d_plan, int32_t n_graphs, int32_t n_nodes, int32_t n_edges,
                    int32_t* d_out, int64_t out_words, void* stream);
int gcmi_gn_collate_host(const gcmi_gn_set* set, const int32_t* plan, int32_t n_graphs, int32_t n_nodes, int32_t n_edges,
                         int32_t* out, int64_t out_words);

/* ---------------------------------------------------------------- crystal-graph convolution of CGCNN (cgcnn.hip)
 * One CGCNNLayer between its two products, over a DIRECTED gcmi_gn_graph on the device (undirected = 0; the arriving
 * list inc_* and the leaving list out_*).  H = the hidden width, a multiple of 4 in [GCMI_CG_MIN_WIDTH,
 * GCMI_CG_MAX_WIDTH].  With linear.weight split by columns into A_s | A_d | C:
 *     Ps = h A_s^T, Pd = h A_d^T (n_nodes rows of 2H floats, two column blocks of one product: they share ldp),
 *     Q = e C^T + b (n_edges rows of 2H floats),      z[k] = (Ps[src k] + Pd[dst k]) + Q[k]   -- never stored.
 * Columns [0, H) of such a row are the gate half, [H, 2H) the message half.  The normalisation is
 *     xhat = (z - mean) * invstd,  zh = xhat * gamma + beta      (vectors of 2H floats; NULL: 0, 1, 1, 0),
 * the message m[k] = sigmoid(zh[k, :H]) * softplus(zh[k, H:]) and the new row
 *     h'[v] = softplus(h[v] + sum over inc(v) of m[edge]),  a ZERO row where inc(v) is empty,
 * softplus with beta 1 and threshold 20.  Every row pointer is 16-byte aligned with a leading dimension that is a
 * multiple of 4 and at least the row's width; vectors are 16-byte aligned.
 *   gcmi_cg_stats      mean and invstd = 1 / sqrt(biased variance + eps) of the columns of z over the n_edges >= 2
 *                      rows: per-workgroup moments about a pivot row in double, combined in double in a fixed order.  With
 *                      running_mean / running_var (optional, both or neither): r = (1 - momentum) r + momentum * (mean |
 *                      unbiased variance); batches_tracked (optional, int64) is incremented.
 *   gcmi_cg_conv_fwd   h' from h with the given normalisation (training: what gcmi_cg_stats wrote; eval: the running
 *                      statistics).  n_edges = 0 is allowed.
 *   gcmi_cg_bwd_stats  with dpre[v] = dh'[v] * sigmoid(h[v] + S[v]) recovered from h' itself (1 - exp(-h'); 0 for an
 *                      empty list): sums = [sum of dzh (2H) | sum of dzh * xhat (2H)] over the edges, which are dbeta
 *                      and dgamma.  n_edges >= 1.
 *   gcmi_cg_bwd_edges  dQ[k] = dz[k], dPd[v] = sum over inc(v) of dz, dpre[v] (n_nodes rows of H floats: the gradient
 *                      of h through the residual).  sums != NULL (training): dz = gamma invstd (dzh - sums_0 / E - xhat
 *                      sums_1 / E); sums == NULL (eval, or no normalisation): dz = gamma invstd dzh.
 *   gcmi_cg_bwd_src    dPs[v] = sum over out(v) of dQ[edge].
 * The two statistics entries take a workspace of gcmi_cg_workspace_floats(n_nodes, n_edges, H) floats.  No atomics;
 * every sum runs in list order or in an order the sizes alone fix: two calls agree bit for bit.                                     */
#define GCMI_CG_MIN_WIDTH 4
#define GCMI_CG_MAX_WIDTH 128
int64_t gcmi_cg_workspace_floats(int32_t n_nodes, int32_t n_edges, int32_t H);
int gcmi_cg_stats(const gcmi_gn_graph* g, const float* d_ps, const float* d_pd, int64_t ldp, const float* d_q, int64_t ldq,
                  int32_t H, float eps, float momentum, float* d_mean, float* d_invstd, float* d_running_mean,
                  float* d_running_var, int64_t* d_batches_tracked, float* d_workspace, int64_t workspace_floats,
                  void* stream);
int gcmi_cg_conv_fwd(const gcmi_gn_graph* g, const float* d_ps, const float* d_pd, int64_t ldp, const float* d_q,
                     int64_t ldq, int32_t H, const float* d_mean, const float* d_invstd, const float* d_gamma,
                     const float* d_beta, const float* d_h, int64_t ldh, float* d_out, int64_t ldo, void* stream);
int gcmi_cg_bwd_stats(const gcmi_gn_graph* g, const float* d_ps, const float* d_pd, int64_t ldp, const float* d_q,
                      int64_t ldq, int32_t H, const float* d_mean, const float* d_invstd, const float* d_gamma,
                      const float* d_beta, const float* d_hnew, int64_t ldhn, const float* d_dhnew, int64_t lddh,
                      float* d_sums, float* d_workspace, int64_t workspace_floats, void* stream);
int gcmi_cg_bwd_edges(const gcmi_gn_graph* g, const float* d_ps, const float* d_pd, int64_t ldp, const float* d_q,
                      int64_t ldq, int32_t H, const float* d_mean, const float* d_invstd, const float* d_gamma,
                      const float* d_beta, const float* d_hnew, int64_t ldhn, const float* d_dhnew, int64_t lddh,
                      const float* d_sums, float* d_dq, int64_t lddq, float* d_dpd, int64_t lddp, float* d_dpre,
                      int64_t lddpre, void* stream);
int gcmi_cg_bwd_src(const gcmi_gn_graph* g, const float* d_dq, int64_t lddq, int32_t H, float* d_dps, int64_t lddp,
                    void* stream);

/* ---------------------------------------------------------------- lattice convolution of LCNN (lcnn.hip)
 * One LCNNBlock behind its one product, fp32.  n_sites sites with P permutations of K neighbour slots each; O = the
 * output width.  With conv_weights.weight (O, K * F) split by slot into K blocks W_j (O, F):
 *     Y = x [W_0; ...; W_{K-1}]^T   (n_sites rows of K * O floats, leading dimension ldy),
 *     X[v, p, :] = bias + sum over j in order of Y[nbr[v, p, j], j, :]           (n_sites, P, O), contiguous,
 *     xhat = (X - mean) / sqrt(var + eps);  mean == var == NULL (training): per site and channel, the mean and the
 *            biased variance over the P rows;  otherwise (eval) the given vectors of O floats, the root in double,
 *     out[v, :] = sum over p of mask[v, p] * (xhat[v, p, :] * gamma + beta)     mask (n_sites, P), NULL: ones.
 * Limits: O in [1, GCMI_LC_MAX_WIDTH], P in [GCMI_LC_MIN_PERM, GCMI_LC_MAX_PERM], K in [1, GCMI_LC_MAX_SLOTS],
 * n_sites * P * K * GCMI_LC_MAX_WIDTH < 2^31.  Every pointer is 4-byte aligned (one channel per lane: no wider access), the
 * workspace 16-byte.  An index of nbr outside [0, n_sites) or of rev_row outside [0, n_sites * P) is compared with
 * the size before it is used and contributes nothing.
 *   gcmi_lc_site_fwd  out, and X when d_x != NULL (the backward and gcmi_lc_running read it).
 *   gcmi_lc_site_bwd  dX (n_sites, P, O) from X, dOut, mask, gamma: training, the BatchNorm backward over the P rows of
 *                     each site; eval, dX = mask dOut gamma / sqrt(var + eps).  sums[3 O] = [dgamma | dbeta | dbias], summed per
 *                     workgroup in double in row order, the workgroups in double by a fixed tree (eval: dbias is
 *                     gamma / sqrt(var + eps) times dbeta in double, not the sum of the rounded dX).  Workspace:
 *                     gcmi_lc_workspace_floats(n_sites, O) floats (-1: bad sizes).
 *   gcmi_lc_rev_sum   dY[u, j, :] = the sum of dX[rev_row[k], :] for k in [rev_ptr[u K + j], rev_ptr[u K + j + 1]) in
 *                     that order: the (v, p) with nbr[v, p, j] = u as rows v P + p.  A zero row for an empty list.
 *   gcmi_lc_running   the running statistics after one update per site in site order, r <- (1 - m) r + m s_v with s_v
 *                     the mean / the UNBIASED variance of site v, in closed form: r = (1 - m)^N r + m sum_v
 *                     (1 - m)^(N - 1 - v) s_v with weights and sums in double in a fixed order, over the last 2048
 *                     sites (the rest cannot reach a float32 result for m >= 0.1, which the entry requires);
 *                     batches_tracked (optional, int64) += n_sites.
 * No atomics: two calls agree bit for bit.                                                                             */
#define GCMI_LC_MAX_WIDTH 64
#define GCMI_LC_MIN_PERM 2
#define GCMI_LC_MAX_PERM 8
#define GCMI_LC_MAX_SLOTS 32
typedef struct {
  int32_t n_sites, P, K, O;
  const int32_t* nbr;     /* (n_sites, P * K) */
  const int32_t* rev_ptr; /* n_sites * K + 1 */
  const int32_t* rev_row; /* n_sites * P * K */
} gcmi_lc_batch;
int64_t gcmi_lc_workspace_floats(int32_t n_sites, int32_t O);
int gcmi_lc_site_fwd(const gcmi_lc_batch* b, const float* d_y, int64_t ldy, const float* d_bias, const float* d_gamma,
                     const float* d_beta, const float* d_mean, const float* d_var, float eps, const float* d_mask,
                     float* d_out, int64_t ldo, float* d_x, void* stream);
int gcmi_lc_site_bwd(const gcmi_lc_batch* b, const float* d_x, const float* d_dout, int64_t lddo, const float* d_mask,
                     const float* d_gamma, const float* d_mean, const float* d_var, float eps, float* d_dx, float* d_sums,
                     float* d_workspace, int64_t workspace_floats, void* stream);
int gcmi_lc_rev_sum(const gcmi_lc_batch* b, const float* d_dx, float* d_dy, int64_t lddy, void* stream);
int gcmi_lc_running(const gcmi_lc_batch* b, const float* d_x, float momentum, float* d_running_mean, float* d_running_var,
                    int64_t* d_batches_tracked, void* stream);

/* ---------------------------------------------------------------- atomic convolution of ACNN (atomconv.hip)
 * The whole AtomicConvolution layer over B samples of N atom slots with M neighbours each, d = 3 coordinates, fp32.
 *     D[m] = x[b, nbrs[b, n, m]] - x[b, n],  with has_box: D -= rint(D / box) * box (half to even),  R[m] = |D[m]|,
 *     rsf(R, l) = exp(-re[l] (R - rs[l])^2) * (R <= rc[l] ? 0.5 (cos(pi R / rc[l]) + 1) : 0),
 *     row[b, n, a L + l] = sum over the m with z[b, n, m] == types[a] of rsf(R[m], l)        (n_types > 0),
 *     row[b, n, l]       = sum over the m with z[b, n, m] != 0 of rsf(R[m], l)               (n_types == 0),
 *     y[b, n, c] = (row[b, n, c] - mean[n]) * invstd[n],   C = max(n_types, 1) * L channels,
 * mean[n] and the UNBIASED variance of slot n over its B * C values, invstd = 1 / sqrt(variance + eps); stats[n] =
 * (mean[n], invstd[n]), N pairs of floats, 8-byte aligned.  The statistics are constants of the backward, and x takes
 * no gradient.  A neighbour whose distance is NaN makes its whole row NaN.  Limits: M <= GCMI_AC_MAX_NEIGHBORS (one lane per neighbour),
 * n_types <= GCMI_AC_MAX_TYPES without duplicates (the table travels by value), C <= GCMI_AC_MAX_CHANNELS (a row is
 * held in LDS, four rows per workgroup).  An index nbrs[b, n, m] outside [0, N) is compared with N before it is used
 * and contributes nothing.  All arrays are contiguous and 4-byte aligned.
 *   gcmi_ac_stats  stats; B * C >= 2.  Per row a mean and a centred second moment in double about the
 *                  row's first value, combined over b in index order in double.  The rows are not written.
 *   gcmi_ac_fwd    y (B, N, C).
 *   gcmi_ac_bwd    grad[3 L] = [d rc | d rs | d re], the sums over b, n, m, a of dy[b, n, a L + l] * invstd[n] *
 *                  d rsf / d{rc, rs, re}, per workgroup in double in row order, the workgroups by a fixed tree.
 * gcmi_ac_stats and gcmi_ac_bwd take a 16-byte aligned workspace of gcmi_ac_workspace_floats(B, N, L) floats (-1: bad
 * sizes).  No atomics: two calls agree bit for bit.                                                                    */
#define GCMI_AC_MAX_NEIGHBORS 64
#define GCMI_AC_MAX_TYPES 32
#define GCMI_AC_MAX_CHANNELS 2048
typedef struct {
  const float* x;       /* (B, N, 3) */
  const int32_t* nbrs;  /* (B, N, M) */
  const float* z;       /* (B, N, M): the type of each neighbour */
  const float *rc, *rs, *re; /* L each */
  int32_t B, N, M, d, L;
  int32_t n_types;
  float types[GCMI_AC_MAX_TYPES];
  int32_t has_box;
  float box[3];
} gcmi_ac_input;
int64_t gcmi_ac_workspace_floats(int32_t B, int32_t N, int32_t L);
int gcmi_ac_stats(const gcmi_ac_input* in, float eps, float* d_stats, float* d_workspace, int64_t workspace_floats,
                  void* stream);
int gcmi_ac_fwd(const gcmi_ac_input* in, const float* d_stats, float* d_out, void* stream);
int gcmi_ac_bwd(const gcmi_ac_input* in, const float* d_stats, const float* d_dy, float* d_grad, float* d_workspace,
                int64_t workspace_floats, void* stream);

/* ---------------------------------------------------------------- measurement
 * Optional per-kernel timing with hipEvents recorded on `stream` around the
 * launches of one kernel family (bench.py roofline).  id: see GCMI_K_*.       */
enum {
  GCMI_K_GATHER_SUM = 0,
  GCMI_K_GATHER_MAX = 1,
  GCMI_K_READOUT = 2,
  GCMI_K_SEG_GEMM = 3,
  GCMI_K_WGRAD = 4,
  GCMI_K_GATHER_MAX_BWD = 5,
  GCMI_K_BATCHNORM = 6, /* column sums, finalize, backward (statistics and dx) */
  GCMI_K_FUSED_BWD = 7, /* the one-pass backward of a GraphConv / dense block (bwd_fused.hip) */
  GCMI_K_COUNT = 8
};
int gcmi_timing_enable(int32_t kernel_id, int32_t on);
/* Diagnostic: `blocks` workgroups of 4 waves each issue iters*32 register-only
 * v_mfma_f32_32x32x2_f32 per wave (4096 flops each): the fp32 MFMA ceiling of the device.  */
int gcmi_diag_mfma_peak(int32_t blocks, int32_t iters, float* d_out, void* stream);
/* Synchronises the recorded events; returns launches and total milliseconds. */
int gcmi_timing_read(int32_t kernel_id, int64_t* n_launches, double* total_ms, int32_t reset);

#ifdef __cplusplus
}
#endif
#endif /* GCMI_H */
