/* hidenn_fem.h -- C ABI of libhidenn_hip.so (MI355X / gfx950 HIP kernels for the
 * HiDeNN-FEM element-evaluation + energy hot path).
 *
 * The reference (achraf-15/HiDeNN-FEM) is pure Python/PyTorch and has no FFI of
 * its own; the boundary below is what a ctypes binding inside the reference's
 * src/models.py / src/loss.py would call instead of its ATen op chains.  Each
 * entry point cites the reference code it replaces (paths are relative to the
 * reference repo root).
 *
 * Conventions
 *   - plain pointers and sizes only; every device buffer is allocated and owned
 *     by the caller (torch tensors on the ROCm device), contiguous, 16-B aligned;
 *   - every call takes the device ordinal and a hipStream_t (as void*); work is
 *     enqueued on that stream, nothing synchronises, results are stream-ordered;
 *   - return 0 = ok, <0 = argument error, >0 = hipError_t; message via
 *     hfem_last_error() (thread-local).  No exceptions, no exit();
 *   - degenerate elements are not errors: divisions by a tiny det / clamp(1e-10)
 *     spans behave as in the reference and NaN/Inf propagate;
 *   - dtype: fp64 (the parity contract of BASELINE.md);
 *   - no thread-affine state: PyTorch runs backward on another thread.
 */
#ifndef HIDENN_FEM_H
#define HIDENN_FEM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HFEM_VERSION 114   /* 0.1.1: round 4 -- plan blobs, sharded L-BFGS, fp32 arithmetic; append-only since 113 */

int hfem_version(void);
const char *hfem_last_error(void);
/* number of HIP devices visible, or -1 (used by the loader to fail loudly) */
int hfem_device_count(void);

/* ------------------------------------------------------------------ TRI3 + EDGE2
 * Plane-stress material: mat = {c11, c12, c22, c33} of C (src/loss.py:29-32).
 * W  = sum_q w_q of the triangle rule (src/utils.py:13-81; 0.25 for the default
 *      gauss_order=4).
 * Bk = [3][2] body-force table  B_k = sum_q w_q N_k(xi_q) b(xi_q), b evaluated
 *      at the REFERENCE points as src/loss.py:80 does (zeros by default).
 * Traction: Tconst[4] = {c_i t, c_j t} with c_i = sum_q w_q (1-xi_q), c_j = sum_q
 *      w_q xi_q over the raw Legendre nodes (src/loss.py:96-110), or a
 *      per-edge table T[Ned][4] = {T_i, T_j} when t depends on the point.      */

/* Planless variant: element-parallel, fp64 global atomics.  Replaces
 * EnergyLoss2D.domain_energy + its autograd backward (src/loss.py:55-88,
 * src/models.py:316-357) on ASSEMBLED arrays X,U [Nn][2].
 * ACCUMULATES: loss_acc[0] += E_domain, gX += dE/dX, gU += dE/dU (caller zeroes).
 * gX/gU may be NULL (forward only).  Elements [e_begin, e_end); an empty range
 * (here, ned == 0 below, and for hfem_quad4_energy_atomic) returns 0 and reads
 * no pointer.                                                                 */
int hfem_tri3_energy_atomic(int device, const double *X, const double *U,
                            const int32_t *conn, int64_t e_begin, int64_t e_end, int64_t nn,
                            const double mat[4], double W, const double Bk[6],
                            double *loss_acc, double *gX, double *gU, void *stream);

/* Planless Neumann-edge work; replaces EnergyLoss2D.edge_energy + backward
 * (src/loss.py:91-110, src/models.py:359-376).  ACCUMULATES the NEGATIVE work:
 * loss_acc[0] -= sum ds*m, gX/gU += d(-work).  edges [Ned][2] int32, i<j.     */
int hfem_edge2_energy_atomic(int device, const double *X, const double *U,
                             const int32_t *edges, int64_t ned, const double *T,
                             const double Tconst[4], double *loss_acc, double *gX,
                             double *gU, void *stream);

/* Planned variant -- the fast path.  A plan is an owner-computes tiling of the
 * mesh (host-side preprocessing, once per mesh): elements are sorted along a
 * Hilbert curve of their centroids and cut into tiles; every node is owned by
 * exactly one tile; a tile evaluates its home elements plus the halo elements
 * that touch its owned nodes, with node data staged in LDS and gradients
 * accumulated in LDS, so each gradient row is written exactly once with a plain
 * store (no global atomics, no zero fill).  TRI3 plans whose elements pair up
 * along shared fan edges (about 62 % of them or more: structured splits with fixed or random diagonals)
 * store two elements per slot, A = (n,b,c) and B = (n,c,d), each in its own
 * local node order, and run the paired-slot kernel (16 instead of 24 LDS
 * atomics per pair); other meshes keep one element per slot.  The choice is
 * made at plan creation ("plan_elem_order" -1 = auto) and is invisible in the
 * results up to fp64 summation order.
 *
 * It also fuses the free/fixed parameter assembly of src/models.py:292-305:
 *   x_src[n] >= 0 -> coords of node n = x_free[x_src[n]]   (node_coords_free row)
 *   x_src[n] <  0 -> coords of node n = x_fixed[-1-x_src[n]]
 *   u_src likewise for u_free / u_fixed rows (Dirichlet rows).
 * NULL maps mean identity (x_free = X, u_free = U are the full arrays).
 * coords_hint [Nn][2] (host) is only used for the locality sort.
 * device < 0 builds a host-only plan (no HIP call; for CPU tests).            */
typedef struct hfem_plan hfem_plan;

typedef struct hfem_plan_stats {
    int64_t n_elems, n_nodes, n_edges;
    int32_t n_tiles, tile_elems;          /* home elements per tile */
    int64_t tile_elem_total;              /* home + halo elements over all tiles */
    int64_t tile_node_total;              /* owned + halo local nodes over all tiles */
    int32_t max_tile_nodes, max_tile_owned, max_tile_elems, max_tile_edges;
    int64_t device_bytes;                 /* plan arrays resident in HBM */
    int32_t lds_bytes;                    /* dynamic LDS per workgroup */
    int32_t shards;                       /* ranks the tile order was prepared for ("plan_shards"; 1 = not sharded) */
    int32_t threads_per_tile;             /* workgroup size of the tiled kernel this plan takes */
    int32_t paired;                       /* 1: paired slots (two fan-adjacent TRI3 per slot) */
    int32_t slot_rows;                    /* paired plans: slots per thread in the widest tile */
    int32_t store_policy;                 /* gradient stores of this plan: 16 sc1 write-through, 2 nt (meshes of >= 750 k nodes
                                             whose rows have locality), 0 plain -- "store_policy" -1 = this choice */
    int32_t nodes_per_elem;               /* 3 (TRI3) or 4 (QUAD4) -- was reserved0 before version 114 */
    double row_line_factor;               /* distinct 128-byte lines among a tile's coordinate rows / the minimum, mean over the
                                             tiles: ~1.3 = rows stored with locality, up to 8 = random numbering */
} hfem_plan_stats;

int hfem_plan_create(int device, const int64_t *conn, int64_t ne, int64_t nn,
                     const double *coords_hint, const int32_t *x_src, const int32_t *u_src,
                     const int64_t *edges, int64_t ned, int32_t tile_elems,
                     hfem_plan **out);
/* Same with an explicit element type: nodes_per_elem = 3 (TRI3, conn [Ne][3]) or 4 (QUAD4 extension,
 * conn [Ne][4], local nodes CCW).                                                          */
int hfem_plan_create_ex(int device, const int64_t *conn, int64_t ne, int64_t nn, int32_t nodes_per_elem,
                        const double *coords_hint, const int32_t *x_src, const int32_t *u_src,
                        const int64_t *edges, int64_t ned, int32_t tile_elems, hfem_plan **out);
int hfem_plan_destroy(hfem_plan *plan);
int hfem_plan_get_stats(const hfem_plan *plan, hfem_plan_stats *out);
/* Copy a host-side plan array out (for tests).  which: 0 tile_desc [n_tiles][8]
 * i32, 1 elem_pack u32, 2 node_src [.][2] i32, 3 edge_pack u32, 4 edge_gid i32,
 * 5 elem_gid i32 (global element id of every slot's element A; -1 = padding), 6 lab stamps
 * (lab build only), 7 elem_pack_hi u32 (QUAD4 plans: 4th local node of every slot; paired TRI3
 * plans: node d + presence/home bits of element B), 8 tile_chunks (chunked lab order), 9 elem_gid_b
 * i32 (paired plans: global id of every slot's element B; -1 = none), 10 shard_desc [shards][4] i32 = {tile_lo,
 * tile_mid, tile_hi, 0} per rank: the rank's boundary tiles are [tile_lo, tile_mid), its interior tiles [tile_mid, tile_hi),
 * 11 owned_node_ids [Nn] i32: the global node id of every tile's owned nodes in (tile, local) order -- a permutation of the
 * nodes; a caller that stores its parameter rows in THIS order gives every tile one contiguous run of rows (full-line
 * gradient stores, perfectly coalesced gathers).
 * Returns the element count, or <0.  buf may be NULL to query the size.  The per-tile arrays are laid out
 * with uniform strides (tile t's node records start at t * node_stride, its slot records at t * elem_stride, padded;
 * extra records follow the last tile): walk them through tile_desc's offsets and counts, not as dense arrays.    */
int64_t hfem_plan_export(const hfem_plan *plan, int which, void *buf, int64_t cap_elems);

/* A plan as one relocatable byte string: the planner costs ~1 s per 10^6 elements and every rank of a multi-GPU job (and
 * every later run on the same mesh) needs the same plan -- one process builds and serialises, the others deserialise
 * (hidenn_fem_amd/plan.py: TilePlan.to_bytes / from_bytes / the cache_dir of TilePlan and bench.py --gpus N).  The blob
 * holds the host plan, the creation-time decisions (element order, tile shape, store policy, shard layout) and a checksum;
 * it is valid for the library version that wrote it (HFEM_VERSION) on any device.  serialize: buf NULL queries the size;
 * returns bytes or <0.  deserialize: device < 0 = host-only plan.  No reference counterpart (the reference has no plan).  */
int64_t hfem_plan_serialize(const hfem_plan *plan, void *buf, int64_t cap_bytes);
int hfem_plan_deserialize(int device, const void *blob, int64_t n_bytes, hfem_plan **out);

#define HFEM_FLAG_NO_GX 1   /* do not write gx_free (nodes fixed / no r-adaptivity) */
#define HFEM_FLAG_NO_GU 2   /* do not write gu_free */
#define HFEM_FLAG_NO_EDGES 4 /* domain energy only (EnergyLoss2D.domain_energy, src/loss.py:55-88) */
#define HFEM_FLAG_NO_LOSS_SUM 8 /* leave the per-tile partial energies unsummed, loss_out untouched
                                   (gradient-only callers; bench.py's kernel-only roofline leg) */
#define HFEM_FLAG_PHYSICAL_GRAD 64 /* opt-in: grad_u = G Jinv (HFEM_GRAD_PHYSICAL below) instead of the reference's
                                   * G Jinv^T (src/models.py:351).  fp64 TRI3 plan path.            */
#define HFEM_FLAG_DETERMINISTIC 128 /* fixed-order accumulation: gradients (and the loss) are bit-identical run to
                                   * run.  Node-centric gather over the node -> element adjacency (every element
                                   * is re-evaluated by each of its corners: 3x the flops, no atomics); the
                                   * cross-check of the atomic kernels SURVEY section 5 asks for, ~3-4x slower.
                                   * Whole plan only (tile_begin = 0, tile_end = -1 / n_tiles), fp64.          */
#define HFEM_FLAG_SUM_PREVIOUS 32 /* with NO_LOSS_SUM: one extra workgroup of THIS launch sums the tile energies the
                                   * PREVIOUS NO_LOSS_SUM launch on this plan left (the plan keeps two banks) into
                                   * loss_out -- the energy of evaluation k arrives with launch k+1, and the 1-block
                                   * reduction + kernel boundary leave the critical path.  hfem_plan_loss_sum
                                   * delivers the last one.  TRI3 default kernel path only.                    */

#define HFEM_FLAG_PEER_GET 512  /* paired-slot plans (no chained records) and 512-thread one-element-per-slot plans, after hfem_plan_set_peer_get: the launch starts with 8 service workgroups that
                                 * ARE the peer-window get (hfem_peer_iface_get's wait + unpack into this launch's x_free / u_free)
                                 * and the tiles named there (the rank's boundary tiles) wait for them inside the kernel        */
#define HFEM_FLAG_PEER_PUT 2048  /* hfem_tri3_energy_adam_step_ex with HFEM_FLAG_PEER_GET, after hfem_plan_set_peer_put: the launch also PUBLISHES --
                                 * its boundary tiles store the new rows of their interface nodes into every rank's window at
                                 * write-out and the last of them completes the put: one launch per owner-sharded training step */
#define HFEM_FLAG_FP32_MATH 1024 /* hfem_tri3_energy_plan_f32, hfem_tri3_energy_adam_step_ex(dtype 1): fp32 ARITHMETIC as well as fp32 rows -- what the reference itself
                                 * computes in for its default dtype (src/loss.py:16): packed-fp32 element math (the two elements of
                                 * a slot side by side), double LDS accumulators (rows rounded once); tile energies and loss stay fp64.  Paired-slot
                                 * plans; body force, tile ranges, NO_LOSS_SUM / SUM_PREVIOUS / SAME_BANK as the fp64 entry point. */
#define HFEM_FLAG_SAME_BANK 256 /* with NO_LOSS_SUM: another tile range of the SAME evaluation as the previous NO_LOSS_SUM
                                 * launch on this plan (a rank's boundary tiles after its interior tiles): the tile energies
                                 * go to the bank that launch wrote, so one hfem_plan_loss_sum / hfem_plan_iface_pack over
                                 * the union delivers the evaluation's energy.  Not with SUM_PREVIOUS.          */

/* One fwd+bwd "element-eval" pass over tiles [tile_begin, tile_end):
 *   loss_out[0]  = sum_elem A (W psi - beta)  -  sum_edge ds m        (OVERWRITTEN)
 *   gx_free[r]   = dL/d node_coords_free[r]   for rows owned by those tiles (OVERWRITTEN)
 *   gu_free[r]   = dL/d u_free[r]             likewise
 * = EnergyLoss2D.__call__ + loss.backward() (src/loss.py:113-116) including the
 * coords/u_full assembly and its backward.  Rows owned by tiles outside the range
 * are not touched (element sharding).  tile_end = -1: all.   */
int hfem_tri3_energy_plan(hfem_plan *plan, const double *x_free, const double *x_fixed,
                          const double *u_free, const double *u_fixed,
                          const double mat[4], double W, const double Bk[6],
                          const double *T_edge, const double Tconst[4],
                          int32_t tile_begin, int32_t tile_end, double *loss_out,
                          double *gx_free, double *gu_free, int32_t flags, void *stream);
/* Same pass for an fp32 model (the reference's default dtype): x / u rows and the gradient rows are float
 * [rows][2]; they are widened on load and rounded once on store, arithmetic and loss_out stay fp64.
 * Needs a zero body force (Bk NULL or all zero) and the default tile shape; any other plan returns an
 * argument error (the caller then widens to the fp64 entry point).  With HFEM_FLAG_FP32_MATH the arithmetic is fp32 too
 * (csrc/tri3_pair_f32.hip): results within the band the reference's own fp32 run occupies around exact arithmetic
 * (tests/test_gpu_tri3_f32.py), ~1.4x faster; body force allowed.                                     */
int hfem_tri3_energy_plan_f32(hfem_plan *plan, const float *x_free, const float *x_fixed,
                              const float *u_free, const float *u_fixed,
                              const double mat[4], double W, const double Bk[6],
                              const double *T_edge, const double Tconst[4],
                              int32_t tile_begin, int32_t tile_end, double *loss_out,
                              float *gx_free, float *gu_free, int32_t flags, void *stream);
/* One training step in one launch (no reference counterpart; the reference runs `loss.backward(); optimizer.step()`
 * with torch.optim.Adam, examples/example4.py:53-64 commented variant, example1-3): the pass above, but every tile
 * applies Adam's update to the rows it owns instead of storing their gradient.  m_*, v_* [rows][2]: moments, updated
 * in place.  x_out / u_out: the NEW parameter rows, buffers different from x_free / u_free (swap after the launch).
 * bc_dev: device {1 - beta1^step, sqrt(1 - beta2^step)} of this step, written by hfem_adam_prep (which also bumps the
 * device step counter) in stream order just before.  loss_out: energy
 * at the old parameters.  Whole plan, default tile shape, zero body force; flags: HFEM_FLAG_NO_EDGES, _NO_LOSS_SUM. */
int hfem_tri3_energy_adam_step(hfem_plan *plan, const double *x_free, const double *x_fixed,
                               const double *u_free, const double *u_fixed, const double mat[4], double W,
                               const double *T_edge, const double Tconst[4], double *x_out, double *u_out,
                               double *m_x, double *v_x, double *m_u, double *v_u, double lr_x, double lr_u,
                               double beta1, double beta2, double eps, const double *bc_dev,
                               double *loss_out, int32_t flags, void *stream);
/* General form.  dtype: 0 = fp64 rows, 1 = fp32 rows -- x / u / fixed rows, moments and new rows all float (an fp32 model, the
 * reference's default dtype src/loss.py:16, src/models.py:274, trains in one launch per iteration with no widening copy;
 * element arithmetic and loss_out stay fp64, the update is torch.optim.Adam's fp32 arithmetic on the once-rounded
 * gradient).  Bk [3][2]: body-force table as in hfem_tri3_energy_plan (NULL / zeros: none; not with SUM_PREVIOUS).
 * [tile_begin, tile_end) (-1 = all): a tile range updates exactly the rows its tiles own and leaves the other rows of
 * x_out / u_out alone (element sharding: the caller keeps both parameter buffers complete); flags accept
 * HFEM_FLAG_SAME_BANK for the second range of one evaluation.                                                      */
int hfem_tri3_energy_adam_step_ex(hfem_plan *plan, int32_t dtype, const void *x_free, const void *x_fixed,
                                  const void *u_free, const void *u_fixed, const double mat[4], double W,
                                  const double Bk[6], const double *T_edge, const double Tconst[4], void *x_out,
                                  void *u_out, void *m_x, void *v_x, void *m_u, void *v_u, double lr_x, double lr_u,
                                  double beta1, double beta2, double eps, const double *bc_dev, int32_t tile_begin,
                                  int32_t tile_end, double *loss_out, int32_t flags, void *stream);
int hfem_adam_prep(int device, int64_t *step_dev, double beta1, double beta2, double *bc_dev, void *stream);
/* loss_out[0] = sum, in tile order, of the per-tile partial energies that a launch with
 * HFEM_FLAG_NO_LOSS_SUM over the same tile range left in the plan (TRI3 and QUAD4 plans alike).   */
int hfem_plan_loss_sum(hfem_plan *plan, int32_t tile_begin, int32_t tile_end, double *loss_out, void *stream);

/* Span stamps (measurement aid): while dev_buf (n_slots x n_tiles x 2 uint64, caller-owned device memory) is set, launch i
 * of the paired-slot kernel through hfem_tri3_energy_plan writes for every tile it evaluates {tick at which the tile's
 * workgroup started, tick at which its first wave's gradient stores had drained} (s_memrealtime, 100 MHz) at
 * dev_buf[(i % n_slots) * n_tiles * 2 + 2 * tile].  max(end) - min(start) over a launch's tiles = its duration from the
 * first workgroup's start to the last one's end, measurable INSIDE any launch sequence (bench.py's cache regimes).
 * NULL = off (default).  Plans that take another kernel ignore it.                                                */
int hfem_plan_set_span_stamps(hfem_plan *plan, uint64_t *dev_buf, int64_t n_slots);

/* Process-wide DEFAULTS (atomics) that hfem_plan_create captures into the plan it builds; changing one
 * never affects an existing plan, and launches on different plans may run from different threads (a plan
 * serialises its own launches with a mutex).  Product knobs: "tiled_block" (threads per tile of the
 * one-element-per-slot kernels: 256, 512, 1024), "store_policy" (gradient stores: -1 = by mesh size and row locality -- nt
 * from 750 k nodes, sc1 write-through below --, 16, 2, 0), "tiled_fast", "fast_const_caps", "quad4_const_caps",
 * "plan_elem_order" (-1 auto, 3 one element per slot, 5 paired slots, 6 paired slots chained into strips), "plan_node_cap"
 * (home nodes per tile; -1 = the shard-aware policy), "plan_shards" (ranks the tiles will be split over: tiles are sized
 * for the elements PER RANK and every rank's boundary tiles come first in its range), "plan_pair_block" (threads per tile
 * of a paired plan: -1 auto, 256, 512), "plan_chunk_cap", "plan_curve" (0 Morton, 1 Hilbert), "plan_snap" (tile cuts snap
 * back to coarse curve cells by up to that percentage of a tile; 0 = off), "plan_read_pack" (paired slots also packed
 * against ds_read_b128 bank conflicts: number of partner rows examined, default 2; 0 = off).  The ablation / stamp /
 * pipeline knobs exist only in the lab build (libhidenn_hip_lab.so, hfem_get_option("lab_build") == 1); the product
 * library rejects them.
 * hfem_get_option returns the value or -1.                                     */
int hfem_set_option(const char *name, int value);
int hfem_get_option(const char *name);

/* ------------------------------------------------------------------ per-point TRI3
 * Unfused forward of src/models.py:316-357 on assembled X,U: u_h [M][2],
 * detJ [M], grad_u [M][2][2] at reference points x_eval [M][2] of elements
 * elem_id [M] (int64, the reference's dtype).                                  */
int hfem_tri3_eval_fwd(int device, const double *X, const double *U, const int32_t *conn,
                       const double *x_eval, const int64_t *elem_id, int64_t m,
                       double *u_h, double *detJ, double *grad_u, void *stream);
/* Backward of the above: cotangents cu [M][2], cd [M], cg [M][2][2] ->
 * ACCUMULATES gX,gU [Nn][2] (fp64 atomics; caller zeroes).                    */
int hfem_tri3_eval_bwd(int device, const double *X, const double *U, const int32_t *conn,
                       const double *x_eval, const int64_t *elem_id, int64_t m,
                       const double *cu, const double *cd, const double *cg,
                       double *gX, double *gU, void *stream);
/* Same two with an explicit gradient convention.  HFEM_GRAD_REFERENCE: dN_dx = Jinv * dN_dxi exactly as
 * src/models.py:351 computes it (grad_u = G Jinv^T; the parity contract and the default everywhere).
 * HFEM_GRAD_PHYSICAL (opt-in): dN_dx = Jinv^T * dN_dxi, i.e. grad_u = G Jinv -- the physical
 * gradient: exact for linear fields and invariant to the local node order of an element.            */
#define HFEM_GRAD_REFERENCE 0
#define HFEM_GRAD_PHYSICAL 1
int hfem_tri3_eval_fwd_conv(int device, const double *X, const double *U, const int32_t *conn,
                            const double *x_eval, const int64_t *elem_id, int64_t m,
                            double *u_h, double *detJ, double *grad_u, int32_t convention, void *stream);
int hfem_tri3_eval_bwd_conv(int device, const double *X, const double *U, const int32_t *conn,
                            const double *x_eval, const int64_t *elem_id, int64_t m,
                            const double *cu, const double *cd, const double *cg,
                            double *gX, double *gU, int32_t convention, void *stream);
/* Edge branch of src/models.py:359-376: u_h [M][2], ds [M]; and its backward. */
int hfem_edge2_eval_fwd(int device, const double *X, const double *U, const int32_t *edges,
                        const double *xi, const int64_t *edge_id, int64_t m,
                        double *u_h, double *ds, void *stream);
int hfem_edge2_eval_bwd(int device, const double *X, const double *U, const int32_t *edges,
                        const double *xi, const int64_t *edge_id, int64_t m,
                        const double *cu, const double *cds, double *gX, double *gU,
                        void *stream);

/* ------------------------------------------------------------------ QUAD4-iso (extension)
 * The reference has no isoparametric quadrilateral; these follow the SURVEY section 8a
 * spec with the reference's conventions (J[i][j] = d x_i/d xi_j, dN_dx = Jinv*D_N as
 * src/models.py:339-351, abs(detJ) as src/loss.py:84): reference square [-1,1]^2, local nodes CCW from
 * (-1,-1), 2x2 Gauss (+-1/sqrt(3), weights 1), zero body force.  conn4 [Ne][4] int32.
 * Planless (fp64 global atomics): ACCUMULATES loss_acc[0], gX, gU (caller zeroes); gX/gU may be NULL. */
int hfem_quad4_energy_atomic(int device, const double *X, const double *U, const int32_t *conn4,
                             int64_t e_begin, int64_t e_end, int64_t nn, const double mat[4],
                             double *loss_acc, double *gX, double *gU, void *stream);
/* Tiled QUAD4 (plan from hfem_plan_create_ex(..., 4, ...)): same contract as hfem_tri3_energy_plan --
 * loss_out / gx_free / gu_free rows of the tile range OVERWRITTEN, free/fixed row maps fused.      */
int hfem_quad4_energy_plan(hfem_plan *plan, const double *x_free, const double *x_fixed,
                           const double *u_free, const double *u_fixed, const double mat[4],
                           const double *T_edge, const double Tconst[4], int32_t tile_begin,
                           int32_t tile_end, double *loss_out, double *gx_free, double *gu_free,
                           int32_t flags, void *stream);
/* Same with a body force: Bq [4][2] = b at the 2x2 Gauss points in REFERENCE coordinates (the reference's triangle
 * path hands b_force the reference points, src/loss.py:60,80 -- SURVEY F6), order (-,-) (+,-) (-,+) (+,+);
 * e -= sum_q |detJ_q| u_h(xi_q).b_q.  NULL / all zero = hfem_quad4_energy_plan.                        */
int hfem_quad4_energy_plan_body(hfem_plan *plan, const double *x_free, const double *x_fixed,
                                const double *u_free, const double *u_fixed, const double mat[4],
                                const double Bq[8], const double *T_edge, const double Tconst[4],
                                int32_t tile_begin, int32_t tile_end, double *loss_out, double *gx_free,
                                double *gu_free, int32_t flags, void *stream);
/* General form.  dtype: 0 = fp64 rows, 1 = fp32 rows (x / u / fixed rows and the gradient rows are float [rows][2]: an
 * fp32 model, the reference's default dtype src/loss.py:16, without widening copies -- widened on load, rounded once on
 * store, arithmetic and loss_out fp64).  flags additionally accept HFEM_FLAG_PHYSICAL_GRAD (grad_u = G Jinv instead of the
 * reference convention's G Jinv^T) and, for fp64 rows on the whole plan, HFEM_FLAG_DETERMINISTIC (node-centric fixed-order
 * kernel: bit-identical run to run, several times slower).  Bq as hfem_quad4_energy_plan_body (NULL: none).           */
int hfem_quad4_energy_plan_ex(hfem_plan *plan, int32_t dtype, const void *x_free, const void *x_fixed,
                              const void *u_free, const void *u_fixed, const double mat[4], const double Bq[8],
                              const double *T_edge, const double Tconst[4], int32_t tile_begin, int32_t tile_end,
                              double *loss_out, void *gx_free, void *gu_free, int32_t flags, void *stream);
/* Per-point forward/backward with the (x_ref, element_id) contract of src/models.py:316:
 * x_eval [M][2] in [-1,1]^2 -> u_h [M][2], detJ [M], grad_u [M][2][2]; backward ACCUMULATES gX,gU. */
int hfem_quad4_eval_fwd(int device, const double *X, const double *U, const int32_t *conn4,
                        const double *x_eval, const int64_t *elem_id, int64_t m,
                        double *u_h, double *detJ, double *grad_u, void *stream);
int hfem_quad4_eval_bwd(int device, const double *X, const double *U, const int32_t *conn4,
                        const double *x_eval, const int64_t *elem_id, int64_t m,
                        const double *cu, const double *cd, const double *cg,
                        double *gX, double *gU, void *stream);

/* ------------------------------------------------------------------ fused optimiser step
 * One launch of torch.optim.Adam's update (examples/example1.py:31, example2.py:37, example3.py:89;
 * default betas/eps, no weight decay, no amsgrad) on a flat tensor of n parameters:
 * m += (g-m)(1-b1); v = v b2 + (1-b2) g g; p -= lr/(1-b1^step) * m / (sqrt(v)/sqrt(1-b2^step) + eps).
 * dtype: 0 = fp64, 1 = fp32 (p, g, m, v all of that type).  step counts from 1.            */
int hfem_adam_step(int device, void *p, const void *g, void *m, void *v, int64_t n, int32_t dtype,
                   double lr, double beta1, double beta2, double eps, int64_t step, void *stream);
/* hipGraph-capturable form: the (1-based) step count is read from device memory when the kernel runs;
 * hfem_counter_add bumps such a counter in stream order (call it once before the step's kernels).   */
int hfem_adam_step_dev(int device, void *p, const void *g, void *m, void *v, int64_t n, int32_t dtype,
                       double lr, double beta1, double beta2, double eps, const int64_t *step_dev,
                       void *stream);
int hfem_counter_add(int device, int64_t *counter, int64_t inc, void *stream);
/* Multi-tensor form: EVERY parameter tensor of the optimiser in ONE launch (the reference's models have 1-3 parameter
 * tensors, examples/example4.py:54-64; per-tensor launches cost a kernel boundary each).  table_dev[n_tensors] lives in
 * DEVICE memory; tensor t is updated by blocks [block_begin_t, block_begin_{t+1}) of 256 threads, block b of a tensor taking
 * the 16-byte vectors [b * chunk_vecs, (b + 1) * chunk_vecs); n_blocks = total.  dtype per tensor: 0 fp64, 1 fp32.
 * Step count: step_dev (may be NULL) holds the number of COMPLETED steps; the update uses step_dev[0] + step_offset
 * (step_offset alone when step_dev is NULL: a host-side count).  With step_dev the kernel itself bumps the counter once
 * all blocks have read it (ticket_dev: HFEM_ADAM_TICKET_INTS int32 of device memory, zero before the first call; a
 * two-level last-arriver count) -- no hfem_counter_add.  Keep n_blocks at a few per CU (<= 2048): every block ends with
 * one device-scope atomic.                                                                                            */
#define HFEM_ADAM_TICKET_INTS 1056
typedef struct hfem_adam_tensor {
    void *p; const void *g; void *m; void *v;
    int64_t n;
    double lr, beta1, beta2, eps;
    int32_t dtype, block_begin;
} hfem_adam_tensor;
int hfem_adam_multi_dev(int device, const hfem_adam_tensor *table_dev, int32_t n_tensors, int32_t n_blocks,
                        int64_t chunk_vecs, int64_t *step_dev, int64_t step_offset, int32_t *ticket_dev, void *stream);

/* ------------------------------------------------------------------ row gather/scatter
 * src/models.py:292-305 as index lists instead of bool-mask index_put (which
 * runs aten::nonzero on every call): dst[idx[r]][0..w) = src[r][0..w).         */
int hfem_scatter_rows(int device, const double *src, const int32_t *idx, int64_t rows,
                      int32_t width, double *dst, void *stream);
int hfem_gather_rows(int device, const double *src, const int32_t *idx, int64_t rows,
                     int32_t width, double *dst, void *stream);

/* ------------------------------------------------------------------ L-BFGS on the flat parameter vector
 * (torch.optim.LBFGS as examples/example4.py:68-78 uses it: fixed step, no line search).
 * State (history ring of `history` (s, y) pairs, Gram blocks, direction d, step t) lives on the device.
 * One inner iteration of torch's loop is:
 *     hfem_lbfgs_direction(g)  ->  hfem_lbfgs_apply(param, offset, numel) per parameter tensor
 *     ->  closure (energy kernel) -> hfem_lbfgs_check(g_new, loss_new, after_update = 1) -> host reads status.
 * dtype: 0 fp64, 1 fp32 (vectors); dots and the recursion are fp64 either way.
 * status[8] (host): loss, flags (bit0 max|g| <= tol_grad, bit1 max|t d| <= tol_change,
 * bit2 |loss - prev_loss| < tol_change, bit3 g.d > -tol_change: nothing was applied), max|g|, g.d, t,
 * history count, n_iter, H_diag.  hfem_lbfgs_check synchronises the stream; the others only enqueue.      */
typedef struct hfem_lbfgs hfem_lbfgs;
int hfem_lbfgs_create(int device, int64_t n, int32_t history, int32_t dtype, hfem_lbfgs **out);
int hfem_lbfgs_destroy(hfem_lbfgs *opt);
int hfem_lbfgs_check(hfem_lbfgs *opt, const void *g, const double *loss, int32_t after_update, double tol_grad,
                     double tol_change, double *status_host, void *stream);
int hfem_lbfgs_direction(hfem_lbfgs *opt, const void *g, double lr, double tol_change, void *stream);
int hfem_lbfgs_apply(hfem_lbfgs *opt, void *p, int64_t offset, int64_t numel, void *stream);
void *hfem_lbfgs_direction_ptr(hfem_lbfgs *opt);
/* NODE-SHARDED L-BFGS (hidenn_fem_amd/optim.py ShardedLBFGS; no reference counterpart -- the reference runs example 4 on one
 * device).  The optimiser object holds the history, gradient copy and direction of the parameter rows ONE RANK owns (n = 2 x
 * its owned rows); per inner iteration every rank
 *     hfem_lbfgs_shard_gather (its gradient rows -> flat local vector)
 *     hfem_lbfgs_shard_local  (speculative pair + ONE pass over its history -> a payload of
 *                              hfem_lbfgs_shard_payload_doubles() doubles: per-slot dots, y.s, y.y, gradient statistics,
 *                              max|d|, its partial energy)
 *     [the caller gathers the payloads of all ranks to every rank, rank order: one small all_gather / peer-window put]
 *     hfem_lbfgs_shard_finish (sums in rank order -> torch's break tests -> memory update, recursion, its part of d; status)
 *     hfem_lbfgs_shard_apply  (x[rows], u[rows] += t d)
 * so the two passes over the history shrink by the number of ranks and every rank takes bit-identical decisions.  With
 * world = 1 (gathered = the payload itself) the flow is torch.optim.LBFGS / hfem_lbfgs_direction on one device.           */
int64_t hfem_lbfgs_shard_payload_doubles(const hfem_lbfgs *opt);
int hfem_lbfgs_shard_gather(hfem_lbfgs *opt, const void *gx, const int32_t *rows_x, int64_t nx, const void *gu,
                            const int32_t *rows_u, int64_t nu, void *out, void *stream);
int hfem_lbfgs_shard_local(hfem_lbfgs *opt, const void *g, const double *loss_local_dev, double *payload_dev, void *stream);
int hfem_lbfgs_shard_finish(hfem_lbfgs *opt, const void *g, const double *gathered_dev, int32_t world, int32_t after_update,
                            int32_t want_direction, double lr, double tol_grad, double tol_change, double *status_host,
                            void *stream);
/* hfem_lbfgs_shard_finish with status_host = NULL only enqueues (the record goes to a pinned buffer of the optimiser): a whole
 * steady-state iteration -- apply, energy, gather, local, the exchange, finish -- is then capturable in ONE hipGraph;
 * hfem_lbfgs_shard_status synchronises the stream and hands the record out.                                          */
int hfem_lbfgs_shard_status(hfem_lbfgs *opt, double *status_host, void *stream);
int hfem_lbfgs_shard_apply(hfem_lbfgs *opt, void *x, const int32_t *rows_x, int64_t nx, void *u, const int32_t *rows_u,
                           int64_t nu, void *stream);

/* ------------------------------------------------------------------ post-processing
 * hfem_tri3_von_mises: per element, grad_u at the centroid (constant on a P1 triangle; reference
 * convention, src/models.py:351-355) -> strain -> plane-stress stress -> von Mises, exactly the chain of
 * src/plots.py:183-198 (sigma_xy = E/(1+nu) eps_xy).  von_mises[Ne]; grad_u[Ne][2][2] optional (NULL).
 * hfem_line2_slopes: out[i][c] = (u[i+1][c] - u[i][c]) / (grid[i+1] - grid[i]), i < n_nodes - 1: the
 * per-element du/dx that src/plots.py:5-27 obtains with one autograd call per element.               */
int hfem_tri3_von_mises(int device, const double *X, const double *U, const int32_t *conn, int64_t ne,
                        double E, double nu, double *von_mises, double *grad_u, void *stream);
int hfem_line2_slopes(int device, const double *grid, const double *u, int64_t n_nodes, int32_t dim_u,
                      double *out, void *stream);
/* hfem_quad4_von_mises: the QUAD4 twin of hfem_tri3_von_mises -- the same chain and outputs with grad_u taken at the cell
 * centre (xi = eta = 0), reference convention; conn[Ne][4], local nodes counter-clockwise from (-1, -1).           */
int hfem_quad4_von_mises(int device, const double *X, const double *U, const int32_t *conn, int64_t ne,
                         double E, double nu, double *von_mises, double *grad_u, void *stream);

/* ------------------------------------------------------------------ nodal stress recovery and ZZ error estimate
 * No reference counterpart.  X[Nn][2], U[Nn][2] by node id, conn[Ne][3 or 4]; mat[4] = (c11, c12, c22, c33) of the
 * plane-stress C (HOST pointer), S = C^-1; Voigt stress sigma = C (eps_xx, eps_yy, gamma_xy) of grad_u in the reference
 * convention or, with flags = HFEM_FLAG_PHYSICAL_GRAD, the physical one.  Points: TRI3 the centroid with w = |det J| / 2,
 * QUAD4 the 2x2 Gauss points with w_q = |det J_q| (|det|: either orientation).
 * hfem_*_stress_recover (lumped L2 projection): nodal_stress[Nn][3] = sum_{e at n} sum_q w_q N_n(q) sigma_h(q) /
 *   sum_{e at n} sum_q w_q N_n(q); nodal_area[Nn] (optional, NULL) = that denominator, the lumped nodal area.  adj_ptr[Nn + 1],
 *   adj[npe Ne]: node -> (element, corner) CSR, entries e << 2 | c ascending in e at every node (hence Ne < 2^29).  One
 *   thread per node adds in that order: no atomics, bitwise reproducible.  A node of no element gets zeros.
 * hfem_*_zz_error: eta2[Ne] = sum_q w_q d_q.S.d_q with d_q = sum_k N_k(q) sigma*_k - sigma_h(q) (TRI3: the exact closed form
 *   A/12 [sum_k d_k.S.d_k + (sum_k d_k).S.(sum_k d_k)]); norm2[Ne] (optional, NULL) = sum_q w_q sigma_h.S.sigma_h = twice the
 *   element's strain energy; totals[2] = {sum eta2, sum norm2}, summed on the device in a fixed order (no atomics).
 *   partials: caller-owned workspace of 2 * ceil(Ne / 256) doubles.
 * All device pointers except mat; launch-only (capturable).  Ne == 0 (or Nn == 0) returns 0 without touching a device. */
int hfem_tri3_stress_recover(int device, const double *X, const double *U, const int32_t *conn, int64_t ne, int64_t nn,
                             const int32_t *adj_ptr, const int32_t *adj, const double *mat, int32_t flags,
                             double *nodal_stress, double *nodal_area, void *stream);
int hfem_quad4_stress_recover(int device, const double *X, const double *U, const int32_t *conn, int64_t ne, int64_t nn,
                              const int32_t *adj_ptr, const int32_t *adj, const double *mat, int32_t flags,
                              double *nodal_stress, double *nodal_area, void *stream);
int hfem_tri3_zz_error(int device, const double *X, const double *U, const int32_t *conn, int64_t ne,
                       const double *nodal_stress, const double *mat, int32_t flags, double *eta2, double *norm2,
                       double *partials, double *totals, void *stream);
int hfem_quad4_zz_error(int device, const double *X, const double *U, const int32_t *conn, int64_t ne,
                        const double *nodal_stress, const double *mat, int32_t flags, double *eta2, double *norm2,
                        double *partials, double *totals, void *stream);

/* ------------------------------------------------------------------ compressible Neo-Hookean energy (TRI3)
 * No reference counterpart.  Total potential of a TRI3 model at finite strain on a ONE-ELEMENT-PER-SLOT tile plan
 * (plan_elem_order 3), with its gradients w.r.t. the free coordinate and displacement rows.  Per element, with
 * Jg = [X0 - X2, X1 - X2], G = [U0 - U2, U1 - U2]:  H = G Jg^-1 (the true displacement gradient, always), j = tr H + det H
 * (= J - 1), L = log1p(j), psi = mu (tr H + H:H / 2 - L) + lambda L^2 / 2, e = |det Jg| (W psi - sum_k U_k . B_k); Neumann
 * edges are dead loads on the reference configuration (T_edge / Tconst as hfem_tri3_energy_plan).  lame[2] = (lambda, mu),
 * Bk[6] (may be NULL = 0) and Tconst[4] are HOST pointers.  dtype: 0 = every row array double, 1 = float (widened on load,
 * fp64 arithmetic, gradient rows rounded once on store).  An element with J <= 0 contributes +inf to the loss and ZERO to
 * both gradients.  loss_out[1] and info_out[2] (may be NULL) = {min J over the elements, number of elements with J <= 0}
 * are device doubles; work = caller-owned device workspace of 3 * n_tiles doubles (the plan's own partials banks are not
 * used, so a lagged loss sum in flight on the plan is undisturbed).  gx_free / gu_free may be NULL only with the matching
 * flag.  flags: HFEM_FLAG_NO_GX, HFEM_FLAG_NO_GU, HFEM_FLAG_NO_EDGES; any other flag, a QUAD4, paired or host-only plan or a
 * missing pointer is an argument error.  Launch-only (capturable).                                                      */
int hfem_tri3_hyper_energy_plan(hfem_plan *plan, int32_t dtype, const void *x_free, const void *x_fixed,
                                const void *u_free, const void *u_fixed, const double lame[2], double W,
                                const double Bk[6], const double *T_edge, const double Tconst[4], double *loss_out,
                                double *info_out, double *work, void *gx_free, void *gu_free, int32_t flags, void *stream);

/* ------------------------------------------------------------------ Neo-Hookean finite-strain energy (QUAD4)
 * The same potential on a QUAD4 plan (one cell per slot, the plan every QUAD4 entry point uses), 2x2 Gauss points
 * (+-1/sqrt(3), weights 1, order (-,-) (+,-) (-,+) (+,+)).  Per point, with J = sum_k X_k (x) dN_k/dxi and
 * G = sum_k U_k (x) dN_k/dxi:  H = G J^-1 (the true displacement gradient, always), j = tr H + det H, L = log1p(j),
 * psi = mu (tr H + H:H / 2 - L) + lambda L^2 / 2, e = sum_q |det J_q| (psi_q - b_q . u_h(xi_q)); Bq[8] (HOST, may be NULL = 0)
 * is the body force at the four points (reference coordinates), lame[2], T_edge / Tconst, dtype, loss_out, info_out, work
 * (3 * n_tiles doubles), gx_free / gu_free and flags exactly as hfem_tri3_hyper_energy_plan.  A cell with j_q <= -1 (or NaN)
 * at any of its points contributes +inf to the loss and ZERO to both gradients and is counted once; info_out[0] is the minimum
 * of 1 + j_q over all points.  Tiles with more than 768 slots run (a plain loop behind the prefetched records); a TRI3 or
 * host-only plan, a missing pointer, any other flag, or a tile that needs more than 64 KiB of LDS (32 bytes per local node +
 * 32 per owned row + 96) is an argument error.  Launch-only (capturable).                                               */
int hfem_quad4_hyper_energy_plan(hfem_plan *plan, int32_t dtype, const void *x_free, const void *x_fixed,
                                 const void *u_free, const void *u_fixed, const double lame[2], const double Bq[8],
                                 const double *T_edge, const double Tconst[4], double *loss_out, double *info_out,
                                 double *work, void *gx_free, void *gu_free, int32_t flags, void *stream);

/* ------------------------------------------------------------------ multi-GPU interface exchange
 * Owner-sharded mode (no reference counterpart): one all_gather per step of a fixed-size
 * payload per rank, in double2 units:  [x rows | u rows | padding][loss partial, 0].
 * hfem_iface_pack: out[i] = x_free[rows[i]] (i < n_x), u_free[rows[i]] (n_x <= i < n_x + n_u).
 * hfem_iface_unpack: x_free[dst[i]] = recv[src[i]] (i < n_x), u_free[dst[i]] = recv[src[i]] (next n_u);
 * src indexes the gathered buffer (world payloads of `stride` double2 each); loss_out (may be NULL)
 * = sum over ranks, in rank order, of recv[r * stride + loss_slot].x.                               */
int hfem_iface_pack(int device, const double *x_free, const double *u_free, const int32_t *rows,
                    int32_t n_x, int32_t n_u, double *out, void *stream);
int hfem_iface_unpack(int device, const double *recv, const int32_t *src, const int32_t *dst, int32_t n_x,
                      int32_t n_u, double *x_free, double *u_free, int32_t world, int64_t stride,
                      int64_t loss_slot, double *loss_out, void *stream);

/* hfem_iface_pack + the rank's energy + the optimiser's step counter in ONE launch (the owner-sharded training step is a
 * chain of small dependent launches, each worth a kernel boundary): out as hfem_iface_pack; out[loss_slot] = {sum, in tile
 * order, of the tile energies that the HFEM_FLAG_NO_LOSS_SUM launch(es) over [tile_begin, tile_end) left in the plan, 0};
 * counter (may be NULL) += 1; bc_next (may be NULL; needs counter) = {1 - beta1^(c + 1), sqrt(1 - beta2^(c + 1))} with c the
 * bumped count: the bias corrections of the NEXT step, for its fused energy + Adam launch (no hfem_adam_prep launch).
 * loss_slot >= n_x + n_u, in double2 units.                                                                       */
int hfem_plan_iface_pack(hfem_plan *plan, int32_t tile_begin, int32_t tile_end, const double *x_free,
                         const double *u_free, const int32_t *rows, int32_t n_x, int32_t n_u, double *out,
                         int64_t loss_slot, int64_t *counter, double beta1, double beta2, double *bc_next, void *stream);
/* The exchange for fp32 models (the reference's default dtype; `_f32` as for the energy entry points): parameter rows are
 * float2, the payload stays double2 -- widened on the way out, rounded back (losslessly) on the way in.               */
int hfem_plan_iface_pack_f32(hfem_plan *plan, int32_t tile_begin, int32_t tile_end, const float *x_free,
                             const float *u_free, const int32_t *rows, int32_t n_x, int32_t n_u, double *out,
                             int64_t loss_slot, int64_t *counter, double beta1, double beta2, double *bc_next, void *stream);
int hfem_iface_unpack_f32(int device, const double *recv, const int32_t *src, const int32_t *dst, int32_t n_x,
                          int32_t n_u, float *x_free, float *u_free, int32_t world, int64_t stride,
                          int64_t loss_slot, double *loss_out, void *stream);

/* Peer-window exchange (csrc/peer.hip): the interface payload of hfem_plan_iface_pack written BY THE PACK KERNEL into a
 * receive window on every rank -- stores over xGMI into IPC-mapped device memory -- with arrival flags, instead of an
 * all_gather: no collective, no second stream, capturable.  One process per GPU (at most 16 ranks).  Set-up, once:
 *   hfem_peer_create(device, rank, world, stride, &peer)   stride = interface rows + 1 (double2 units, as the all_gather
 *                                                          payload); allocates and zeroes this rank's window
 *   hfem_peer_ipc_handle(peer, h64)                        64-byte hipIpcMemHandle_t of the window; exchange the handles of
 *                                                          all ranks by any side channel (torch.distributed, a file, MPI)
 *   hfem_peer_connect(peer, handles[world][64])            maps the other ranks' windows (own entry ignored); world == 1
 *                                                          needs neither call.  Barrier before the first put.
 * Per step, stream-ordered, STRICTLY alternating on every rank:
 *   hfem_plan_iface_put(...)   = hfem_plan_iface_pack with out = slot (puts so far) & 1 of my lane in every window, then a
 *                                system-scope fence and flag = puts + 1 in every window
 *   hfem_peer_iface_get(...)   = waits until every rank's flag of that slot has arrived in MY window, then
 *                                hfem_iface_unpack from it (src indices as for the gathered [world][stride] payload).
 * The wait is bounded: after timeout_ticks (100 MHz: 1e8 = 1 s) without a flag the kernel sets the sticky status bit 1 and
 * goes on (later gets no longer wait) -- a lost peer is an error the host reads with hfem_peer_status (which synchronises
 * with the device), never a hung GPU.  hfem_peer_status: status_out = sticky bits, puts_out = completed puts (either may
 * be NULL).                                                                                                       */
typedef struct hfem_peer hfem_peer;
int hfem_peer_create(int device, int32_t rank, int32_t world, int64_t stride, hfem_peer **out);
int hfem_peer_ipc_handle(hfem_peer *peer, void *handle_out_64_bytes);
int hfem_peer_connect(hfem_peer *peer, const void *handles_world_x_64_bytes);
int hfem_peer_destroy(hfem_peer *peer);
int hfem_peer_status(hfem_peer *peer, int32_t *status_out, int64_t *puts_out);
/* The get INSIDE the next energy launch (one launch less per step, and no tile that does not need foreign rows waits):
 * hfem_peer_attach_get stores hfem_peer_iface_get's tables / loss slot / timeout in device memory, hfem_plan_set_peer_get
 * binds them to a plan together with the tile range [wait_begin, wait_end) that must wait (the rank's boundary tiles:
 * hfem_plan_export id 10), and hfem_tri3_energy_plan / hfem_tri3_energy_adam_step_ex with HFEM_FLAG_PEER_GET then run the
 * get as their first workgroups.  Status bit 2: a boundary tile gave up waiting (after 2 x timeout_ticks).           */
int hfem_peer_attach_get(hfem_peer *peer, const int32_t *src, const int32_t *dst, int32_t n_x, int32_t n_u,
                         int64_t loss_slot, double *loss_out, int64_t timeout_ticks);
int hfem_plan_set_peer_get(hfem_plan *plan, hfem_peer *peer, int32_t wait_begin, int32_t wait_end);
/* The put INSIDE the fused energy + Adam launch (round 4: ONE launch per owner-sharded training step).  hfem_peer_attach_put
 * stores in device memory where every parameter row sits in this rank's payload lane (pos_x / pos_u: per row of x_free /
 * u_free the double2 index, -1 = not an interface row), the loss slot and the optimiser's step counter + betas;
 * hfem_plan_set_peer_put binds them to a paired-slot plan with the TWO bias-correction buffers the steps alternate between.
 * hfem_tri3_energy_adam_step_ex(..., HFEM_FLAG_PEER_GET | HFEM_FLAG_PEER_PUT | HFEM_FLAG_NO_LOSS_SUM) then: the boundary tiles
 * [wait_begin, wait_end) of hfem_plan_set_peer_get store the NEW rows of their interface nodes into every rank's window at
 * write-out; the last of them to finish writes the rank's energy of the PREVIOUS evaluation into the loss slot (this one's is
 * not complete yet: the global energy a get delivers therefore lags one step more; hfem_plan_iface_put flushes the last),
 * bumps the step counter, writes the next step's bias corrections into the other buffer and raises the flags.  Protocol,
 * slots and bounded waits as hfem_plan_iface_put / the in-launch get.                                                */
int hfem_peer_attach_put(hfem_peer *peer, const int32_t *pos_x, const int32_t *pos_u, int64_t loss_slot, int64_t *counter,
                         double beta1, double beta2);
int hfem_plan_set_peer_put(hfem_plan *plan, hfem_peer *peer, double *bc_a, double *bc_b);
int hfem_plan_iface_put(hfem_plan *plan, hfem_peer *peer, int32_t tile_begin, int32_t tile_end, const double *x_free,
                        const double *u_free, const int32_t *rows, int32_t n_x, int32_t n_u, int64_t loss_slot,
                        int64_t *counter, double beta1, double beta2, double *bc_next, void *stream);
int hfem_peer_iface_get(hfem_peer *peer, const int32_t *src, const int32_t *dst, int32_t n_x, int32_t n_u, double *x_free,
                        double *u_free, int64_t loss_slot, double *loss_out, int64_t timeout_ticks, void *stream);
int hfem_plan_iface_put_f32(hfem_plan *plan, hfem_peer *peer, int32_t tile_begin, int32_t tile_end, const float *x_free,
                            const float *u_free, const int32_t *rows, int32_t n_x, int32_t n_u, int64_t loss_slot,
                            int64_t *counter, double beta1, double beta2, double *bc_next, void *stream);
int hfem_peer_iface_get_f32(hfem_peer *peer, const int32_t *src, const int32_t *dst, int32_t n_x, int32_t n_u, float *x_free,
                            float *u_free, int64_t loss_slot, double *loss_out, int64_t timeout_ticks, void *stream);

/* In-library collectives: one RCCL communicator per rank (one process per GPU).  Rank 0 calls
 * hfem_mg_unique_id and broadcasts the 128 bytes by any side channel (torch.distributed, a file, MPI); every rank
 * then calls hfem_mg_comm_create.  The collectives only ENQUEUE on the caller's stream -- in stream order right
 * after the energy kernel -- so a whole multi-GPU step can be captured into one hipGraph.  fp64, sum.
 * hfem_mg_allgather: recv = [rank 0's `count` doubles | rank 1's | ...].  send == recv + rank * count is allowed.
 * RCCL is bound at run time (dlopen, in this order: the path given to hfem_mg_load, $HFEM_RCCL_PATH, a librccl already
 * mapped into the process, the ROCm installation); without it these calls return an error, the rest works.   */
typedef struct hfem_mg_comm hfem_mg_comm;
int hfem_mg_load(const char *librccl_path);
int hfem_mg_unique_id(void *id_out_128_bytes);
int hfem_mg_comm_create(int device, int rank, int world, const void *id_128_bytes, hfem_mg_comm **out);
int hfem_mg_comm_destroy(hfem_mg_comm *comm);
int hfem_mg_allreduce_sum(hfem_mg_comm *comm, const double *send, double *recv, int64_t count, void *stream);
int hfem_mg_allgather(hfem_mg_comm *comm, const double *send, double *recv, int64_t count, void *stream);
/* Adam on the ROWS a rank owns (owner-sharded mode: a rank updates exactly the parameter rows its tiles own):
 * hfem_adam_step_dev restricted to rows[n_rows] of [.][2] fp64 arrays p, g, m, v.                          */
int hfem_adam_step_rows_dev(int device, double *p, const double *g, double *m, double *v, const int32_t *rows,
                            int64_t n_rows, double lr, double beta1, double beta2, double eps,
                            const int64_t *step_dev, void *stream);

/* Both parameter tensors of the triangular model in one launch: rows_x[n_x] of (px, gx, mx, vx) with lr_x and rows_u[n_u]
 * of (pu, gu, mu, vu) with lr_u.  The (1-based) step of the bias corrections is step_dev[0] + step_offset: 0 when the
 * counter was bumped before (hfem_counter_add), 1 when it is bumped after (hfem_plan_iface_pack).                */
int hfem_adam_step_rows2_dev(int device, double *px, const double *gx, double *mx, double *vx, const int32_t *rows_x,
                             int64_t n_x, double lr_x, double *pu, const double *gu, double *mu, double *vu,
                             const int32_t *rows_u, int64_t n_u, double lr_u, double beta1, double beta2, double eps,
                             const int64_t *step_dev, int64_t step_offset, void *stream);
/* The same on float rows (an fp32 model): torch's fp32 arithmetic. */
int hfem_adam_step_rows2_dev_f32(int device, float *px, const float *gx, float *mx, float *vx, const int32_t *rows_x,
                                 int64_t n_x, double lr_x, float *pu, const float *gu, float *mu, float *vu,
                                 const int32_t *rows_u, int64_t n_u, double lr_u, double beta1, double beta2, double eps,
                                 const int64_t *step_dev, int64_t step_offset, void *stream);

/* ------------------------------------------------------------------ 1D / structured
 * Grid parametrisation softplus -> clamp(1e-6) -> cumsum -> renormalise
 * (src/models.py:45-56, 146-168): p[n] -> grid[n+1]; backward ggrid[n+1] -> gp[n].
 * mask (uint8[n+1], may be NULL) + initial[n+1]: grid = where(mask, initial, grid)
 * (src/models.py:165-166); masked entries get no gradient.                     */
int hfem_grid_param_fwd(int device, const double *p, int64_t n, double x0, double xN,
                        const uint8_t *mask, const double *initial, double *grid,
                        void *stream);
int hfem_grid_param_bwd(int device, const double *p, int64_t n, double x0, double xN,
                        const uint8_t *mask, const double *ggrid, double *gp, void *stream);
/* Same for long grids, over all CUs (three small launches each way): ws = hfem_grid_param_ws_elems(n) doubles
 * of scratch; cum[n] is written by the forward (running sums of the clamped softplus, cum[n-1] = total) and
 * read by the backward.                                                                              */
int64_t hfem_grid_param_ws_elems(int64_t n);
int hfem_grid_param_fwd_ws(int device, const double *p, int64_t n, double x0, double xN, const uint8_t *mask,
                           const double *initial, double *grid, double *cum, double *ws, void *stream);
int hfem_grid_param_bwd_ws(int device, const double *p, int64_t n, double x0, double xN, const uint8_t *mask,
                           const double *ggrid, const double *cum, double *gp, double *ws, void *stream);

/* LINE2 hat-function interpolation, src/models.py:70-90: grid[n], u[n] full
 * arrays, x_eval[m] physical points -> pred[m] and dudx[m] = (u_{e+1}-u_e)/h of the
 * element e = clamp(searchsorted(grid,x)-1, 0, n-2) (either output may be NULL).
 * dudx is the explicit, differentiable replacement for the reference's
 * autograd.grad(u, xq, create_graph=True) (examples/example3.py:56).           */
int hfem_line2_eval_fwd(int device, const double *grid, const double *u, int64_t n,
                        const double *x_eval, int64_t m, double *pred, double *dudx,
                        void *stream);
/* Backward: cot[m] (d/dpred), cot_dudx[m] (d/d dudx, may be NULL) -> ACCUMULATES
 * ggrid[n], gu[n]; writes gx_eval[m] (may be NULL).                            */
int hfem_line2_eval_bwd(int device, const double *grid, const double *u, int64_t n,
                        const double *x_eval, int64_t m, const double *cot,
                        const double *cot_dudx, double *ggrid, double *gu, double *gx_eval,
                        void *stream);
/* Fused 1D bar energy of examples/example3.py:27-70 with detached quadrature
 * (SURVEY F8): xq,wq,bq [npts] constants.  ONE launch; loss_acc[0], ggrid[n],
 * gu[n] are all ACCUMULATED (caller zeroes; ggrid/gu may be NULL).              */
int hfem_bar_energy(int device, const double *grid, const double *u, int64_t n,
                    const double *xq, const double *wq, const double *bq, int64_t npts,
                    double E, double *loss_acc, double *ggrid, double *gu, void *stream);
/* Fused L2-projection loss mean((pred-target)^2) of examples/example1.py:38 with
 * its backward in one launch: loss_acc, ggrid, gu ACCUMULATED (caller zeroes).  */
int hfem_line2_mse(int device, const double *grid, const double *u, int64_t n,
                   const double *x_eval, const double *target, int64_t m, double *loss_acc,
                   double *ggrid, double *gu, void *stream);

/* RECT-Q4 bilinear interpolation on the tensor-product grid, src/models.py:180-212:
 * gx[nx], gy[ny], u[nx][ny] (u_full, i.e. after where(node_mask,u_fixed,u)),
 * x_eval [m][2] physical -> pred[m].                                           */
int hfem_rectq4_eval_fwd(int device, const double *gx, int64_t nx, const double *gy,
                         int64_t ny, const double *u, const double *x_eval, int64_t m,
                         double *pred, void *stream);
/* Backward: cot[m] -> ACCUMULATES ggx[nx], ggy[ny], gu[nx][ny]; writes
 * gx_eval[m][2] (may be NULL).                                                 */
int hfem_rectq4_eval_bwd(int device, const double *gx, int64_t nx, const double *gy,
                         int64_t ny, const double *u, const double *x_eval, int64_t m,
                         const double *cot, double *ggx, double *ggy, double *gu,
                         double *gx_eval, void *stream);
/* Fused 2D L2-projection loss mean((pred-target)^2) of examples/example2.py:45-46
 * with its backward in one launch: loss_acc, ggx, ggy, gu ACCUMULATED.         */
int hfem_rectq4_mse(int device, const double *gx, int64_t nx, const double *gy, int64_t ny,
                    const double *u, const double *x_eval, const double *target, int64_t m,
                    double *loss_acc, double *ggx, double *ggy, double *gu, void *stream);

/* Float-row twins of the 1D / structured entry points above, for models in the reference's default dtype
 * (torch.float32: src/models.py:36-40, 142; examples 1-3 as shipped): every array argument is float -- parameters,
 * points, targets, per-point outputs, gradient accumulators and the loss scalar.  Inputs are widened on load, the
 * arithmetic in between is fp64, per-point outputs are rounded once on store.  The ACCUMULATED outputs (ggrid, gu, ggx,
 * ggy, loss_acc) are float atomics: every contribution is rounded when it is added and the order varies -- the last
 * bits are not reproducible (unlike hfem_tri3_energy_plan_f32, whose gradient rows are summed in fp64 and rounded once).
 * No widening copies on either side of the call.  The scratch of the *_ws forms (cum, ws) stays fp64.           */
int hfem_grid_param_fwd_f32(int device, const float *p, int64_t n, double x0, double xN, const uint8_t *mask,
                            const float *initial, float *grid, void *stream);
int hfem_grid_param_bwd_f32(int device, const float *p, int64_t n, double x0, double xN, const uint8_t *mask,
                            const float *ggrid, float *gp, void *stream);
int hfem_grid_param_fwd_ws_f32(int device, const float *p, int64_t n, double x0, double xN, const uint8_t *mask,
                               const float *initial, float *grid, double *cum, double *ws, void *stream);
int hfem_grid_param_bwd_ws_f32(int device, const float *p, int64_t n, double x0, double xN, const uint8_t *mask,
                               const float *ggrid, const double *cum, float *gp, double *ws, void *stream);
int hfem_line2_eval_fwd_f32(int device, const float *grid, const float *u, int64_t n, const float *x_eval, int64_t m,
                            float *pred, float *dudx, void *stream);
int hfem_line2_eval_bwd_f32(int device, const float *grid, const float *u, int64_t n, const float *x_eval, int64_t m,
                            const float *cot, const float *cot_dudx, float *ggrid, float *gu, float *gx_eval, void *stream);
int hfem_bar_energy_f32(int device, const float *grid, const float *u, int64_t n, const float *xq, const float *wq,
                        const float *bq, int64_t npts, double E, float *loss_acc, float *ggrid, float *gu, void *stream);
int hfem_line2_mse_f32(int device, const float *grid, const float *u, int64_t n, const float *x_eval, const float *target,
                       int64_t m, float *loss_acc, float *ggrid, float *gu, void *stream);
int hfem_rectq4_eval_fwd_f32(int device, const float *gx, int64_t nx, const float *gy, int64_t ny, const float *u,
                             const float *x_eval, int64_t m, float *pred, void *stream);
int hfem_rectq4_eval_bwd_f32(int device, const float *gx, int64_t nx, const float *gy, int64_t ny, const float *u,
                             const float *x_eval, int64_t m, const float *cot, float *ggx, float *ggy, float *gu,
                             float *gx_eval, void *stream);
int hfem_rectq4_mse_f32(int device, const float *gx, int64_t nx, const float *gy, int64_t ny, const float *u,
                        const float *x_eval, const float *target, int64_t m, float *loss_acc, float *ggx, float *ggy,
                        float *gu, void *stream);

/* ------------------------------------------------------------------ frozen-mesh displacement solve (TRI3 and QUAD4)
 * Matrix-free preconditioned conjugate gradients for u_free at FIXED coordinates (hidenn_fem_amd/solve.py; no reference
 * counterpart -- the reference reaches this minimum only by iterating Adam / L-BFGS on the energy).  The energy is exactly
 * quadratic in u there, E(u) = 1/2 u^T K u - f^T u, so K p = dE/du(p) with no forces and r = -dE/du(u): the caller
 * forms g0 = dE/du(u0) and g_zero = dE/du(u_free = 0) with hfem_tri3_energy_plan (fp64 rows, the forces of its loss) and
 * the solver never sees the forces.  Paired-slot TRI3 plans (the default), or QUAD4 plans as hfem_quad4_energy_plan_ex takes
 * them (g0 / g_zero from that entry point, W is not read -- the 2x2 rule's weights are 1).  The driver -- the vector
 * kernels, the status record, the halt logic -- is csrc/cg.hip and knows no element; q = K p and the Jacobi blocks are the
 * element kernels of csrc/tri3_cg.hip or csrc/quad4_cg.hip.  All vectors are fp64 free u rows [n_u][2]
 * in the plan's storage order.  Two launches per iteration: q = K p with p = z + beta p_old formed in
 * the gather, then u += alpha p, r -= alpha q, z = D^-1 r; alpha, beta and the stopping test |r|_2 <= max(rtol |f|_2, atol)
 * are reduced on the device in a fixed order.  Once halted (converged, max_iter, breakdown: p^T K p <= 0 or a non-finite
 * scalar) later iterations do nothing on the device: u keeps the last good iterate.
 *   create   flags: HFEM_FLAG_PHYSICAL_GRAD or 0 (the gradient convention of K).  The plan must outlive the solver.
 *   setup    binds the coordinate rows (fp64; they must stay allocated and unchanged while iterating) and the material, and
 *            builds the preconditioner: precond 1 = block Jacobi (2x2 diagonal blocks of K), 0 = none.  diag_out [n_u][3]
 *            (may be NULL): the blocks {K_xx, K_xy, K_yy}.
 *   start    r = -g0, z = D^-1 r, |f| = |g_zero|; resets the status record.
 *   iterate  n_iter iterations on u_free (launch only: capturable in a hipGraph).
 *   status   synchronises the stream; status_host[16] = {iterations, |r|, |f|, rho = r^T z, reason (0 running, 1 rtol,
 *            2 atol, 3 max_iter, 4 breakdown), alpha, beta, p^T K p, tolerance, max_iter, halted, ...}.
 *   apply    standalone q = K p (fixed rows read as 0) and pq_out[0] = p^T q on the device; not during iterate.   */
typedef struct hfem_cg hfem_cg;
int hfem_cg_create(hfem_plan *plan, int64_t n_u, int32_t flags, hfem_cg **out);
int hfem_cg_destroy(hfem_cg *cg);
int hfem_cg_setup(hfem_cg *cg, const double *x_free, const double *x_fixed, const double mat[4], double W, int32_t precond,
                  double *diag_out, void *stream);
int hfem_cg_start(hfem_cg *cg, const double *g0, const double *g_zero, double rtol, double atol, int64_t max_iter,
                  void *stream);
int hfem_cg_iterate(hfem_cg *cg, double *u_free, int32_t n_iter, void *stream);
int hfem_cg_status(hfem_cg *cg, double *status_host, void *stream);
int hfem_cg_apply(hfem_cg *cg, const double *p, double *q, double *pq_out, void *stream);

/* ------------------------------------------------------------------ Newton-Krylov on the Neo-Hookean tangent (TRI3, QUAD4)
 * The same driver with a third element kind (csrc/tri3_hyper_cg.hip; hidenn_fem_amd/newton.py): K is the tangent
 * K_T = d2Pi/du2 of hfem_tri3_hyper_energy_plan's potential at a linearisation point u_lin, on that entry point's plan (TRI3,
 * ONE element per slot), so the residual launch and the operator share a plan and its row maps.  Per element, with T = F^-T,
 * L = log1p(j) and dH = dG Jg^-1:  dP = mu dH + (mu - lambda L) T dH^T T + lambda (T : dH) T,  q = |det Jg| W dP Jg^-T; dead
 * loads do not enter.  An element with J <= 0 contributes a ZERO block and is counted.  K_T may be indefinite: the driver's
 * breakdown halt (p^T K p <= 0, before u moves) is then the truncation rule of truncated Newton, and a diagonal block that is
 * not positive definite is the identity in the block-Jacobi preconditioner.
 * A QUAD4 plan (the model's own, the one hfem_quad4_hyper_energy_plan takes) selects the fourth element kind
 * (csrc/quad4_hyper_cg.hip): the tangent of that entry point's potential, the same dP at each of the 2x2 Gauss points with
 * A = |det J_q|, spread through grad_xi N_k(xi_q).  A cell with j_q <= -1 at ANY point contributes a zero block and is counted
 * once; min J is taken over all points.  For a QUAD4 plan setup_hyper's block launch also stores mu - lambda log1p(j_q) of
 * every slot and point in the solver's own allocation (32 bytes per slot of the plan); apply and iterate read it, so they
 * evaluate the tangent at the point setup_hyper last saw.
 *   create_hyper  a paired or host-only plan, a QUAD4 plan without its fourth-corner records, or a tile that needs more than
 *                 64 KiB of LDS in either kernel (apply: 48 bytes per local node + 16 per owned row; blocks: 32 + 24), is an
 *                 argument error.
 *   setup_hyper   binds the coordinate rows, the linearisation point's rows (u_lin_free [n_u][2], u_fixed; fp64, they must
 *                 stay allocated and unchanged while iterating) and lame[2] = (lambda, mu) (host), W (the sum of the triangle
 *                 weights; not read for a QUAD4 plan, whose 2x2 weights are 1, as in hfem_cg_setup), and builds the
 *                 preconditioner at u_lin: precond 1 = block Jacobi, 0 = none.  diag_out [n_u][3] (may be NULL): the blocks;
 *                 info_out[2] (device, may be NULL) = {min J, number of elements with J <= 0} at u_lin.  Pointers are bound,
 *                 not copied: writing a new point into the same buffers and calling setup_hyper again re-linearises, and a
 *                 captured hfem_cg_iterate graph stays valid.
 * hfem_cg_start / iterate / status / apply / start_amg / iterate_amg work on such a solver unchanged; hfem_cg_setup refuses
 * it, and hfem_cg_setup_hyper refuses a solver of hfem_cg_create.
 *   setup_hyper_shifted  setup_hyper for the operator A(u) = c_k K_T(u) + c_m M of an implicit finite-strain Newmark step
 *                 (DESIGN 27): the same bindings and checks, c_k and c_m as hfem_cg_setup_shifted (finite, >= 0, not both zero;
 *                 c_k = 0 is the pure mass operator; c_m includes the density; lumped != 0: the row-sum mass).  The MASS
 *                 instances of the tangent kernels: c_k scales lambda and mu on the host (K_T is linear in them), the mass term
 *                 is formed in the slot loop from the corner rows the element already holds, always with |det J| of the
 *                 coordinates.  An inverted element contributes zeros to K_T and its full mass to M; info_out is setup_hyper's.
 *                 diag_out: the blocks of A.  An argument error leaves the solver as it was.  A later setup_hyper returns it to
 *                 plain K_T; hfem_cg_setup_shifted keeps refusing such a solver.                                           */
int hfem_cg_create_hyper(hfem_plan *plan, int64_t n_u, hfem_cg **out);
int hfem_cg_setup_hyper_shifted(hfem_cg *cg, const double *x_free, const double *x_fixed, const double *u_lin_free,
                                const double *u_fixed, const double lame[2], double W, double c_k, double c_m, int32_t lumped,
                                int32_t precond, double *diag_out, double *info_out, void *stream);
int hfem_cg_setup_hyper(hfem_cg *cg, const double *x_free, const double *x_fixed, const double *u_lin_free,
                        const double *u_fixed, const double lame[2], double W, int32_t precond, double *diag_out,
                        double *info_out, void *stream);

/* ------------------------------------------------------------------ mesh validity for r-adaptivity (TRI3)
 * What keeps a coordinate update valid (hidenn_fem_amd/radapt.py; no reference counterpart -- the reference's example 4
 * moves the nodes with L-BFGS unguarded and calls a mesh_quality_loss it never defines).  One thread per element over the
 * int32 connectivity conn [ne][3] (caller numbering); corner rows through the x row map x_src [nn] (>= 0: x_free row,
 * < 0: x_fixed row -1 - x_src), so any storage row order works.  x_free / x_fixed / x_ref rows are fp64 (plain) or fp32
 * (_f32); the arithmetic is fp64.  detJ = (x0-x2)(y1-y2) - (x1-x2)(y0-y2); the signed mean-ratio quality is
 * q = 4 sqrt(3) s A / (|e1|^2 + |e2|^2 + |e3|^2), s = sign of detJ on x_ref (the model's initial coordinates, [nn][2] by node
 * id): q in (0, 1] for a valid element, <= 0 for an inverted one, whatever the mesh's orientation.
 *   mesh_measure     q_out [ne], ratio_out [ne] = detJ / detJ_ref (both may be NULL); summary_out [3] (device) = {min q,
 *                    min ratio, number of inverted elements (s detJ <= 0)}.  Deterministic (order-independent reductions).
 *   step_bound       d [n_x][2] fp64 over the free rows (fixed rows move by 0), eta in (0, 1): alpha_out [1] (device) = the
 *                    smallest alpha > 0 with detJ(x + alpha d) = eta detJ(x) over all elements, +inf if there is none
 *                    (0 for an element with detJ(x) = 0).  detJ(x + alpha d) is an exact quadratic in alpha; stable roots.
 *                    Deterministic; launch-only (capturable in a hipGraph).
 *   quality_barrier  ACCUMULATES value_acc[0] += Q = (weight / ne) sum_e (1/q_e - 1) and grad_acc [n_x][2] += dQ/dx_free
 *                    (either may be NULL; fixed rows get nothing).  fp64 atomics: not deterministic in the last bits.
 *                    Finite for valid elements only.                                                                   */
int hfem_tri3_mesh_measure(int device, const int32_t *conn, int64_t ne, const int32_t *x_src, const double *x_free,
                           const double *x_fixed, const double *x_ref, double *q_out, double *ratio_out, double *summary_out,
                           void *stream);
int hfem_tri3_mesh_measure_f32(int device, const int32_t *conn, int64_t ne, const int32_t *x_src, const float *x_free,
                               const float *x_fixed, const float *x_ref, double *q_out, double *ratio_out,
                               double *summary_out, void *stream);
int hfem_tri3_step_bound(int device, const int32_t *conn, int64_t ne, const int32_t *x_src, const double *x_free,
                         const double *x_fixed, const double *d, double eta, double *alpha_out, void *stream);
int hfem_tri3_step_bound_f32(int device, const int32_t *conn, int64_t ne, const int32_t *x_src, const float *x_free,
                             const float *x_fixed, const double *d, double eta, double *alpha_out, void *stream);
int hfem_tri3_quality_barrier(int device, const int32_t *conn, int64_t ne, const int32_t *x_src, const double *x_free,
                              const double *x_fixed, const double *x_ref, double weight, double *value_acc, double *grad_acc,
                              void *stream);
int hfem_tri3_quality_barrier_f32(int device, const int32_t *conn, int64_t ne, const int32_t *x_src, const float *x_free,
                                  const float *x_fixed, const float *x_ref, double weight, double *value_acc,
                                  double *grad_acc, void *stream);

/* ------------------------------------------------------------------ mesh validity for r-adaptivity (QUAD4)
 * The bilinear-cell twins of the TRI3 entry points above (csrc/mesh_guard.hip; Quad4RAdaptiveSolver in
 * hidenn_fem_amd/radapt.py): the same argument lists, row maps, row types and argument checks, over conn [ne][4] (local nodes
 * counter-clockwise, neighbour indices mod 4).  Corner cross product c_k = (X_k+1 - X_k) x (X_k-1 - X_k) = 4 detJ at corner k;
 * detJ is affine over the reference square, so a cell is valid everywhere iff all four s c_k > 0, s = sign of c_0 + c_2 (twice
 * the signed area) on x_ref.  q_k = 2 s c_k / (|X_k+1 - X_k|^2 + |X_k-1 - X_k|^2) (1 at a right-angled corner with equal
 * sides), q = min_k q_k.
 *   mesh_measure     q_out [ne] = q, ratio_out [ne] = min_k c_k / c_k_ref (both may be NULL); summary_out [3] (device) = {min q,
 *                    min ratio, number of inverted elements (some s c_k <= 0)}.  Deterministic.
 *   step_bound       alpha_out [1] (device) = the smallest alpha > 0 at which some corner of some element has
 *                    c_k(x + alpha d) = eta c_k(x) (exact quadratics; +inf if there is none, 0 for a corner with c_k(x) = 0).
 *                    Every Gauss-point detJ then keeps at least eta of its value.  Deterministic; launch-only.
 *   quality_barrier  ACCUMULATES value_acc[0] += Q = (weight / (4 ne)) sum_e sum_k (1/q_ek - 1) and grad_acc [n_x][2] +=
 *                    dQ/dx_free (either may be NULL).  fp64 atomics: not deterministic in the last bits.  Finite for valid
 *                    elements only.                                                                                     */
int hfem_quad4_mesh_measure(int device, const int32_t *conn, int64_t ne, const int32_t *x_src, const double *x_free,
                            const double *x_fixed, const double *x_ref, double *q_out, double *ratio_out, double *summary_out,
                            void *stream);
int hfem_quad4_mesh_measure_f32(int device, const int32_t *conn, int64_t ne, const int32_t *x_src, const float *x_free,
                                const float *x_fixed, const float *x_ref, double *q_out, double *ratio_out,
                                double *summary_out, void *stream);
int hfem_quad4_step_bound(int device, const int32_t *conn, int64_t ne, const int32_t *x_src, const double *x_free,
                          const double *x_fixed, const double *d, double eta, double *alpha_out, void *stream);
int hfem_quad4_step_bound_f32(int device, const int32_t *conn, int64_t ne, const int32_t *x_src, const float *x_free,
                              const float *x_fixed, const double *d, double eta, double *alpha_out, void *stream);
int hfem_quad4_quality_barrier(int device, const int32_t *conn, int64_t ne, const int32_t *x_src, const double *x_free,
                               const double *x_fixed, const double *x_ref, double weight, double *value_acc, double *grad_acc,
                               void *stream);
int hfem_quad4_quality_barrier_f32(int device, const int32_t *conn, int64_t ne, const int32_t *x_src, const float *x_free,
                                   const float *x_fixed, const float *x_ref, double weight, double *value_acc,
                                   double *grad_acc, void *stream);

/* ------------------------------------------------------------------ mesh validity for r-adaptivity at finite strain
 * The det F-safe step bound and the deformation measure (csrc/mesh_guard.hip;
 * HyperRAdaptiveSolver / Quad4HyperRAdaptiveSolver in hidenn_fem_amd/radapt.py).  The argument lists of the step_bound entry
 * points above plus the displacement rows after the coordinate rows: u_src [nn] the u row map (>= 0: row of u_free, < 0: row
 * -1 - u_src of u_fixed, the Dirichlet rows), u_free, u_fixed in the row type of the coordinates (either may be NULL when no
 * node maps to it, not both).  A coordinate step at fixed nodal u moves R(a) = detJ(X + a d) and D(a) = detJ(X + u + a d), and
 * det F(a) = D(a) / R(a).
 *   hyper_step_bound      alpha_out [1] (device) = the smallest alpha > 0 at which some element has R(alpha) = eta R(0) or
 *                         det F(alpha) = eta det F(0) (exact quadratics; +inf if there is none, 0 when some element has
 *                         R(0) D(0) <= 0 or NaN).  QUAD4: per corner, on the cross products c_k and c_k^def; below the bound
 *                         det F at every point of a cell stays at or above eta times the cell's smallest corner ratio
 *                         r_k = c_k^def / c_k before the step.  Deterministic; launch-only.
 *   deformation_measure   j_out [ne] (may be NULL) = det F of the element (QUAD4: min_k r_k); summary_out [2] (device) =
 *                         {min J, number of elements with J <= 0 or NaN}.  Deterministic.
 * Errors as for the entry points above: null pointers, ne outside [0, 2^31), eta outside (0, 1).                          */
int hfem_tri3_hyper_step_bound(int device, const int32_t *conn, int64_t ne, const int32_t *x_src, const double *x_free,
                               const double *x_fixed, const int32_t *u_src, const double *u_free, const double *u_fixed,
                               const double *d, double eta, double *alpha_out, void *stream);
int hfem_tri3_hyper_step_bound_f32(int device, const int32_t *conn, int64_t ne, const int32_t *x_src, const float *x_free,
                                   const float *x_fixed, const int32_t *u_src, const float *u_free, const float *u_fixed,
                                   const double *d, double eta, double *alpha_out, void *stream);
int hfem_tri3_deformation_measure(int device, const int32_t *conn, int64_t ne, const int32_t *x_src, const double *x_free,
                                  const double *x_fixed, const int32_t *u_src, const double *u_free, const double *u_fixed,
                                  double *j_out, double *summary_out, void *stream);
int hfem_tri3_deformation_measure_f32(int device, const int32_t *conn, int64_t ne, const int32_t *x_src, const float *x_free,
                                      const float *x_fixed, const int32_t *u_src, const float *u_free, const float *u_fixed,
                                      double *j_out, double *summary_out, void *stream);
int hfem_quad4_hyper_step_bound(int device, const int32_t *conn, int64_t ne, const int32_t *x_src, const double *x_free,
                                const double *x_fixed, const int32_t *u_src, const double *u_free, const double *u_fixed,
                                const double *d, double eta, double *alpha_out, void *stream);
int hfem_quad4_hyper_step_bound_f32(int device, const int32_t *conn, int64_t ne, const int32_t *x_src, const float *x_free,
                                    const float *x_fixed, const int32_t *u_src, const float *u_free, const float *u_fixed,
                                    const double *d, double eta, double *alpha_out, void *stream);
int hfem_quad4_deformation_measure(int device, const int32_t *conn, int64_t ne, const int32_t *x_src, const double *x_free,
                                   const double *x_fixed, const int32_t *u_src, const double *u_free, const double *u_fixed,
                                   double *j_out, double *summary_out, void *stream);
int hfem_quad4_deformation_measure_f32(int device, const int32_t *conn, int64_t ne, const int32_t *x_src, const float *x_free,
                                       const float *x_fixed, const int32_t *u_src, const float *u_free, const float *u_fixed,
                                       double *j_out, double *summary_out, void *stream);

/* ------------------------------------------------------------------ smoothed-aggregation AMG for the frozen-mesh solve
 * A symmetric V-cycle of smoothed aggregation over K_ff in 2x2 node blocks (hidenn_fem_amd/solve.py, precond="amg").
 * Host setup (amg.cpp, no GPU), once per mesh topology: conn [ne][npe] int32 (host_create: npe = 3, TRI3; host_create_ex: npe
 * 3 or 4, QUAD4 -- a cell's diagonal partners are neighbours), x_src / u_src [nn] the model's row maps (u_src < 0:
 * a Dirichlet node).  Builds the fine block pattern (diagonal + free neighbours through shared elements, sorted columns), the
 * node -> element fan with the block slots each corner writes to, the aggregation of every level (SA phases 1-3, no strength
 * filter, singletons merged into a neighbour's aggregate; until a level has <= 1500 dofs or stops shrinking) and the
 * symbolic products P = pattern(A) pattern(P_tent), R = P^T, A P and A_c = R A P.  Never reads coordinates.
 *   host_info   level -1: {levels, n_u, ne, fan entries, host setup ns, npe, 0, 0}; level l: {block rows, block size, A block
 *               nnz, aggregates (0 on the coarsest), P block nnz, AP block nnz, 0, 0}
 *   host_copy   *n_out = length of an int32 array, copied into out when out != NULL.  level -1: which 0 fan_ptr, 1 fan
 *               element, 2 fan corner, 3 fan slots [.][npe], 4 conn_u [ne][npe] (the u row code of every corner: u_src of the node);
 *               level l: 0 A row_ptr, 1 A columns, 2 A diagonal slot, 3 aggregate
 *               of each row, 4 P row_ptr, 5 P columns, 6 R row_ptr, 7 R columns (fine rows), 8 R -> P block index,
 *               9 AP row_ptr, 10 AP columns
 * Device hierarchy (tri3_amg.hip, fp64), from a host setup (which may be destroyed afterwards):
 *   assemble    level-0 A values (K_ff, 2x2 blocks, row-major, in the host pattern) at the coordinates x_free / x_fixed (fp64
 *               rows; mat, W as hfem_cg_setup).  One thread per row, no atomics: bit-deterministic.  A QUAD4 host setup
 *               selects the four-corner instance of the same kernel; everything below the assembly is the same code.
 *   setup       assemble + the numeric hierarchy (block-diagonal inverses, lambda_max(D^-1 A) by power iteration, tentative
 *               and smoothed prolongators, Galerkin products); writes the coarsest level as a dense row-major N x N matrix
 *               into coarse_out (an all-zero row gets a 1 on the diagonal).  The caller inverts it and hands the inverse
 *               over with set_coarse (the pointer must stay valid; it is read by every later cycle).
 *   vcycle      z = M r over the free u rows (fp64 [n_u][2]); launch-only.
 *   values      *n_out = length of a device fp64 array of level `level`, copied (device to device) into out when out != NULL:
 *               which 0 A blocks, 1 D^-1 blocks, 2 coefficients {lambda_hat, 1/theta, c1, c2, omega, ., ., .}, 3 near-null
 *               space [rows][bs][3], 4 P_tent [rows][bs][3], 5 P blocks [bs][3]
 * The same hierarchy on the assembled Neo-Hookean tangent K_T,ff at (x, u) (newton.py, precond="amg_tangent"):
 *   assemble_hyper  level-0 A values = K_T,ff at the coordinates and the displacement rows u_free [n_u][2] / u_fixed (fp64;
 *               lame, W as hfem_cg_setup_hyper; QUAD4: W is not read).  The same walk, the element tangent of the hyper CG
 *               kernels; an inverted element or cell contributes zeros, so the matrix is exactly the operator hfem_cg_apply
 *               applies on a hyper handle.  Bit-deterministic.
 *   setup_hyper hfem_amg_setup with that assembly and with the fine near-null space at the deformed position (rotation
 *               column (-(y + v), x + u)).  K_T may be indefinite: the caller checks the coarsest matrix before it inverts it.
 * One handle may be set up by either entry point, in any order.  Pointers and patterns never change, only values: a captured
 * hfem_cg_iterate_amg graph stays valid across re-setups of either kind.
 * PCG with the V-cycle: cg_start_amg / cg_iterate_amg replace hfem_cg_start / hfem_cg_iterate (same status record, same
 * halting; hfem_cg_setup still binds the coordinates).  Four launch groups per iteration: apply, vector update, V-cycle,
 * r^T z.                                                                                                                */
typedef struct hfem_amg_host hfem_amg_host;
typedef struct hfem_amg hfem_amg;
int hfem_amg_host_create(const int32_t *conn, int64_t ne, int64_t nn, const int32_t *x_src, const int32_t *u_src,
                         hfem_amg_host **out);
int hfem_amg_host_create_ex(const int32_t *conn, int64_t ne, int32_t npe, int64_t nn, const int32_t *x_src,
                            const int32_t *u_src, hfem_amg_host **out);
int hfem_amg_host_destroy(hfem_amg_host *host);
int hfem_amg_host_info(const hfem_amg_host *host, int32_t level, int64_t info[8]);
int hfem_amg_host_copy(const hfem_amg_host *host, int32_t level, int32_t which, int32_t *out, int64_t *n_out);
int hfem_amg_create(int device, const hfem_amg_host *host, int32_t flags, hfem_amg **out);
int hfem_amg_destroy(hfem_amg *amg);
int hfem_amg_assemble(hfem_amg *amg, const double *x_free, const double *x_fixed, const double mat[4], double W, void *stream);
int hfem_amg_setup(hfem_amg *amg, const double *x_free, const double *x_fixed, const double mat[4], double W,
                   double *coarse_out, void *stream);
int hfem_amg_assemble_hyper(hfem_amg *amg, const double *x_free, const double *x_fixed, const double *u_free,
                            const double *u_fixed, const double lame[2], double W, void *stream);
int hfem_amg_setup_hyper(hfem_amg *amg, const double *x_free, const double *x_fixed, const double *u_free,
                         const double *u_fixed, const double lame[2], double W, double *coarse_out, void *stream);
int hfem_amg_set_coarse(hfem_amg *amg, const double *coarse_inv);
int hfem_amg_vcycle(hfem_amg *amg, const double *r, double *z, void *stream);
int hfem_amg_values(hfem_amg *amg, int32_t level, int32_t which, double *out, int64_t *n_out, void *stream);
int hfem_cg_start_amg(hfem_cg *cg, hfem_amg *amg, const double *g0, const double *g_zero, double rtol, double atol,
                      int64_t max_iter, void *stream);
int hfem_cg_iterate_amg(hfem_cg *cg, hfem_amg *amg, double *u_free, int32_t n_iter, void *stream);

/* ------------------------------------------------------------------ Cauchy stress recovery and a ZZ indicator at finite strain
 * No reference counterpart.  The arrays, the points, the weights (on the REFERENCE configuration), the adjacency and the
 * lumped projection of hfem_*_stress_recover / hfem_*_zz_error, with the stress of the Neo-Hookean material of
 * hfem_*_hyper_energy_plan: lame[2] = (lambda, mu) (HOST pointer, mu > 0 and lambda + mu > 0), per point H = G J^-1 (always the
 * physical gradient), j = tr H + det H (= det F - 1), L = log1p(j) and the Cauchy stress
 *   sigma_h = (mu (H + H^T + H H^T) + lambda L I) / (1 + j)  ->  (sxx, syy, sxy).
 * S = C0^-1 with C0 the linearisation at F = I (c11 = c22 = lambda + 2 mu, c12 = lambda, c33 = mu): an INDICATOR, not an
 * estimate, away from small strain.  nodal_J[Nn] (optional, NULL) = the same projection of 1 + j.
 * An element is inverted when j <= -1 or j is NaN at any of its points: it is evaluated at j = 0, has weight 0 in the projection
 * (a node with no other element gets zeros and area 0), eta2 = +inf and norm2 = 0.
 * totals[4] = {sum eta2, sum norm2, min over all points of 1 + j, number of inverted elements}; partials: caller-owned workspace of
 * 4 * ceil(Ne / 256) doubles.  Launch-only (capturable).  Ne == 0 (or Nn == 0) returns 0 without touching a device. */
int hfem_tri3_hyper_stress_recover(int device, const double *X, const double *U, const int32_t *conn, int64_t ne, int64_t nn,
                                   const int32_t *adj_ptr, const int32_t *adj, const double lame[2], double *nodal_stress,
                                   double *nodal_J, double *nodal_area, void *stream);
int hfem_quad4_hyper_stress_recover(int device, const double *X, const double *U, const int32_t *conn, int64_t ne, int64_t nn,
                                    const int32_t *adj_ptr, const int32_t *adj, const double lame[2], double *nodal_stress,
                                    double *nodal_J, double *nodal_area, void *stream);
int hfem_tri3_hyper_zz_error(int device, const double *X, const double *U, const int32_t *conn, int64_t ne,
                             const double *nodal_stress, const double lame[2], double *eta2, double *norm2, double *partials,
                             double *totals, void *stream);
int hfem_quad4_hyper_zz_error(int device, const double *X, const double *U, const int32_t *conn, int64_t ne,
                              const double *nodal_stress, const double lame[2], double *eta2, double *norm2, double *partials,
                              double *totals, void *stream);

/* ------------------------------------------------------------------ free-vibration modes: mass operator and block-vector kernels
 * (csrc/modal.hip; hidenn_fem_amd/modal.py).  K_ff phi = lambda M_ff phi by block LOBPCG; K_ff is what hfem_cg_apply
 * applies.  fp64; a block vector is [m][n_u][2]: every vector contiguous in the storage order of u_free, so a slice is what
 * hfem_cg_apply / hfem_amg_vcycle take.  `len` = 2 n_u doubles of one vector (even).  Every entry point is bitwise reproducible
 * (fixed-order sums, no floating-point atomics), checks its arguments before it touches a device (negative codes, message through
 * hfem_last_error) and only enqueues launches on `stream`.
 *   mass_apply   MV[k] = M_ff V[k], k < m <= 8, matrix-free: one thread per free u row walks the row's node fan (adj_ptr / adj:
 *                the node -> (element, corner) CSR of the stress recovery, entries e << 2 | c, ascending e) and forms each
 *                element's mass row from X [nn][2] (coordinates by node id).  npe 3: rho |det J| / 24 (1 + delta_ab); npe 4:
 *                rho sum_q N_a N_b |det J_q| over the 2x2 Gauss points; lumped != 0: the row sum on the diagonal.  M x I_2, unit
 *                thickness, always |det J|.  row_node [n_u]: node id of every row; node_row [nn]: row of every node, -1 for a
 *                Dirichlet node (contributes 0).  MV must not alias V.
 *   block_gram   G [ma][mb] = A B^T, A [ma][len], B [mb][len], ma, mb <= 24; one pass with per-workgroup partials (at least
 *                HFEM_BLOCK_GRAM_PARTIALS doubles) and a fixed-order finish into the device matrix G.
 *   block_combine  Out[j] = sum_i C[i][j] S[i]: S [ms][len], C [ms][mo] row-major on the device, Out [mo][len], ms, mo <= 24;
 *                Out must not overlap S.
 *   block_residual  R[k] = KX[k] - lambda[k] MX[k], k < m <= 8 (lambda on the device); norms[2k] = |R_k|_2, norms[2k + 1] =
 *                |MX_k|_2 on the device; partials: at least HFEM_BLOCK_RESIDUAL_PARTIALS doubles.
 *   block_jacobi_apply  W[k] = D^-1 R[k], D the 2x2 blocks {K_xx, K_xy, K_yy} of hfem_cg_setup's diag_out [n_u][3]; W may be R.
 */
#define HFEM_BLOCK_GRAM_PARTIALS 73728
#define HFEM_BLOCK_RESIDUAL_PARTIALS 16384
int hfem_mass_apply(int device, int32_t npe, const double *X, const int32_t *conn, int64_t ne, int64_t nn, const int32_t *adj_ptr,
                    const int32_t *adj, const int32_t *row_node, const int32_t *node_row, int64_t n_u, double rho, int32_t lumped,
                    const double *V, int32_t m, double *MV, void *stream);
int hfem_block_gram(int device, const double *A, int32_t ma, const double *B, int32_t mb, int64_t len, double *partials, double *G,
                    void *stream);
int hfem_block_combine(int device, const double *S, int32_t ms, const double *C, int32_t mo, int64_t len, double *Out, void *stream);
int hfem_block_residual(int device, const double *KX, const double *MX, const double *lambda, int32_t m, int64_t len, double *R,
                        double *partials, double *norms, void *stream);
int hfem_block_jacobi_apply(int device, const double *diag, const double *R, int32_t m, int64_t len, double *W, void *stream);

/* ------------------------------------------------------------------ implicit transient dynamics: Newmark on A = c_M M + c_K K
 * (the MASS instances of the kernels of csrc/tri3_cg.hip, csrc/quad4_cg.hip and csrc/tri3_amg.hip; csrc/dynamics.hip;
 * hidenn_fem_amd/dynamics.py).  No reference counterpart.  M u'' + C u' + K u = load(t) b0 over the free u rows, C = alpha_R M + beta_R K, Newmark (beta, gamma) in the
 * a-form: per step one solve A a+ = load b0 - K w - alpha_R M v~ with A = c_M M + c_K K, c_M = 1 + gamma dt alpha_R,
 * c_K = beta dt^2 + gamma dt beta_R.  K is hfem_cg_apply's operator, M hfem_mass_apply's (always |det J|).
 *   cg_setup_shifted   hfem_cg_setup for the shifted operator (the MASS instances of the plain element kernels): binds the coordinate rows and the material
 *                as hfem_cg_setup does, and c_k >= 0, c_m >= 0 (c_m INCLUDES the density; both finite, not both zero), lumped != 0:
 *                the row-sum mass.  diag_out [n_u][3] (may be NULL): the 2x2 diagonal blocks of A (the mass on xx and yy).  After
 *                it hfem_cg_start / iterate / status / apply / start_amg / iterate_amg work on A; a later hfem_cg_setup returns
 *                the solver to plain K.  The mass term is formed in the slot loop of the apply from the corner rows the element
 *                already holds.  A solver of hfem_cg_create_hyper is refused.
 *   amg_assemble_shifted / amg_setup_shifted   hfem_amg_assemble / hfem_amg_setup with the fine level A_ff = c_k K_ff + c_m M_ff
 *                (one thread per row, no atomics: bit-deterministic); near-null space and coarse inverse as hfem_amg_setup.
 *   newmark_predict  u_pred = u + dt v + dt^2 (1/2 - beta) a, v_pred = v + dt (1 - gamma) a, w = u_pred + beta_r v_pred.
 *   newmark_rhs      rhs = load b0 - kw - alpha_r mv (mv may be NULL: no such term); g_zero = rhs, g0 = aa - rhs with aa = A a of
 *                the warm start a: the two vectors hfem_cg_start takes.
 *   newmark_correct  u = u_pred + beta dt^2 a, v = v_pred + gamma dt a (u may be u_pred, v may be v_pred).
 *   newmark_trial    (finite strain) a_t = a + s d, u_t = u_pred + c_k a_t, ma_t = ma + s md in one pass: the trial
 *                state of a Newton line search with M a carried along (ma = M a, md = M d).  a_t may be a, ma_t may be ma.
 *   newmark_residual (finite strain) r = c_m ma + alpha_r mv + f_int - load b_ext (mv may be NULL: no such term), neg_r = -r (may
 *                be NULL).  hfem_cg_start with g0 = g_zero = r starts the Newton system A d = -r; neg_r is its right-hand side
 *                as a vector (what hfem_block_jacobi_apply takes where A is block diagonal).
 * The five vector entry points work on fp64 rows, len = 2 n_u doubles (even), are elementwise (a few FMAs per entry:
 * bitwise reproducible), launch-only (capturable) and check their arguments before they touch a device. */
int hfem_cg_setup_shifted(hfem_cg *cg, const double *x_free, const double *x_fixed, const double mat[4], double W, double c_k,
                          double c_m, int32_t lumped, int32_t precond, double *diag_out, void *stream);
int hfem_amg_assemble_shifted(hfem_amg *amg, const double *x_free, const double *x_fixed, const double mat[4], double W,
                              double c_k, double c_m, int32_t lumped, void *stream);
int hfem_amg_setup_shifted(hfem_amg *amg, const double *x_free, const double *x_fixed, const double mat[4], double W, double c_k,
                           double c_m, int32_t lumped, double *coarse_out, void *stream);
int hfem_newmark_predict(int device, const double *u, const double *v, const double *a, int64_t len, double dt, double beta,
                         double gamma, double beta_r, double *u_pred, double *v_pred, double *w, void *stream);
int hfem_newmark_rhs(int device, const double *b0, const double *kw, const double *mv, const double *aa, int64_t len, double load,
                     double alpha_r, double *g0, double *g_zero, void *stream);
int hfem_newmark_correct(int device, const double *u_pred, const double *v_pred, const double *a, int64_t len, double dt,
                         double beta, double gamma, double *u, double *v, void *stream);
int hfem_newmark_trial(int device, const double *a, const double *d, const double *u_pred, const double *ma, const double *md,
                       int64_t len, double s, double c_k, double *a_t, double *u_t, double *ma_t, void *stream);
int hfem_newmark_residual(int device, const double *ma, const double *mv, const double *f_int, const double *b_ext, int64_t len,
                          double c_m, double alpha_r, double load, double *r, double *neg_r, void *stream);

/* ------------------------------------------------------------------ linearised buckling: the geometric stiffness operator
 * (csrc/buckling.hip; hidenn_fem_amd/buckling.py).  (K + lambda K_G(sigma_0)) phi = 0 as K_G phi = theta K phi,
 * theta = -1 / lambda, by the block LOBPCG of the modal entry points above with K_G in the role of K and K in the role of M.
 * No reference counterpart.
 *   v^T K_G v = sum_e sum_q w_q |det J_q| sum_{i in x, y} (grad v_i)^T S_0(q) (grad v_i),  S_0 = [[s_xx, s_xy], [s_xy, s_yy]],
 *   sigma = C eps(u_0) at the point; grad is the shape-function gradient of the convention (flags: HFEM_FLAG_PHYSICAL_GRAD or 0,
 *   as hfem_cg_create), npe 3: constant gradients and the weight W |det J| (mat, W as hfem_cg_setup), npe 4: the 2x2 Gauss rule
 *   with weights 1 (W is not read for the weights but must be > 0).  K_G acts per component (G x I_2).  fp64, bitwise
 *   reproducible (no floating-point atomics, fixed-order sums); arguments are checked before a device is touched (negative codes,
 *   message through hfem_last_error); launches only.
 *   geom_setup   G [ne][npe][npe] (full rows, row-major): G_e[a][b] = sum_q w_q |det J_q| (g_a . S_0 g_b).  One thread per
 *                element.  X [nn][2]: coordinates by node id; u_0 of a node n: u_free[node_row[n]] where node_row[n] >= 0, else
 *                u_fixed[fixed_row[n]] (u_free [n_u][2], u_fixed [n_fix][2]; node_row, fixed_row [nn]; an index outside its
 *                table reads as 0).
 *   geom_apply   GV[k] = K_G V[k], k < m <= 8, over the free u rows: one thread per row walks the row's node fan (adj_ptr / adj,
 *                row_node, node_row as hfem_mass_apply), reads row c of G_e and gathers the columns at the element's corners
 *                (node_row -1 = Dirichlet: contributes 0).  One launch per call, in a register tile of 1, 2, 4 or 8 columns (a
 *                ragged tile reads its last column again and does not store the surplus).  GV must not alias V.             */
int hfem_geom_setup(int device, int32_t npe, int32_t flags, const double *X, const int32_t *conn, int64_t ne, int64_t nn,
                    const double *u_free, int64_t n_u, const double *u_fixed, int64_t n_fix, const int32_t *node_row,
                    const int32_t *fixed_row, const double mat[4], double W, double *G, void *stream);
int hfem_geom_apply(int device, int32_t npe, const double *G, const int32_t *conn, int64_t ne, int64_t nn, const int32_t *adj_ptr,
                    const int32_t *adj, const int32_t *row_node, const int32_t *node_row, int64_t n_u, const double *V, int32_t m,
                    double *GV, void *stream);

/* ------------------------------------------------------------------ harmonic frequency response: complex shifted operator and COCG
 * (csrc/harmonic.hip; hidenn_fem_amd/harmonic.py).  No reference counterpart.  The steady state of
 * M u'' + C u' + K u = Re(b e^{i w t}), C = alpha_R M + beta_R K (+ structural damping i eta K), over the free u rows:
 *   A x = b,   A = z_k K + z_m M,   z_k = 1 + i (w beta_R + eta),   z_m = rho (-w^2 + i w alpha_R)
 * K is hfem_cg_apply's operator, M hfem_mass_apply's at unit density (z_m INCLUDES the density), always |det J|.  A is complex
 * symmetric; its real part is indefinite above the first resonance.  A complex vector is an fp64 block vector [2][n_u][2]: plane
 * 0 real, plane 1 imaginary, each in the storage order of u_free (a plane is what hfem_amg_vcycle takes, both are what
 * hfem_block_jacobi_apply takes at m = 2); `len` = 4 n_u doubles.  The solver is preconditioned COCG (conjugate orthogonal
 * conjugate gradients) with a REAL SPD preconditioner T applied to each plane: every inner product unconjugated, the stopping
 * test |r|_2 <= max(rtol |b|_2, atol) in the Hermitian norm; all scalars reduced and consumed on the device in a fixed order.
 * Once halted (converged, max_iter, breakdown: a non-finite scalar, or |p^T A p| = 0 or |r^T z| = 0 before x moves) later
 * launches write nothing: x keeps the last good iterate.  Launches per iteration: 3 (apply; update of x and r with z = T r,
 * rho, beta and the stopping test; p = z + beta p) with T = none or block Jacobi, 6 with AMG (apply; update; one V-cycle per
 * plane; rho and beta; p).
 *   create   plan and flags as hfem_cg_create (a paired TRI3 plan or a QUAD4 plan).  Refused: a host-only plan, the
 *            one-element-per-slot TRI3 plan of the Neo-Hookean tangent, and a plan with a tile whose apply needs more than 64 KiB
 *            of LDS:  48 x (max local nodes of a tile) + 32 x (max owned rows of a tile) + 8 x (2 x threads / 64 + 2) bytes,
 *            threads = 256 (512 for a 512-thread paired plan); the message carries the numbers.  The plan must outlive the solver.
 *   setup    binds the coordinate rows (fp64; they must stay allocated and unchanged while iterating), the material (mat, W as
 *            hfem_cg_setup: UNSCALED) and the mass kind (lumped != 0: the row sum), and stores zk[2] = (Re, Im) z_k, zm[2] =
 *            (Re, Im) z_m (HOST pointers) in device memory on `stream`: finite, not all zero, any sign.  A captured
 *            hfem_harm_iterate reads them there, so it stays valid across setups.
 *   apply    standalone Q = A P and pq_out[2] (device) = (Re, Im) of the unconjugated P^T Q; not during iterate.  Q != P.
 *   start    r = b - A x0 (x0 NULL: r = b), z = T r, p = z; resets the status record.  T: amg != NULL: one V-cycle of that
 *            hierarchy per plane (hfem_amg_setup_shifted on a REAL SPD operator, e.g. K + w^2 rho M); diag != NULL: the inverses
 *            of the 2x2 blocks diag [n_u][3] (hfem_cg_setup_shifted's diag_out; a block that is not positive definite is the
 *            identity); both NULL: none; both given is an argument error.
 *   iterate  n_iter > 0 iterations on x, which must hold x0 (zeros when x0 was NULL) at the first call after start; amg: the
 *            hierarchy start was given (NULL when it was given none).  Launch only: capturable in a hipGraph.
 *   status   synchronises the stream; status_host[16] = {iterations, |r|, |b|, Re rho, reason (0 running, 1 rtol, 2 atol,
 *            3 max_iter, 4 breakdown), Re alpha, Re beta, Re mu, tolerance, max_iter, halted, rtol-wins, Im rho, Im alpha, Im beta,
 *            Im mu}, rho = r^T z, mu = p^T A p, the last ones formed.
 * Every entry point checks its arguments before it touches a device (negative code, message through hfem_last_error).       */
typedef struct hfem_harm hfem_harm;
int hfem_harm_create(hfem_plan *plan, int64_t n_u, int32_t flags, hfem_harm **out);
int hfem_harm_destroy(hfem_harm *harm);
int hfem_harm_setup(hfem_harm *harm, const double *x_free, const double *x_fixed, const double mat[4], double W, const double zk[2],
                    const double zm[2], int32_t lumped, void *stream);
int hfem_harm_apply(hfem_harm *harm, const double *P, double *Q, int64_t len, double *pq_out, void *stream);
int hfem_harm_start(hfem_harm *harm, hfem_amg *amg, const double *diag, const double *b, const double *x0, int64_t len, double rtol,
                    double atol, int64_t max_iter, void *stream);
int hfem_harm_iterate(hfem_harm *harm, hfem_amg *amg, double *x, int64_t len, int32_t n_iter, void *stream);
int hfem_harm_status(hfem_harm *harm, double *status_host, void *stream);

/* ------------------------------------------------------------------ element-scaled stiffness K(w) = sum_e w_e K_e
 * (csrc/topopt.hip, csrc/cg.hip, csrc/tri3_amg.hip; hidenn_fem_amd/solve.py set_element_scale).  No reference
 * counterpart.  One weight per element -- two materials, or the SIMP interpolation of a density design -- through the
 * matrix-free PCG solve, the block-Jacobi blocks and the AMG fine level.
 *   hfem_cg_setup_scaled      hfem_cg_setup for K(w), for a solver of hfem_cg_create (a solver of hfem_cg_create_hyper is
 *                             refused).  w_slot (device, fp64): one weight record per slot of the solver's plan, n_tiles x
 *                             elem_stride records addressed as the plan's elem_pack: a paired TRI3 plan: two doubles {w_A, w_B};
 *                             a QUAD4 plan: one double (hfem_topt_weights writes it; hfem_topt_slots gives its length in
 *                             doubles).  The record of a slot without an element, and w_B of a slot with one element, are never
 *                             used.  w_slot is bound as a POINTER: it must stay allocated; writing new weights into the same
 *                             buffer and calling this again re-linearises (the blocks are rebuilt), and a captured
 *                             hfem_cg_iterate stays valid, as after hfem_cg_setup_hyper.  hfem_cg_start / iterate / status /
 *                             apply / start_amg / iterate_amg then work on K(w) unchanged.  A later hfem_cg_setup or
 *                             hfem_cg_setup_shifted returns the solver to the unscaled operator.  NULL w_slot: argument error.
 *   hfem_amg_assemble_scaled  hfem_amg_assemble / hfem_amg_setup with w_elem[ne] (device, fp64, by global element id: the row
 *   hfem_amg_setup_scaled     order of the connectivity hfem_amg_host_create_ex was given) multiplied into every element's
 *                             blocks.  One thread per row, no atomics: bit-reproducible.  The hierarchy's patterns and
 *                             aggregates are the mesh's and are not rebuilt, only the values.
 * The design handle maps a density design onto those weights and holds the density filter:
 *   create    plan: the solver's (a paired TRI3 plan or a QUAD4 plan, on a device); its elem_gid / elem_gid_b are uploaded.
 *             centroids[ne][2], volumes[ne] (HOST, fp64): the filter's geometry, read when radius > 0.  The filter's CSR is
 *             built here on the host with a uniform grid: per row e every j with H_ej = radius - |x_e - x_j| > 0, columns
 *             ascending, and s_e = sum_j H_ej v_j.  radius <= 0: the identity filter (centroids and volumes may be NULL).  More
 *             than 2^31 - 1 entries: argument error, the message gives the count.
 *   slots     doubles of a w_slot buffer of this plan (n_tiles x elem_stride, x 2 for a paired TRI3 plan); < 0 on NULL.
 *   weights   w_e = e_min + rho_f[e]^penal (1 - e_min) (penal >= 1, 0 <= e_min < 1; penal = 1, e_min = 0 passes rho_f
 *             through bit for bit): once by element id into w_elem[ne], once per slot into w_slot (entries without an element
 *             0).  Either output may be NULL.  One launch.
 *   filter    out = F in (transpose = 0: out_e = sum_j H_ej v_j in_j / s_e) or out = F^T in (transpose = 1:
 *             out_j = v_j sum_e H_je in_e / s_e); one thread per element gathers its row: bit-reproducible.  out != in.
 *   energy    one launch on the tile plan (the apply's gather and slot loop, no accumulation): at each element's home slot
 *             ce_out[e] = u_e^T K_e u_e (UNSCALED: twice the element's strain energy; mat, W, flags as hfem_cg_setup /
 *             hfem_cg_create) and, when dc_out is given, dc_out[e] = -penal rho_f[e]^(penal-1) (1 - e_min) ce_out[e].  Every
 *             element is written exactly once; fixed u rows read as 0.
 *   oc        the optimality-criteria update, launches only (capturable, no host synchronisation):
 *               rho_new,e(lambda) = clamp(rho_e sqrt(r_e / lambda), max(0, rho_e - move), min(1, rho_e + move)),
 *               r_e = max(0, -dc_e / dv_e),
 *             lambda by bisection so that V(lambda) = sum_e v_e (F rho_new(lambda))_e <= vol_target.  The bracket, the
 *             midpoint and every decision live in a device status record.  The upper end starts at R = max_e r_e (there no
 *             entry grows, so the update is feasible whenever the current design is); the first launch evaluates V there, and
 *             while it is not feasible the bracket moves up (lambda_lo = lambda_hi, lambda_hi x 4), one launch each.  Then one
 *             launch per halving at m = (lambda_lo + lambda_hi) / 2: V(m) <= vol_target moves lambda_hi, else lambda_lo; a
 *             bracket one ulp wide is left alone.  n_bisect + 1 step launches in all, each with the filter gather evaluating
 *             the neighbours' updates on the fly and V summed in block order by a ticket workgroup.  A last launch writes
 *             rho_new = the update at lambda_hi (the feasible end) and rho_f_new = F rho_new.  Needs a handle created with
 *             volumes.  rho_new, rho_f_new and rho must be three different buffers.
 *   status    synchronises the stream; status_host[16] = {lambda_lo, lambda_hi, V(lambda_hi), step launches that evaluated V,
 *             feasible (1: V(lambda_hi) <= vol_target was seen), phase (0 moving up, 1 halving), vol_target, R, V(lambda_lo),
 *             0 ...} of the last hfem_topt_oc.  V at an end of the bracket that was never evaluated is NaN: V(lambda_lo) while
 *             lambda_lo = 0, and V(lambda_hi) when the last launch moved the bracket up without reaching a feasible end
 *             (only with feasible = 0).
 * Every entry point checks its arguments before it touches a device (negative code, message through hfem_last_error).       */
typedef struct hfem_topt hfem_topt;
int hfem_cg_setup_scaled(hfem_cg *cg, const double *x_free, const double *x_fixed, const double mat[4], double W,
                         const double *w_slot, int32_t precond, double *diag_out, void *stream);
int hfem_amg_assemble_scaled(hfem_amg *amg, const double *x_free, const double *x_fixed, const double mat[4], double W,
                             const double *w_elem, void *stream);
int hfem_amg_setup_scaled(hfem_amg *amg, const double *x_free, const double *x_fixed, const double mat[4], double W,
                          const double *w_elem, double *coarse_out, void *stream);
int hfem_topt_create(hfem_plan *plan, const double *centroids, const double *volumes, int64_t ne, double radius, hfem_topt **out);
int hfem_topt_destroy(hfem_topt *topt);
int64_t hfem_topt_slots(const hfem_topt *topt);
int hfem_topt_weights(hfem_topt *topt, const double *rho_f, double penal, double e_min, double *w_elem, double *w_slot,
                      void *stream);
int hfem_topt_filter(hfem_topt *topt, const double *in, double *out, int32_t transpose, void *stream);
int hfem_topt_energy(hfem_topt *topt, const double *x_free, const double *x_fixed, const double *u_free, const double mat[4],
                     double W, int32_t flags, const double *rho_f, double penal, double e_min, double *ce_out, double *dc_out,
                     void *stream);
int hfem_topt_oc(hfem_topt *topt, const double *rho, const double *dc, const double *dv, double vol_target, double move,
                 int32_t n_bisect, double *rho_new, double *rho_f_new, void *stream);
int hfem_topt_status(hfem_topt *topt, double *status_host, void *stream);

/* ------------------------------------------------------------------ small-strain J2 elastoplasticity, TRI3, plane strain
 * (csrc/tri3_j2.hip, csrc/hfem_j2_dev.h, csrc/cg.hip; hidenn_fem_amd/plasticity.py).  No reference counterpart.
 * Rate-independent J2 plasticity with linear isotropic hardening: the closed-form radial return per element (TRI3 has one
 * state point) against a COMMITTED state, the incremental potential Pi whose gradient is the internal force, and the
 * consistent tangent as the PCG driver's J2 operator kind.  Physical gradient convention.  State per element, fp64:
 * {eps^p_xx, eps^p_yy, eps^p_xy (tensor components), alpha}; stress {s_xx, s_yy, s_xy, s_zz}; both by global element id (the
 * row order of the connectivity the plan was created from).
 *   hfem_j2_create    plan: a TRI3 plan with one element per slot (plan_elem_order 3: hfem_tri3_hyper_energy_plan's), on a
 *                     device; its elem_gid is uploaded.  mat = {mu, kappa, sigma_y, H} (mu, kappa, sigma_y > 0, H >= 0),
 *                     W the sum of the triangle weights.  Committed, trial and stress arrays start at zero (virgin).
 *   hfem_j2_slots     doubles of a tangent-record buffer of this plan: 5 x n_tiles x elem_stride; < 0 on NULL.
 *   hfem_j2_update    one element launch + a one-block reduction at u_free (fp64 rows; u_fixed: the Dirichlet rows):
 *                       out[3] = {Pi, plastic home elements, max dgamma},  g_out = dPi/du_free (every free row the plan owns),
 *                       Pi = sum_e A_e Psi_e + load g_ext . u_free,  g = A_e B^T sigma + load g_ext
 *                     g_ext (device, free rows; may be NULL: no external load): the gradient of the linear energy at u = 0 with
 *                     zero Dirichlet values, formed once by the caller; it is not recomputed here.  The committed state is
 *                     read by element id and never written.  write_state = 1: home slots also store the trial state and the
 *                     stress by element id.
 *   hfem_j2_commit    trial -> committed (a device copy).
 *   hfem_j2_get       out[ne][4] (device) = the committed (which = 0) or trial (1) state or the stress (2).
 *   hfem_j2_set       committed = trial = state[ne][4] (device); NULL: the virgin state.  The stress array is zeroed.
 *   hfem_cg_setup_j2  binds the J2 tangent on a solver of hfem_cg_create_hyper (TRI3 plan, the plan j2 was created on): the
 *                     linearisation launch runs the return map at u_lin_free against the committed state and writes one
 *                     tangent record {theta, theta_bar, n_xx, n_yy, n_xy} per slot into tan (hfem_j2_slots doubles, planes
 *                     [n_tiles][5][elem_stride]), the 2x2 diagonal blocks (diag_out may be NULL) and info_out[2] = {plastic
 *                     home elements, 0} (may be NULL).  tan is bound as a POINTER: another call re-linearises into the same
 *                     buffer and a captured hfem_cg_iterate stays valid, as after hfem_cg_setup_hyper.  hfem_cg_start / iterate /
 *                     status / apply / start_amg / iterate_amg then work on K_T unchanged; the apply reads x rows, p rows and
 *                     the records only.  A later hfem_cg_setup_hyper returns the solver to the Neo-Hookean tangent.
 * Every entry point checks its arguments before it touches a device (negative code, message through hfem_last_error).       */
typedef struct hfem_j2 hfem_j2;
int hfem_j2_create(hfem_plan *plan, int64_t ne, const double mat[4], double W, hfem_j2 **out);
int hfem_j2_destroy(hfem_j2 *j2);
int64_t hfem_j2_slots(const hfem_j2 *j2);
int hfem_j2_update(hfem_j2 *j2, const double *x_free, const double *x_fixed, const double *u_free, const double *u_fixed,
                   const double *g_ext, double load, int32_t write_state, double *out, double *g_out, void *stream);
int hfem_j2_commit(hfem_j2 *j2, void *stream);
int hfem_j2_get(hfem_j2 *j2, int32_t which, double *out, void *stream);
int hfem_j2_set(hfem_j2 *j2, const double *state, void *stream);
int hfem_cg_setup_j2(hfem_cg *cg, hfem_j2 *j2, const double *x_free, const double *x_fixed, const double *u_lin_free,
                     const double *u_fixed, double *tan, int32_t precond, double *diag_out, double *info_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HIDENN_FEM_H */
