// Free-vibration modes K_ff phi = lambda M_ff phi by block LOBPCG, TRI3 and QUAD4, gfx950: the mass operator and the
// block-vector kernels of the iteration.  No reference counterpart: the reference has no mass matrix.
//
//   M_e[a][b] = rho |det J| / 24 (1 + delta_ab)                         TRI3 (exact)
//   M_e[a][b] = rho sum_q N_a(q) N_b(q) |det J_q|, 2x2 Gauss             QUAD4 (exact: the integrand is cubic per variable)
//   lumped: the row sum on the diagonal -- rho |det J| / 6 (TRI3), rho sum_q N_a(q) |det J_q| (QUAD4)
//   M acts per displacement component (M x I_2), unit thickness, always |det J| (no gradient convention enters).
//
// A block vector is [m][n] double2: m vectors of n rows (x, y), each contiguous in the storage order of u_free, so a slice is
// what hfem_cg_apply / hfem_amg_vcycle take.  Everything here is fp64 and bitwise reproducible: no floating-point atomics, every
// sum in a fixed order (per-workgroup partials + a one-block finish, as zz_error_kernel / zz_finish_kernel of recover.hip).
// Column counts are compile-time (register tiles); the host walks other widths in tiles, a ragged tile reads its last valid
// row again (a clamped POINTER, never an indexed register array) and does not store the surplus.
//
// * mass_apply_kernel<NPE, M>: one thread per free u row; the row's node walks its node -> (element, corner) fan in the fixed
//   order of post.node_adjacency (the frame of stress_recover_kernel), forms the element's mass row from the coordinates by node id
//   and gathers the M vectors at the element's corners through the node -> row map (-1 = Dirichlet: contributes 0).
// * mass_lumped_kernel<NPE>: the same walk for the lumped diagonal, then a run-time loop over the columns.
// * gram_kernel: G = A B^T in 8 x 8 register tiles (blockIdx.y = tile pair), grid-stride over the rows with a fixed grid, so the
//   order of every sum depends on (n, tile) only; gram_finish_kernel adds the workgroups' partials in ascending order.
//   Plain fp64 FMAs, not MFMA: per row of a 24 x 24 Gram the kernel does 1152 flops on 384 bytes (3 flop/byte at the ideal
//   traffic) -- below the vector-ALU ridge of the part, so the matrix cores would wait on the same loads.
// * combine_kernel<TO>: Out[j] = sum_i C[i][j] S[i], TO output columns per thread in registers, run-time loop over i with the
//   coefficients as wave-uniform loads.
// * residual_kernel / residual_finish_kernel: R[k] = KX[k] - lambda_k MX[k] and the two norms per column.
// * jacobi_kernel: W[k] = D^-1 R[k] with the 2x2 blocks {K_xx, K_xy, K_yy} of hfem_cg_setup.
#include <hip/hip_runtime.h>

#include "hfem_device.h"

namespace hfem {

constexpr int kModBlock = 256;
constexpr int kGramTile = 8;                  // register tile of the Gram kernel: 8 x 8 accumulators
constexpr int kGramBlocks = 128;              // workgroups per tile pair (HFEM_BLOCK_GRAM_PARTIALS = 9 * 64 * 128)
constexpr int kResBlocks = 1024;              // workgroups per column of the residual (HFEM_BLOCK_RESIDUAL_PARTIALS = 2 * 8 * 1024)
constexpr int kMaxBlockCols = 8, kMaxBasisCols = 24;

__device__ __forceinline__ constexpr double mod_corner_xi(int k) { return (k == 1 || k == 2) ? 1.0 : -1.0; }
__device__ __forceinline__ constexpr double mod_corner_eta(int k) { return k >= 2 ? 1.0 : -1.0; }

// The mass row of the run-time corner c of one element: mrow[b] = M_e[c][b] / rho, and their sum (the lumped share).  c enters
// through selects on the unrolled b and through the corner signs, never as an index of a local array (that would be scratch).
template <int NPE>
__device__ __forceinline__ double mass_row(const double2 (&Xn)[NPE], int c, double (&mrow)[NPE]) {
    if constexpr (NPE == 3) {
        const double det = (Xn[1].x - Xn[0].x) * (Xn[2].y - Xn[0].y) - (Xn[2].x - Xn[0].x) * (Xn[1].y - Xn[0].y);
        const double w = fabs(det) * (1.0 / 24.0);
#pragma unroll
        for (int b = 0; b < 3; ++b) mrow[b] = (b == c) ? 2.0 * w : w;
        return 4.0 * w;
    } else {
        const double cx = mod_corner_xi(c), ce = mod_corner_eta(c), gp = 0.57735026918962576451;
        double sum = 0.0;
#pragma unroll
        for (int b = 0; b < 4; ++b) mrow[b] = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double xi = (q & 1) ? gp : -gp, eta = (q & 2) ? gp : -gp;
            double a = 0.0, bb = 0.0, cc = 0.0, d = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double D0 = 0.25 * mod_corner_xi(k) * (1.0 + mod_corner_eta(k) * eta);
                const double D1 = 0.25 * mod_corner_eta(k) * (1.0 + mod_corner_xi(k) * xi);
                a += Xn[k].x * D0; bb += Xn[k].x * D1; cc += Xn[k].y * D0; d += Xn[k].y * D1;
            }
            const double wn = fabs(a * d - bb * cc) * (0.25 * (1.0 + cx * xi) * (1.0 + ce * eta));
            sum += wn;
#pragma unroll
            for (int b = 0; b < 4; ++b) mrow[b] += wn * (0.25 * (1.0 + mod_corner_xi(b) * xi) * (1.0 + mod_corner_eta(b) * eta));
        }
        return sum;
    }
}

template <int NPE, int M>
__global__ __launch_bounds__(kModBlock) void mass_apply_kernel(
    int32_t n_u, const double2 *__restrict__ X, const int32_t *__restrict__ conn, const int32_t *__restrict__ adj_ptr,
    const int32_t *__restrict__ adj, const int32_t *__restrict__ row_node, const int32_t *__restrict__ node_row, double rho,
    const double2 *__restrict__ V, double2 *__restrict__ MV) {
    const int64_t r = (int64_t)blockIdx.x * kModBlock + threadIdx.x;
    if (r >= n_u) return;
    const int32_t n = row_node[r];
    double2 acc[M];
#pragma unroll
    for (int k = 0; k < M; ++k) acc[k] = make_double2(0.0, 0.0);
    const int32_t i0 = adj_ptr[n], i1 = adj_ptr[n + 1];
    for (int32_t i = i0; i < i1; ++i) {
        const int32_t ec = adj[i], e = ec >> 2, c = ec & 3;
        int32_t nd[NPE];
        double2 Xn[NPE];
#pragma unroll
        for (int b = 0; b < NPE; ++b) nd[b] = conn[NPE * (int64_t)e + b];
#pragma unroll
        for (int b = 0; b < NPE; ++b) Xn[b] = X[nd[b]];
        double mrow[NPE];
        mass_row<NPE>(Xn, c, mrow);
#pragma unroll
        for (int b = 0; b < NPE; ++b) {
            const int32_t rb = node_row[nd[b]];
            if (rb < 0) continue;                                          // a Dirichlet node: its value is 0
            const double w = rho * mrow[b];
#pragma unroll
            for (int k = 0; k < M; ++k) {
                const double2 v = V[(int64_t)k * n_u + rb];
                acc[k].x += w * v.x; acc[k].y += w * v.y;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < M; ++k) MV[(int64_t)k * n_u + r] = acc[k];
}

template <int NPE>
__global__ __launch_bounds__(kModBlock) void mass_lumped_kernel(
    int32_t n_u, const double2 *__restrict__ X, const int32_t *__restrict__ conn, const int32_t *__restrict__ adj_ptr,
    const int32_t *__restrict__ adj, const int32_t *__restrict__ row_node, double rho, const double2 *__restrict__ V, int32_t m,
    double2 *__restrict__ MV) {
    const int64_t r = (int64_t)blockIdx.x * kModBlock + threadIdx.x;
    if (r >= n_u) return;
    const int32_t n = row_node[r];
    double ml = 0.0;
    const int32_t i0 = adj_ptr[n], i1 = adj_ptr[n + 1];
    for (int32_t i = i0; i < i1; ++i) {
        const int32_t ec = adj[i], e = ec >> 2, c = ec & 3;
        double2 Xn[NPE];
#pragma unroll
        for (int b = 0; b < NPE; ++b) Xn[b] = X[conn[NPE * (int64_t)e + b]];
        double mrow[NPE];
        ml += rho * mass_row<NPE>(Xn, c, mrow);
    }
    for (int k = 0; k < m; ++k) {
        const double2 v = V[(int64_t)k * n_u + r];
        MV[(int64_t)k * n_u + r] = make_double2(ml * v.x, ml * v.y);
    }
}

// ---------------------------------------------------------------- G = A B^T
// blockIdx.y = ta * tiles_b + tb: rows [8 ta, 8 ta + 8) of A against rows [8 tb, 8 tb + 8) of B; a row past the end is the last
// row again.  Thread t of workgroup b adds the rows b * 256 + t + k * 256 * gridDim.x, k = 0, 1, ... in that order; then the wave
// tree, then the waves in order.  partials[(tile * gridDim.x + b) * 64 + 8 i + j].
__global__ __launch_bounds__(kModBlock) void gram_kernel(const double2 *__restrict__ A, int32_t ma, const double2 *__restrict__ B,
                                                         int32_t mb, int64_t n, int32_t tiles_b, double *__restrict__ partials) {
    constexpr int T = kGramTile;
    __shared__ double red[kModBlock / 64][T * T];
    const int ta = blockIdx.y / tiles_b, tb = blockIdx.y % tiles_b;
    const double2 *pa[T], *pb[T];
#pragma unroll
    for (int i = 0; i < T; ++i) {
        pa[i] = A + (int64_t)min(T * ta + i, ma - 1) * n;
        pb[i] = B + (int64_t)min(T * tb + i, mb - 1) * n;
    }
    double acc[T][T];
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) acc[i][j] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kModBlock;
    for (int64_t r = (int64_t)blockIdx.x * kModBlock + threadIdx.x; r < n; r += stride) {
        double2 a[T], b[T];
#pragma unroll
        for (int i = 0; i < T; ++i) { a[i] = pa[i][r]; b[i] = pb[i][r]; }
#pragma unroll
        for (int i = 0; i < T; ++i)
#pragma unroll
            for (int j = 0; j < T; ++j) acc[i][j] += a[i].x * b[j].x + a[i].y * b[j].y;
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) {
            const double w = wave_sum(acc[i][j]);
            if (lane == 0) red[wid][T * i + j] = w;
        }
    __syncthreads();
    if (threadIdx.x < T * T) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < kModBlock / 64; ++w) s += red[w][threadIdx.x];
        partials[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (T * T) + threadIdx.x] = s;
    }
}

// one workgroup per tile pair: thread (part p = t / 64, entry e = t % 64) adds partials p, p + 4, ... of its entry, the four
// parts are added in order; G is [ma][mb] row-major
__global__ __launch_bounds__(kModBlock) void gram_finish_kernel(const double *__restrict__ partials, int32_t nb, int32_t ma, int32_t mb,
                                                                int32_t tiles_b, double *__restrict__ G) {
    constexpr int T = kGramTile;
    __shared__ double red[kModBlock / 64][T * T];
    const int e = threadIdx.x & 63, p = threadIdx.x >> 6;
    double s = 0.0;
    for (int b = p; b < nb; b += kModBlock / 64) s += partials[((int64_t)blockIdx.x * nb + b) * (T * T) + e];
    red[p][e] = s;
    __syncthreads();
    if (p == 0) {
        double g = 0.0;
#pragma unroll
        for (int w = 0; w < kModBlock / 64; ++w) g += red[w][e];
        const int i = T * (blockIdx.x / tiles_b) + e / T, j = T * (blockIdx.x % tiles_b) + e % T;
        if (i < ma && j < mb) G[i * mb + j] = g;
    }
}

// ---------------------------------------------------------------- Out[j] = sum_i C[i][j] S[i]
// blockIdx.y = output tile of TO columns; C is [ms][mo] row-major on the device (wave-uniform loads)
template <int TO>
__global__ __launch_bounds__(kModBlock) void combine_kernel(const double2 *__restrict__ S, int32_t ms, const double *__restrict__ Cm,
                                                            int32_t mo, int64_t n, double2 *__restrict__ Out) {
    const int j0 = TO * blockIdx.y;
    const int64_t r = (int64_t)blockIdx.x * kModBlock + threadIdx.x;
    if (r >= n) return;
    double2 acc[TO];
#pragma unroll
    for (int j = 0; j < TO; ++j) acc[j] = make_double2(0.0, 0.0);
    for (int i = 0; i < ms; ++i) {
        const double2 s = S[(int64_t)i * n + r];
        const double *crow = Cm + i * mo;
#pragma unroll
        for (int j = 0; j < TO; ++j) {
            const double c = crow[min(j0 + j, mo - 1)];
            acc[j].x += c * s.x; acc[j].y += c * s.y;
        }
    }
#pragma unroll
    for (int j = 0; j < TO; ++j)
        if (j0 + j < mo) Out[(int64_t)(j0 + j) * n + r] = acc[j];
}

// ---------------------------------------------------------------- R[k] = KX[k] - lambda_k MX[k], |R_k|, |MX_k|
// blockIdx.y = column; grid-stride over the rows with a fixed grid; partials[(k * gridDim.x + b)] = {sum r^2, sum (Mx)^2}
__global__ __launch_bounds__(kModBlock) void residual_kernel(const double2 *__restrict__ KX, const double2 *__restrict__ MX,
                                                             const double *__restrict__ lambda, int64_t n, double2 *__restrict__ R,
                                                             double2 *__restrict__ partials) {
    __shared__ double red_r[kModBlock / 64], red_m[kModBlock / 64];
    const int k = blockIdx.y;
    const double lam = lambda[k];
    const int64_t base = (int64_t)k * n, stride = (int64_t)gridDim.x * kModBlock;
    double vr = 0.0, vm = 0.0;
    for (int64_t r = (int64_t)blockIdx.x * kModBlock + threadIdx.x; r < n; r += stride) {
        const double2 kx = KX[base + r], mx = MX[base + r];
        const double2 res = make_double2(kx.x - lam * mx.x, kx.y - lam * mx.y);
        R[base + r] = res;
        vr += res.x * res.x + res.y * res.y;
        vm += mx.x * mx.x + mx.y * mx.y;
    }
    const double tr = block_sum(vr, red_r), tm = block_sum(vm, red_m);
    if (threadIdx.x == 0) partials[(int64_t)k * gridDim.x + blockIdx.x] = make_double2(tr, tm);
}

// one workgroup per column: norms[2 k] = |R_k|_2, norms[2 k + 1] = |MX_k|_2
__global__ __launch_bounds__(kModBlock) void residual_finish_kernel(const double2 *__restrict__ partials, int32_t nb,
                                                                    double *__restrict__ norms) {
    __shared__ double red_r[kModBlock / 64], red_m[kModBlock / 64];
    double vr = 0.0, vm = 0.0;
    for (int b = threadIdx.x; b < nb; b += kModBlock) {
        const double2 p = partials[(int64_t)blockIdx.x * nb + b];
        vr += p.x; vm += p.y;
    }
    const double tr = block_sum(vr, red_r), tm = block_sum(vm, red_m);
    if (threadIdx.x == 0) { norms[2 * blockIdx.x] = sqrt(tr); norms[2 * blockIdx.x + 1] = sqrt(tm); }
}

// ---------------------------------------------------------------- W[k] = D^-1 R[k], D = [[kxx, kxy], [kxy, kyy]] per row
// (W may be R: every thread reads its row before it writes it)
__global__ __launch_bounds__(kModBlock) void jacobi_kernel(const double *__restrict__ diag, const double2 *R, int64_t n, double2 *W) {
    const int64_t r = (int64_t)blockIdx.x * kModBlock + threadIdx.x;
    if (r >= n) return;
    const double kxx = diag[3 * r], kxy = diag[3 * r + 1], kyy = diag[3 * r + 2];
    const double inv = 1.0 / (kxx * kyy - kxy * kxy);
    const int64_t at = (int64_t)blockIdx.y * n + r;
    const double2 v = R[at];
    W[at] = make_double2((kyy * v.x - kxy * v.y) * inv, (kxx * v.y - kxy * v.x) * inv);
}

template <int NPE, int M>
static void launch_mass(int64_t n_u, const double *X, const int32_t *conn, const int32_t *adj_ptr, const int32_t *adj,
                        const int32_t *row_node, const int32_t *node_row, double rho, const double *V, double *MV, hipStream_t s) {
    hipLaunchKernelGGL((mass_apply_kernel<NPE, M>), dim3((unsigned)((n_u + kModBlock - 1) / kModBlock)), dim3(kModBlock), 0, s,
                       (int32_t)n_u, (const double2 *)X, conn, adj_ptr, adj, row_node, node_row, rho, (const double2 *)V,
                       (double2 *)MV);
}

// the columns in chunks of 8, 4, 2, 1 (every column is computed on its own: the chunking does not change a bit)
template <int NPE>
static void mass_chunks(int64_t n_u, const double *X, const int32_t *conn, const int32_t *adj_ptr, const int32_t *adj,
                        const int32_t *row_node, const int32_t *node_row, double rho, const double *V, int32_t m, double *MV,
                        hipStream_t s) {
    int32_t k = 0;
    while (k < m) {
        const double *v = V + 2 * n_u * k;
        double *o = MV + 2 * n_u * k;
        const int32_t left = m - k;
        if (left >= 8) { launch_mass<NPE, 8>(n_u, X, conn, adj_ptr, adj, row_node, node_row, rho, v, o, s); k += 8; }
        else if (left >= 4) { launch_mass<NPE, 4>(n_u, X, conn, adj_ptr, adj, row_node, node_row, rho, v, o, s); k += 4; }
        else if (left >= 2) { launch_mass<NPE, 2>(n_u, X, conn, adj_ptr, adj, row_node, node_row, rho, v, o, s); k += 2; }
        else { launch_mass<NPE, 1>(n_u, X, conn, adj_ptr, adj, row_node, node_row, rho, v, o, s); k += 1; }
    }
}

template <int NPE>
static void mass_lumped(int64_t n_u, const double *X, const int32_t *conn, const int32_t *adj_ptr, const int32_t *adj,
                        const int32_t *row_node, double rho, const double *V, int32_t m, double *MV, hipStream_t s) {
    hipLaunchKernelGGL((mass_lumped_kernel<NPE>), dim3((unsigned)((n_u + kModBlock - 1) / kModBlock)), dim3(kModBlock), 0, s,
                       (int32_t)n_u, (const double2 *)X, conn, adj_ptr, adj, row_node, rho, (const double2 *)V, m, (double2 *)MV);
}

static int64_t row_blocks(int64_t n, int64_t cap) {
    const int64_t nb = (n + kModBlock - 1) / kModBlock;
    return nb < cap ? nb : cap;
}

// len doubles = len / 2 rows of (x, y); the block kernels move whole rows
static int block_len(const char *who, int64_t len) {
    if (len < 0 || (len & 1)) { set_error(std::string(who) + ": len must be even and >= 0 (rows of two doubles)"); return -1; }
    if (len / 2 > (int64_t)INT32_MAX * kModBlock) { set_error(std::string(who) + ": len too large for one launch"); return -1; }
    return 0;
}

}  // namespace hfem

using namespace hfem;

extern "C" int hfem_mass_apply(int device, int32_t npe, const double *X, const int32_t *conn, int64_t ne, int64_t nn,
                               const int32_t *adj_ptr, const int32_t *adj, const int32_t *row_node, const int32_t *node_row,
                               int64_t n_u, double rho, int32_t lumped, const double *V, int32_t m, double *MV, void *stream) {
    const char *who = "hfem_mass_apply";
    if (device < 0) { set_error(std::string(who) + ": negative device"); return -1; }
    if (npe != 3 && npe != 4) { set_error(std::string(who) + ": npe must be 3 (TRI3) or 4 (QUAD4)"); return -1; }
    if (m < 1 || m > kMaxBlockCols) { set_error(std::string(who) + ": m must be in 1..8"); return -1; }
    if (ne < 0 || nn < 0 || n_u < 0) { set_error(std::string(who) + ": negative count"); return -1; }
    if (!(X && conn && adj_ptr && adj && row_node && node_row && V && MV)) { set_error(std::string(who) + ": null pointer"); return -1; }
    if (V == MV) { set_error(std::string(who) + ": MV must not alias V"); return -1; }
    if (!(rho > 0.0)) { set_error(std::string(who) + ": rho must be > 0"); return -1; }
    if (ne >= ((int64_t)1 << 29) || nn > INT32_MAX - kModBlock || n_u > nn) {
        set_error(std::string(who) + ": fewer than 2^29 elements (adjacency entries are e << 2 | c), int32 node ids, n_u <= nn");
        return -1;
    }
    if (n_u == 0 || ne == 0) return 0;
    if (int rc = use_device(device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (lumped) {
        if (npe == 4) mass_lumped<4>(n_u, X, conn, adj_ptr, adj, row_node, rho, V, m, MV, s);
        else mass_lumped<3>(n_u, X, conn, adj_ptr, adj, row_node, rho, V, m, MV, s);
    } else {
        if (npe == 4) mass_chunks<4>(n_u, X, conn, adj_ptr, adj, row_node, node_row, rho, V, m, MV, s);
        else mass_chunks<3>(n_u, X, conn, adj_ptr, adj, row_node, node_row, rho, V, m, MV, s);
    }
    return launch_status(who);
}

extern "C" int hfem_block_gram(int device, const double *A, int32_t ma, const double *B, int32_t mb, int64_t len, double *partials,
                               double *G, void *stream) {
    const char *who = "hfem_block_gram";
    if (device < 0) { set_error(std::string(who) + ": negative device"); return -1; }
    if (ma < 1 || ma > kMaxBasisCols || mb < 1 || mb > kMaxBasisCols) { set_error(std::string(who) + ": ma and mb must be in 1..24"); return -1; }
    if (!(A && B && partials && G)) { set_error(std::string(who) + ": null pointer"); return -1; }
    if (int rc = block_len(who, len)) return rc;
    if (len == 0) { set_error(std::string(who) + ": len must be > 0"); return -1; }
    if (int rc = use_device(device)) return rc;
    const int64_t n = len / 2;
    const int32_t tiles_a = (ma + kGramTile - 1) / kGramTile, tiles_b = (mb + kGramTile - 1) / kGramTile;
    const int32_t nb = (int32_t)row_blocks(n, kGramBlocks);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(gram_kernel, dim3((unsigned)nb, (unsigned)(tiles_a * tiles_b)), dim3(kModBlock), 0, s, (const double2 *)A, ma,
                       (const double2 *)B, mb, n, tiles_b, partials);
    if (int rc = launch_status(who)) return rc;
    hipLaunchKernelGGL(gram_finish_kernel, dim3((unsigned)(tiles_a * tiles_b)), dim3(kModBlock), 0, s, (const double *)partials, nb, ma,
                       mb, tiles_b, G);
    return launch_status(who);
}

extern "C" int hfem_block_combine(int device, const double *S, int32_t ms, const double *Cm, int32_t mo, int64_t len, double *Out,
                                  void *stream) {
    const char *who = "hfem_block_combine";
    if (device < 0) { set_error(std::string(who) + ": negative device"); return -1; }
    if (ms < 1 || ms > kMaxBasisCols || mo < 1 || mo > kMaxBasisCols) { set_error(std::string(who) + ": ms and mo must be in 1..24"); return -1; }
    if (!(S && Cm && Out)) { set_error(std::string(who) + ": null pointer"); return -1; }
    if (int rc = block_len(who, len)) return rc;
    const double *s_end = S + (int64_t)ms * len, *o_end = Out + (int64_t)mo * len;
    if (Out < s_end && S < o_end) { set_error(std::string(who) + ": Out must not overlap S (not in place)"); return -1; }
    if (len == 0) return 0;
    if (int rc = use_device(device)) return rc;
    const int64_t n = len / 2;
    const unsigned nb = (unsigned)((n + kModBlock - 1) / kModBlock);
    if (mo > 8)
        hipLaunchKernelGGL(combine_kernel<16>, dim3(nb, (unsigned)((mo + 15) / 16)), dim3(kModBlock), 0, (hipStream_t)stream,
                           (const double2 *)S, ms, Cm, mo, n, (double2 *)Out);
    else
        hipLaunchKernelGGL(combine_kernel<8>, dim3(nb, 1u), dim3(kModBlock), 0, (hipStream_t)stream, (const double2 *)S, ms, Cm, mo, n,
                           (double2 *)Out);
    return launch_status(who);
}

extern "C" int hfem_block_residual(int device, const double *KX, const double *MX, const double *lambda, int32_t m, int64_t len,
                                   double *R, double *partials, double *norms, void *stream) {
    const char *who = "hfem_block_residual";
    if (device < 0) { set_error(std::string(who) + ": negative device"); return -1; }
    if (m < 1 || m > kMaxBlockCols) { set_error(std::string(who) + ": m must be in 1..8"); return -1; }
    if (!(KX && MX && lambda && R && partials && norms)) { set_error(std::string(who) + ": null pointer"); return -1; }
    if (int rc = block_len(who, len)) return rc;
    if (len == 0) { set_error(std::string(who) + ": len must be > 0"); return -1; }
    if (int rc = use_device(device)) return rc;
    const int64_t n = len / 2;
    const int32_t nb = (int32_t)row_blocks(n, kResBlocks);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(residual_kernel, dim3((unsigned)nb, (unsigned)m), dim3(kModBlock), 0, s, (const double2 *)KX, (const double2 *)MX,
                       lambda, n, (double2 *)R, (double2 *)partials);
    if (int rc = launch_status(who)) return rc;
    hipLaunchKernelGGL(residual_finish_kernel, dim3((unsigned)m), dim3(kModBlock), 0, s, (const double2 *)partials, nb, norms);
    return launch_status(who);
}

extern "C" int hfem_block_jacobi_apply(int device, const double *diag, const double *R, int32_t m, int64_t len, double *W, void *stream) {
    const char *who = "hfem_block_jacobi_apply";
    if (device < 0) { set_error(std::string(who) + ": negative device"); return -1; }
    if (m < 1 || m > kMaxBlockCols) { set_error(std::string(who) + ": m must be in 1..8"); return -1; }
    if (!(diag && R && W)) { set_error(std::string(who) + ": null pointer"); return -1; }
    if (int rc = block_len(who, len)) return rc;
    if (len == 0) return 0;
    if (int rc = use_device(device)) return rc;
    const int64_t n = len / 2;
    hipLaunchKernelGGL(jacobi_kernel, dim3((unsigned)((n + kModBlock - 1) / kModBlock), (unsigned)m), dim3(kModBlock), 0,
                       (hipStream_t)stream, diag, (const double2 *)R, n, (double2 *)W);
    return launch_status(who);
}
