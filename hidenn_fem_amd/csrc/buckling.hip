// Linearised buckling (K + lambda K_G(sigma_0)) phi = 0, TRI3 and QUAD4, gfx950: the geometric stiffness operator.
// The iteration itself is the block LOBPCG of csrc/modal.hip on the pencil (K_G, K).  No reference counterpart.
//
//   v^T K_G v = sum_e sum_q w_q |det J_q| sum_{i in {x, y}} (grad v_i)^T S_0(q) (grad v_i)
//   S_0 = [[s_xx, s_xy], [s_xy, s_yy]],  sigma = C eps(u_0) at the point, u_0 with the model's u_fixed on the Dirichlet rows
//   grad: the shape-function gradient of the loss's convention (PHYS: D J^-1, else the reference's D J^-T -- b and c of the
//   Jacobian swap, as in hfem_device.h / hfem_quad4_dev.h); TRI3: constant gradients, weight W |det J| (W = the sum of the
//   loss's quadrature weights, as hfem_cg_setup takes it); QUAD4: the 2x2 Gauss rule with weights 1, the rule of K (it does
//   NOT integrate K_G of a distorted cell exactly: the rule is part of the definition).
//   K_G acts per displacement component (G x I_2): per element one scalar matrix
//   G_e[a][b] = sum_q w_q |det J_q| (g_a . S_0 g_b).
//
// Everything here is fp64 and bitwise reproducible: no floating-point atomics, every sum in a fixed order.
//
// * geom_setup_kernel<NPE, PHYS>: one thread per element; coordinates by node id, u_0 through the node -> row map (a Dirichlet
//   node reads its row of the u_fixed table), writes the FULL matrix G_e as [ne][NPE][NPE] (72 B per TRI3 element, 128 B per
//   QUAD4 cell): the apply then reads the row of its run-time corner c by a pointer offset and never indexes a register array
//   with c (that would be scratch).  Run once per prestress state.
// * geom_apply_kernel<NPE, M>: the frame of mass_apply_kernel (csrc/modal.hip): one thread per free u row, the row's node walks
//   its (element, corner) fan in the fixed order of post.node_adjacency, reads row c of G_e and gathers the M columns at the
//   element's corners through the node -> row map (-1 = Dirichlet: contributes 0).  Where the mass kernel gathers NPE
//   coordinate rows and integrates, this one reads NPE stored doubles.  Column counts are compile-time register tiles (1, 2, 4,
//   8); a ragged tile reads its last valid column again through a clamped pointer and does not store the surplus.
#include <hip/hip_runtime.h>

#include "hfem_device.h"

namespace hfem {

constexpr int kGeomBlock = 256;
constexpr int kGeomMaxCols = 8;

struct GeomMat {                 // C (Voigt, engineering shear): by value
    double c11, c12, c22, c33;
};

__device__ __forceinline__ constexpr double geom_corner_xi(int k) { return (k == 1 || k == 2) ? 1.0 : -1.0; }
__device__ __forceinline__ constexpr double geom_corner_eta(int k) { return k >= 2 ? 1.0 : -1.0; }

// One point of an element: J = [[a, b0], [c0, d]] (J[i][j] = d x_i / d xi_j), D0 / D1 the reference gradients of the NPE shape
// functions there, wq the rule's weight; adds wq |det| (g_a . S_0 g_b) to Ge.
template <int NPE, bool PHYS>
__device__ __forceinline__ void geom_point(double a, double b0, double c0, double d, const double (&D0)[NPE], const double (&D1)[NPE],
                                           const double2 (&Un)[NPE], const GeomMat &m, double wq, double (&Ge)[NPE][NPE]) {
    const double b = PHYS ? c0 : b0, c = PHYS ? b0 : c0;                   // as LinearLaw<PHYS>::point (hfem_recover_hyper_dev.h)
    const double det = a * d - b * c;
    const double inv = fast_rcp(det);
    double gx[NPE], gy[NPE];
    double h00 = 0.0, h01 = 0.0, h10 = 0.0, h11 = 0.0;
#pragma unroll
    for (int k = 0; k < NPE; ++k) {
        gx[k] = (D0[k] * d - D1[k] * b) * inv;
        gy[k] = (D1[k] * a - D0[k] * c) * inv;
        h00 += Un[k].x * gx[k]; h01 += Un[k].x * gy[k];
        h10 += Un[k].y * gx[k]; h11 += Un[k].y * gy[k];
    }
    const double sxx = m.c11 * h00 + m.c12 * h11, syy = m.c12 * h00 + m.c22 * h11, sxy = m.c33 * (h01 + h10);
    const double w = wq * fabs(det);
#pragma unroll
    for (int k = 0; k < NPE; ++k) {
        const double tx = w * (sxx * gx[k] + sxy * gy[k]), ty = w * (sxy * gx[k] + syy * gy[k]);      // w S_0 g_k
#pragma unroll
        for (int l = 0; l < NPE; ++l) Ge[l][k] += gx[l] * tx + gy[l] * ty;
    }
}

template <int NPE, bool PHYS>
__global__ __launch_bounds__(kGeomBlock) void geom_setup_kernel(
    int64_t ne, const double2 *__restrict__ X, const int32_t *__restrict__ conn, const double2 *__restrict__ u_free, int32_t n_u,
    const double2 *__restrict__ u_fixed, int32_t n_fix, const int32_t *__restrict__ node_row, const int32_t *__restrict__ fixed_row,
    GeomMat m, double W, double *__restrict__ G) {
    const int64_t e = (int64_t)blockIdx.x * kGeomBlock + threadIdx.x;
    if (e >= ne) return;
    double2 Xn[NPE], Un[NPE];
#pragma unroll
    for (int k = 0; k < NPE; ++k) {
        const int32_t nd = conn[NPE * e + k];
        Xn[k] = X[nd];
        const int32_t r = node_row[nd];
        double2 u = make_double2(0.0, 0.0);
        if (r >= 0) {
            if (r < n_u) u = u_free[r];
        } else {
            const int32_t f = fixed_row[nd];
            if (f >= 0 && f < n_fix) u = u_fixed[f];
        }
        Un[k] = u;
    }
    double Ge[NPE][NPE];
#pragma unroll
    for (int k = 0; k < NPE; ++k)
#pragma unroll
        for (int l = 0; l < NPE; ++l) Ge[k][l] = 0.0;
    if constexpr (NPE == 3) {                                              // N = (xi, eta, 1 - xi - eta): constant gradients
        const double D0[3] = {1.0, 0.0, -1.0}, D1[3] = {0.0, 1.0, -1.0};
        geom_point<3, PHYS>(Xn[0].x - Xn[2].x, Xn[1].x - Xn[2].x, Xn[0].y - Xn[2].y, Xn[1].y - Xn[2].y, D0, D1, Un, m, W, Ge);
    } else {
        const double gp = 0.57735026918962576451;                          // 1 / sqrt(3)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double xi = (q & 1) ? gp : -gp, eta = (q & 2) ? gp : -gp;
            double D0[4], D1[4];
            double a = 0.0, b = 0.0, c = 0.0, d = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                D0[k] = 0.25 * geom_corner_xi(k) * (1.0 + geom_corner_eta(k) * eta);
                D1[k] = 0.25 * geom_corner_eta(k) * (1.0 + geom_corner_xi(k) * xi);
                a += Xn[k].x * D0[k]; b += Xn[k].x * D1[k]; c += Xn[k].y * D0[k]; d += Xn[k].y * D1[k];
            }
            geom_point<4, PHYS>(a, b, c, d, D0, D1, Un, m, 1.0, Ge);
        }
    }
    double *out = G + (int64_t)(NPE * NPE) * e;
#pragma unroll
    for (int k = 0; k < NPE; ++k)
#pragma unroll
        for (int l = 0; l < NPE; ++l) out[NPE * k + l] = Ge[k][l];
}

// m <= M columns are valid: a ragged tile reads its last valid column again through a clamped POINTER (never an indexed register
// array) and does not store the surplus.  Every column is summed on its own in the order of the fan, so the tile width does not
// change a bit of any column.
template <int NPE, int M>
__global__ __launch_bounds__(kGeomBlock) void geom_apply_kernel(
    int32_t n_u, const double *__restrict__ G, const int32_t *__restrict__ conn, const int32_t *__restrict__ adj_ptr,
    const int32_t *__restrict__ adj, const int32_t *__restrict__ row_node, const int32_t *__restrict__ node_row,
    const double2 *__restrict__ V, int32_t m, double2 *__restrict__ GV) {
    const int64_t r = (int64_t)blockIdx.x * kGeomBlock + threadIdx.x;
    if (r >= n_u) return;
    const int32_t n = row_node[r];
    const double2 *pv[M];
    double2 acc[M];
#pragma unroll
    for (int k = 0; k < M; ++k) {
        pv[k] = V + (int64_t)min(k, m - 1) * n_u;
        acc[k] = make_double2(0.0, 0.0);
    }
    const int32_t i0 = adj_ptr[n], i1 = adj_ptr[n + 1];
    for (int32_t i = i0; i < i1; ++i) {
        const int32_t ec = adj[i], e = ec >> 2, c = ec & 3;
        const double *__restrict__ grow = G + (int64_t)(NPE * NPE) * e + NPE * c;      // row c of G_e: a pointer offset
        int32_t nd[NPE];
        double g[NPE];
#pragma unroll
        for (int b = 0; b < NPE; ++b) { nd[b] = conn[NPE * (int64_t)e + b]; g[b] = grow[b]; }
#pragma unroll
        for (int b = 0; b < NPE; ++b) {
            const int32_t rb = node_row[nd[b]];
            if (rb < 0) continue;                                          // a Dirichlet node: its value is 0
#pragma unroll
            for (int k = 0; k < M; ++k) {
                const double2 v = pv[k][rb];
                acc[k].x += g[b] * v.x; acc[k].y += g[b] * v.y;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < M; ++k)
        if (k < m) GV[(int64_t)k * n_u + r] = acc[k];
}

template <int NPE, bool PHYS>
static void launch_geom_setup(int64_t ne, const double *X, const int32_t *conn, const double *u_free, int64_t n_u,
                              const double *u_fixed, int64_t n_fix, const int32_t *node_row, const int32_t *fixed_row,
                              const GeomMat &m, double W, double *G, hipStream_t s) {
    hipLaunchKernelGGL((geom_setup_kernel<NPE, PHYS>), dim3((unsigned)((ne + kGeomBlock - 1) / kGeomBlock)), dim3(kGeomBlock), 0, s,
                       ne, (const double2 *)X, conn, (const double2 *)u_free, (int32_t)n_u, (const double2 *)u_fixed,
                       (int32_t)n_fix, node_row, fixed_row, m, W, G);
}

template <int NPE, int M>
static void launch_geom_apply(int64_t n_u, const double *G, const int32_t *conn, const int32_t *adj_ptr, const int32_t *adj,
                              const int32_t *row_node, const int32_t *node_row, const double *V, int32_t m, double *GV, hipStream_t s) {
    hipLaunchKernelGGL((geom_apply_kernel<NPE, M>), dim3((unsigned)((n_u + kGeomBlock - 1) / kGeomBlock)), dim3(kGeomBlock), 0, s,
                       (int32_t)n_u, G, conn, adj_ptr, adj, row_node, node_row, (const double2 *)V, m, (double2 *)GV);
}

// ONE launch for the m <= 8 columns of a call, in the narrowest register tile of 1, 2, 4 or 8 that holds them: the fan, the
// connectivity and the rows of G_e are walked once whatever m is (the default block of a four-mode solve is 6)
template <int NPE>
static void geom_tile(int64_t n_u, const double *G, const int32_t *conn, const int32_t *adj_ptr, const int32_t *adj,
                      const int32_t *row_node, const int32_t *node_row, const double *V, int32_t m, double *GV, hipStream_t s) {
    if (m > 4) launch_geom_apply<NPE, 8>(n_u, G, conn, adj_ptr, adj, row_node, node_row, V, m, GV, s);
    else if (m > 2) launch_geom_apply<NPE, 4>(n_u, G, conn, adj_ptr, adj, row_node, node_row, V, m, GV, s);
    else if (m == 2) launch_geom_apply<NPE, 2>(n_u, G, conn, adj_ptr, adj, row_node, node_row, V, m, GV, s);
    else launch_geom_apply<NPE, 1>(n_u, G, conn, adj_ptr, adj, row_node, node_row, V, m, GV, s);
}

static int geom_counts(const char *who, int32_t npe, int64_t ne, int64_t nn, int64_t n_u) {
    if (npe != 3 && npe != 4) { set_error(std::string(who) + ": npe must be 3 (TRI3) or 4 (QUAD4)"); return -1; }
    if (ne < 0 || nn < 0 || n_u < 0) { set_error(std::string(who) + ": negative count"); return -1; }
    if (ne >= ((int64_t)1 << 29) || nn > INT32_MAX - kGeomBlock || n_u > nn) {
        set_error(std::string(who) + ": fewer than 2^29 elements (adjacency entries are e << 2 | c), int32 node ids, n_u <= nn");
        return -1;
    }
    return 0;
}

}  // namespace hfem

using namespace hfem;

extern "C" int hfem_geom_setup(int device, int32_t npe, int32_t flags, const double *X, const int32_t *conn, int64_t ne, int64_t nn,
                               const double *u_free, int64_t n_u, const double *u_fixed, int64_t n_fix, const int32_t *node_row,
                               const int32_t *fixed_row, const double mat[4], double W, double *G, void *stream) {
    const char *who = "hfem_geom_setup";
    if (device < 0) { set_error(std::string(who) + ": negative device"); return -1; }
    if (flags & ~HFEM_FLAG_PHYSICAL_GRAD) { set_error(std::string(who) + ": flags: HFEM_FLAG_PHYSICAL_GRAD or 0"); return -1; }
    if (int rc = geom_counts(who, npe, ne, nn, n_u)) return rc;
    if (n_fix < 0 || n_fix > nn) { set_error(std::string(who) + ": n_fix must be in 0..nn"); return -1; }
    if (!(X && conn && node_row && fixed_row && mat && G) || (n_u > 0 && !u_free) || (n_fix > 0 && !u_fixed)) {
        set_error(std::string(who) + ": null pointer");
        return -1;
    }
    if (!(W > 0.0)) { set_error(std::string(who) + ": W must be > 0"); return -1; }
    if (ne == 0) return 0;
    if (int rc = use_device(device)) return rc;
    const GeomMat m{mat[0], mat[1], mat[2], mat[3]};
    hipStream_t s = (hipStream_t)stream;
    const bool phys = (flags & HFEM_FLAG_PHYSICAL_GRAD) != 0;
    if (npe == 4) {
        if (phys) launch_geom_setup<4, true>(ne, X, conn, u_free, n_u, u_fixed, n_fix, node_row, fixed_row, m, W, G, s);
        else launch_geom_setup<4, false>(ne, X, conn, u_free, n_u, u_fixed, n_fix, node_row, fixed_row, m, W, G, s);
    } else {
        if (phys) launch_geom_setup<3, true>(ne, X, conn, u_free, n_u, u_fixed, n_fix, node_row, fixed_row, m, W, G, s);
        else launch_geom_setup<3, false>(ne, X, conn, u_free, n_u, u_fixed, n_fix, node_row, fixed_row, m, W, G, s);
    }
    return launch_status(who);
}

extern "C" int hfem_geom_apply(int device, int32_t npe, const double *G, const int32_t *conn, int64_t ne, int64_t nn,
                               const int32_t *adj_ptr, const int32_t *adj, const int32_t *row_node, const int32_t *node_row,
                               int64_t n_u, const double *V, int32_t m, double *GV, void *stream) {
    const char *who = "hfem_geom_apply";
    if (device < 0) { set_error(std::string(who) + ": negative device"); return -1; }
    if (m < 1 || m > kGeomMaxCols) { set_error(std::string(who) + ": m must be in 1..8"); return -1; }
    if (int rc = geom_counts(who, npe, ne, nn, n_u)) return rc;
    if (!(G && conn && adj_ptr && adj && row_node && node_row && V && GV)) { set_error(std::string(who) + ": null pointer"); return -1; }
    if (V == GV) { set_error(std::string(who) + ": GV must not alias V"); return -1; }
    if (n_u == 0 || ne == 0) return 0;
    if (int rc = use_device(device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (npe == 4) geom_tile<4>(n_u, G, conn, adj_ptr, adj, row_node, node_row, V, m, GV, s);
    else geom_tile<3>(n_u, G, conn, adj_ptr, adj, row_node, node_row, V, m, GV, s);
    return launch_status(who);
}
