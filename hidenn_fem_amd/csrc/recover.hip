// Nodal stress recovery and the Zienkiewicz-Zhu (ZZ) energy-norm error estimate, TRI3 and QUAD4, gfx950.
// No reference counterpart: the reference stops at the per-element von Mises plot (its src/plots.py:177-198).
//
//   sigma_h = C (eps_xx, eps_yy, gamma_xy) of grad_u in the convention of the loss (PHYS: grad_u = G Jinv, else the
//   reference's G Jinv^T -- b and c of the Jacobian swap, as in hfem_device.h / hfem_quad4_dev.h);
//   points: TRI3 the centroid with w = |det| / 2 (sigma_h is constant), QUAD4 the 2x2 Gauss points with w_q = |det_q|;
//   sigma*_n = sum_{e at n} sum_q w_q N_n(q) sigma_h(q) / sum_{e at n} sum_q w_q N_n(q)      (lumped L2 projection)
//   eta_e^2  = sum_q w_q d_q.S.d_q,  d_q = sum_k N_k(q) sigma*_k - sigma_h(q),  S = C^-1      (TRI3: exact closed form)
//   |u_h|_e^2 = sum_q w_q sigma_h.S.sigma_h                                                    (2 x the strain energy)
//
// * stress_recover_kernel: one thread per NODE walks the node -> (element, corner) CSR adjacency in ascending element id
//   (entries e << 2 | c, as tri3_det.hip), re-evaluates each adjacent element from its nodes and adds this corner's share
//   in that fixed order: no atomics, no zero-fill, bitwise reproducible.  Four dependent gather levels (adjacency ->
//   connectivity -> node rows -> arithmetic): L2-latency bound like the deterministic energy path, and run once per solve.
// * zz_error_kernel: one thread per element; per-block partial sums of eta_e^2 and |u_h|_e^2 (shuffle tree + wave order),
//   which zz_finish_kernel (one block) adds in a fixed order into totals[2].  No floating-point atomics.
#include <hip/hip_runtime.h>

#include "hfem_device.h"
#include "hfem_quad4_dev.h"

namespace hfem {

constexpr int kRecBlock = 256;

struct RecMat {                  // plane-stress C and its inverse S (Voigt, engineering shear): by value
    double c11, c12, c22, c33;
    double s11, s12, s22, s33;
};

struct Sig3 {
    double xx, yy, xy;
};

__device__ __forceinline__ double s_form(const RecMat &m, const Sig3 &d) {   // d.S.d
    return m.s11 * d.xx * d.xx + 2.0 * m.s12 * d.xx * d.yy + m.s22 * d.yy * d.yy + m.s33 * d.xy * d.xy;
}

// sigma_h at one point from J = [[a, b], [c, d]] (J[i][j] = d x_i / d xi_j) and G = [g0 g1] (columns du / d xi_j)
template <bool PHYS>
__device__ __forceinline__ Sig3 point_stress(double a, double b0, double c0, double d, double2 g0, double2 g1, const RecMat &m,
                                             double &det) {
    const double b = PHYS ? c0 : b0, c = PHYS ? b0 : c0;                   // E_phys(a, b, c, d) = E_ref(a, c, b, d)
    det = a * d - b * c;
    const double inv = 1.0 / det;
    const double h00 = (g0.x * d - g1.x * b) * inv, h01 = (g1.x * a - g0.x * c) * inv;
    const double h10 = (g0.y * d - g1.y * b) * inv, h11 = (g1.y * a - g0.y * c) * inv;
    const double gam = h01 + h10;
    return Sig3{m.c11 * h00 + m.c12 * h11, m.c12 * h00 + m.c22 * h11, m.c33 * gam};
}

template <int NPE> struct RecPoints { static constexpr int NQ = NPE == 3 ? 1 : 4; };

// sigma_h and the weights at the element's points; Xn, Un = the element's node rows in local order
template <int NPE, bool PHYS>
__device__ __forceinline__ void element_points(const double2 (&Xn)[NPE], const double2 (&Un)[NPE], const RecMat &m,
                                               Sig3 (&sg)[RecPoints<NPE>::NQ], double (&w)[RecPoints<NPE>::NQ]) {
    if constexpr (NPE == 3) {
        double det;
        sg[0] = point_stress<PHYS>(Xn[0].x - Xn[2].x, Xn[1].x - Xn[2].x, Xn[0].y - Xn[2].y, Xn[1].y - Xn[2].y,
                                   make_double2(Un[0].x - Un[2].x, Un[0].y - Un[2].y),
                                   make_double2(Un[1].x - Un[2].x, Un[1].y - Un[2].y), m, det);
        w[0] = 0.5 * fabs(det);
    } else {
        const double gp = 0.57735026918962576451;   // 1/sqrt(3); points in the order (-,-) (+,-) (-,+) (+,+)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double xi = (q & 1) ? gp : -gp, eta = (q & 2) ? gp : -gp;
            double D0[4], D1[4];
            shape_derivs(xi, eta, D0, D1);
            double a = 0.0, b = 0.0, c = 0.0, d = 0.0;
            double2 g0 = make_double2(0.0, 0.0), g1 = make_double2(0.0, 0.0);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                a += Xn[k].x * D0[k]; b += Xn[k].x * D1[k]; c += Xn[k].y * D0[k]; d += Xn[k].y * D1[k];
                g0.x += Un[k].x * D0[k]; g0.y += Un[k].y * D0[k]; g1.x += Un[k].x * D1[k]; g1.y += Un[k].y * D1[k];
            }
            double det;
            sg[q] = point_stress<PHYS>(a, b, c, d, g0, g1, m, det);
            w[q] = fabs(det);
        }
    }
}

template <int NPE>
__device__ __forceinline__ void gather_element(const double2 *__restrict__ X, const double2 *__restrict__ U,
                                               const int32_t *__restrict__ conn, int64_t e, double2 (&Xn)[NPE],
                                               double2 (&Un)[NPE], int32_t (&nd)[NPE]) {
#pragma unroll
    for (int k = 0; k < NPE; ++k) nd[k] = conn[NPE * e + k];
#pragma unroll
    for (int k = 0; k < NPE; ++k) { Xn[k] = X[nd[k]]; Un[k] = U[nd[k]]; }
}

template <int NPE, bool PHYS>
__global__ __launch_bounds__(kRecBlock) void stress_recover_kernel(
    int32_t nn, const double2 *__restrict__ X, const double2 *__restrict__ U, const int32_t *__restrict__ conn,
    const int32_t *__restrict__ adj_ptr, const int32_t *__restrict__ adj, RecMat m, double *__restrict__ nodal_stress,
    double *__restrict__ nodal_area) {
    constexpr int NQ = RecPoints<NPE>::NQ;
    const int64_t n = (int64_t)blockIdx.x * kRecBlock + threadIdx.x;
    if (n >= nn) return;
    double sxx = 0.0, syy = 0.0, sxy = 0.0, den = 0.0;
    const int32_t i0 = adj_ptr[n], i1 = adj_ptr[n + 1];
    for (int32_t i = i0; i < i1; ++i) {
        const int32_t ec = adj[i], e = ec >> 2, c = ec & 3;
        double2 Xn[NPE], Un[NPE];
        int32_t nd[NPE];
        gather_element<NPE>(X, U, conn, e, Xn, Un, nd);
        Sig3 sg[NQ];
        double w[NQ];
        element_points<NPE, PHYS>(Xn, Un, m, sg, w);
        // N_c(q) of the run-time corner c from the corner signs (selects), never by indexing a local array: that would
        // put the array in scratch
        [[maybe_unused]] const double cx = corner_xi(c), ce = corner_eta(c), gp = 0.57735026918962576451;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            double N = 1.0 / 3.0;                                          // TRI3: N_c at the centroid
            if constexpr (NPE == 4) N = 0.25 * (1.0 + cx * ((q & 1) ? gp : -gp)) * (1.0 + ce * ((q & 2) ? gp : -gp));
            const double wn = w[q] * N;
            sxx += wn * sg[q].xx; syy += wn * sg[q].yy; sxy += wn * sg[q].xy;
            den += wn;
        }
    }
    // a node that no element references has no stress to recover: zeros, lumped area 0
    const bool has = i1 > i0;
    nodal_stress[3 * n] = has ? sxx / den : 0.0;
    nodal_stress[3 * n + 1] = has ? syy / den : 0.0;
    nodal_stress[3 * n + 2] = has ? sxy / den : 0.0;
    if (nodal_area) nodal_area[n] = den;
}

template <int NPE, bool PHYS>
__global__ __launch_bounds__(kRecBlock) void zz_error_kernel(int64_t ne, const double2 *__restrict__ X,
                                                             const double2 *__restrict__ U, const int32_t *__restrict__ conn,
                                                             const double *__restrict__ nodal_stress, RecMat m,
                                                             double *__restrict__ eta2, double *__restrict__ norm2,
                                                             double2 *__restrict__ partials) {
    constexpr int NQ = RecPoints<NPE>::NQ;
    __shared__ double red_e[kRecBlock / 64], red_n[kRecBlock / 64];
    const int64_t e = (int64_t)blockIdx.x * kRecBlock + threadIdx.x;
    double ve = 0.0, vn = 0.0;
    if (e < ne) {
        double2 Xn[NPE], Un[NPE];
        int32_t nd[NPE];
        gather_element<NPE>(X, U, conn, e, Xn, Un, nd);
        Sig3 ss[NPE];
#pragma unroll
        for (int k = 0; k < NPE; ++k)
            ss[k] = Sig3{nodal_stress[3 * (int64_t)nd[k]], nodal_stress[3 * (int64_t)nd[k] + 1], nodal_stress[3 * (int64_t)nd[k] + 2]};
        Sig3 sg[NQ];
        double w[NQ];
        element_points<NPE, PHYS>(Xn, Un, m, sg, w);
        if constexpr (NPE == 3) {
            // exact integral of the linear d(x) = sum_k N_k d_k over the triangle:
            //   A/12 [sum_k d_k.S.d_k + (sum_k d_k).S.(sum_k d_k)],  A = w[0]
            Sig3 t = Sig3{0.0, 0.0, 0.0};
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const Sig3 d = Sig3{ss[k].xx - sg[0].xx, ss[k].yy - sg[0].yy, ss[k].xy - sg[0].xy};
                acc += s_form(m, d);
                t.xx += d.xx; t.yy += d.yy; t.xy += d.xy;
            }
            ve = (w[0] * (1.0 / 12.0)) * (acc + s_form(m, t));
            vn = w[0] * s_form(m, sg[0]);
        } else {
            const double gp = 0.57735026918962576451;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double xi = (q & 1) ? gp : -gp, eta = (q & 2) ? gp : -gp;
                Sig3 d = Sig3{-sg[q].xx, -sg[q].yy, -sg[q].xy};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double N = 0.25 * (1.0 + corner_xi(k) * xi) * (1.0 + corner_eta(k) * eta);
                    d.xx += N * ss[k].xx; d.yy += N * ss[k].yy; d.xy += N * ss[k].xy;
                }
                ve += w[q] * s_form(m, d);
                vn += w[q] * s_form(m, sg[q]);
            }
        }
        eta2[e] = ve;
        if (norm2) norm2[e] = vn;
    }
    const double te = block_sum(ve, red_e), tn = block_sum(vn, red_n);
    if (threadIdx.x == 0) partials[blockIdx.x] = make_double2(te, tn);
}

// totals = {sum eta_e^2, sum |u_h|_e^2}: thread t adds partials t, t + 256, ... in ascending index, then the block tree --
// one fixed order for a given block count
__global__ __launch_bounds__(kRecBlock) void zz_finish_kernel(const double2 *__restrict__ partials, int64_t n,
                                                              double *__restrict__ totals) {
    __shared__ double red_e[kRecBlock / 64], red_n[kRecBlock / 64];
    double ve = 0.0, vn = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kRecBlock) {
        const double2 p = partials[i];
        ve += p.x; vn += p.y;
    }
    const double te = block_sum(ve, red_e), tn = block_sum(vn, red_n);
    if (threadIdx.x == 0) { totals[0] = te; totals[1] = tn; }
}

static int rec_mat(const double *mat, RecMat &m, const char *who) {
    m.c11 = mat[0]; m.c12 = mat[1]; m.c22 = mat[2]; m.c33 = mat[3];
    const double D = m.c11 * m.c22 - m.c12 * m.c12;
    if (!(D > 0.0) || !(m.c33 > 0.0) || !(m.c11 > 0.0)) {
        set_error(std::string(who) + ": mat is not positive definite");
        return -1;
    }
    m.s11 = m.c22 / D; m.s12 = -m.c12 / D; m.s22 = m.c11 / D; m.s33 = 1.0 / m.c33;
    return 0;
}

template <int NPE>
static int stress_recover(const char *who, int device, const double *X, const double *U, const int32_t *conn, int64_t ne,
                          int64_t nn, const int32_t *adj_ptr, const int32_t *adj, const double *mat, int32_t flags,
                          double *nodal_stress, double *nodal_area, void *stream) {
    if (ne < 0 || nn < 0) { set_error(std::string(who) + ": negative count"); return -1; }
    if (ne == 0 || nn == 0) return 0;
    if (!(X && U && conn && adj_ptr && adj && mat && nodal_stress)) { set_error(std::string(who) + ": null pointer"); return -1; }
    if (flags & ~HFEM_FLAG_PHYSICAL_GRAD) { set_error(std::string(who) + ": flags: HFEM_FLAG_PHYSICAL_GRAD or 0"); return -1; }
    if (ne >= ((int64_t)1 << 29) || nn > INT32_MAX - kRecBlock) {
        set_error(std::string(who) + ": fewer than 2^29 elements (adjacency entries are e << 2 | c) and int32 node ids");
        return -1;
    }
    RecMat m;
    if (int rc = rec_mat(mat, m, who)) return rc;
    if (int rc = use_device(device)) return rc;
    const dim3 grid((unsigned)((nn + kRecBlock - 1) / kRecBlock));
#define HFEM_REC(P)                                                                                                        \
    hipLaunchKernelGGL((stress_recover_kernel<NPE, P>), grid, dim3(kRecBlock), 0, (hipStream_t)stream, (int32_t)nn,       \
                       (const double2 *)X, (const double2 *)U, conn, adj_ptr, adj, m, nodal_stress, nodal_area)
    if (flags & HFEM_FLAG_PHYSICAL_GRAD) HFEM_REC(true); else HFEM_REC(false);
#undef HFEM_REC
    return launch_status(who);
}

template <int NPE>
static int zz_error(const char *who, int device, const double *X, const double *U, const int32_t *conn, int64_t ne,
                    const double *nodal_stress, const double *mat, int32_t flags, double *eta2, double *norm2,
                    double *partials, double *totals, void *stream) {
    if (ne < 0) { set_error(std::string(who) + ": negative element count"); return -1; }
    if (ne == 0) return 0;
    if (!(X && U && conn && nodal_stress && mat && eta2 && partials && totals)) { set_error(std::string(who) + ": null pointer"); return -1; }
    if (flags & ~HFEM_FLAG_PHYSICAL_GRAD) { set_error(std::string(who) + ": flags: HFEM_FLAG_PHYSICAL_GRAD or 0"); return -1; }
    if (ne >= ((int64_t)1 << 29)) { set_error(std::string(who) + ": fewer than 2^29 elements"); return -1; }
    RecMat m;
    if (int rc = rec_mat(mat, m, who)) return rc;
    if (int rc = use_device(device)) return rc;
    const int64_t nb = (ne + kRecBlock - 1) / kRecBlock;
#define HFEM_ZZ(P)                                                                                                        \
    hipLaunchKernelGGL((zz_error_kernel<NPE, P>), dim3((unsigned)nb), dim3(kRecBlock), 0, (hipStream_t)stream, ne,        \
                       (const double2 *)X, (const double2 *)U, conn, nodal_stress, m, eta2, norm2, (double2 *)partials)
    if (flags & HFEM_FLAG_PHYSICAL_GRAD) HFEM_ZZ(true); else HFEM_ZZ(false);
#undef HFEM_ZZ
    if (int rc = launch_status(who)) return rc;
    hipLaunchKernelGGL(zz_finish_kernel, dim3(1), dim3(kRecBlock), 0, (hipStream_t)stream, (const double2 *)partials, nb, totals);
    return launch_status(who);
}

}  // namespace hfem

using namespace hfem;

extern "C" int hfem_tri3_stress_recover(int device, const double *X, const double *U, const int32_t *conn, int64_t ne,
                                        int64_t nn, const int32_t *adj_ptr, const int32_t *adj, const double *mat,
                                        int32_t flags, double *nodal_stress, double *nodal_area, void *stream) {
    return stress_recover<3>("hfem_tri3_stress_recover", device, X, U, conn, ne, nn, adj_ptr, adj, mat, flags, nodal_stress,
                             nodal_area, stream);
}

extern "C" int hfem_quad4_stress_recover(int device, const double *X, const double *U, const int32_t *conn, int64_t ne,
                                         int64_t nn, const int32_t *adj_ptr, const int32_t *adj, const double *mat,
                                         int32_t flags, double *nodal_stress, double *nodal_area, void *stream) {
    return stress_recover<4>("hfem_quad4_stress_recover", device, X, U, conn, ne, nn, adj_ptr, adj, mat, flags, nodal_stress,
                             nodal_area, stream);
}

extern "C" int hfem_tri3_zz_error(int device, const double *X, const double *U, const int32_t *conn, int64_t ne,
                                  const double *nodal_stress, const double *mat, int32_t flags, double *eta2, double *norm2,
                                  double *partials, double *totals, void *stream) {
    return zz_error<3>("hfem_tri3_zz_error", device, X, U, conn, ne, nodal_stress, mat, flags, eta2, norm2, partials, totals,
                       stream);
}

extern "C" int hfem_quad4_zz_error(int device, const double *X, const double *U, const int32_t *conn, int64_t ne,
                                   const double *nodal_stress, const double *mat, int32_t flags, double *eta2, double *norm2,
                                   double *partials, double *totals, void *stream) {
    return zz_error<4>("hfem_quad4_zz_error", device, X, U, conn, ne, nodal_stress, mat, flags, eta2, norm2, partials, totals,
                       stream);
}
