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
//
// The same two kernels at finite strain: the stress law CauchyLaw of hfem_recover_hyper_dev.h gives the Cauchy
// stress of the Neo-Hookean material, S is the compliance at F = I, an inverted element (j <= -1 or NaN at a point) gets weight 0
// in the projection and eta_e^2 = +inf, and the totals become {sum eta^2, sum |u_h|^2, min det F, inverted elements}.
#include <hip/hip_runtime.h>

#include "hfem_device.h"
#include "hfem_quad4_dev.h"
#include "hfem_recover_hyper_dev.h"

namespace hfem {

constexpr int kRecBlock = 256;

template <int NPE>
__device__ __forceinline__ void gather_element(const double2 *__restrict__ X, const double2 *__restrict__ U,
                                               const int32_t *__restrict__ conn, int64_t e, double2 (&Xn)[NPE],
                                               double2 (&Un)[NPE], int32_t (&nd)[NPE]) {
#pragma unroll
    for (int k = 0; k < NPE; ++k) nd[k] = conn[NPE * e + k];
#pragma unroll
    for (int k = 0; k < NPE; ++k) { Xn[k] = X[nd[k]]; Un[k] = U[nd[k]]; }
}

// The frame of both kernels is parametrised by the stress law (hfem_recover_hyper_dev.h).  A finite-strain law adds the
// inversion rule and the recovered J; `if constexpr (Law::kFinite)` keeps all of that out of the linear instances.
template <int NPE, class Law>
__global__ __launch_bounds__(kRecBlock) void stress_recover_kernel(
    int32_t nn, const double2 *__restrict__ X, const double2 *__restrict__ U, const int32_t *__restrict__ conn,
    const int32_t *__restrict__ adj_ptr, const int32_t *__restrict__ adj, Law law, double *__restrict__ nodal_stress,
    double *__restrict__ nodal_area, double *__restrict__ nodal_J) {
    constexpr int NQ = RecPoints<NPE>::NQ;
    const int64_t n = (int64_t)blockIdx.x * kRecBlock + threadIdx.x;
    if (n >= nn) return;
    double sxx = 0.0, syy = 0.0, sxy = 0.0, den = 0.0;
    [[maybe_unused]] double sJ = 0.0;
    const int32_t i0 = adj_ptr[n], i1 = adj_ptr[n + 1];
    for (int32_t i = i0; i < i1; ++i) {
        const int32_t ec = adj[i], e = ec >> 2, c = ec & 3;
        double2 Xn[NPE], Un[NPE];
        int32_t nd[NPE];
        gather_element<NPE>(X, U, conn, e, Xn, Un, nd);
        Sig3 sg[NQ];
        double w[NQ], jq[NQ];
        const bool ok = element_points<NPE>(Xn, Un, law, sg, w, jq);
        if (Law::kFinite && !ok) continue;                                 // an inverted element: no numerator, no denominator
        // N_c(q) of the run-time corner c from the corner signs (selects), never by indexing a local array: that would
        // put the array in scratch
        [[maybe_unused]] const double cx = corner_xi(c), ce = corner_eta(c), gp = 0.57735026918962576451;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            double N = 1.0 / 3.0;                                          // TRI3: N_c at the centroid
            if constexpr (NPE == 4) N = 0.25 * (1.0 + cx * ((q & 1) ? gp : -gp)) * (1.0 + ce * ((q & 2) ? gp : -gp));
            const double wn = w[q] * N;
            sxx += wn * sg[q].xx; syy += wn * sg[q].yy; sxy += wn * sg[q].xy;
            if constexpr (Law::kFinite) sJ += wn * (1.0 + jq[q]);
            den += wn;
        }
    }
    // a node that no element references (finite strain: or only inverted ones) has no stress to recover: zeros, lumped area 0
    const bool has = Law::kFinite ? den > 0.0 : i1 > i0;
    nodal_stress[3 * n] = has ? sxx / den : 0.0;
    nodal_stress[3 * n + 1] = has ? syy / den : 0.0;
    nodal_stress[3 * n + 2] = has ? sxy / den : 0.0;
    if constexpr (Law::kFinite)
        if (nodal_J) nodal_J[n] = has ? sJ / den : 0.0;
    if (nodal_area) nodal_area[n] = den;
}

__device__ __forceinline__ double block_min(double v, double *scratch) {   // valid in thread 0
    v = wave_min(v);
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kRecBlock / 64; ++w) v = fmin(v, scratch[w]);
    return v;
}

// partials: per block {sum eta_e^2, sum |u_h|_e^2}; a finite-strain law: {..., min j + 1 over all points, inverted elements}
template <int NPE, class Law>
__global__ __launch_bounds__(kRecBlock) void zz_error_kernel(int64_t ne, const double2 *__restrict__ X,
                                                             const double2 *__restrict__ U, const int32_t *__restrict__ conn,
                                                             const double *__restrict__ nodal_stress, Law law,
                                                             double *__restrict__ eta2, double *__restrict__ norm2,
                                                             double2 *__restrict__ partials) {
    constexpr int NQ = RecPoints<NPE>::NQ;
    __shared__ double red_e[kRecBlock / 64], red_n[kRecBlock / 64];
    const int64_t e = (int64_t)blockIdx.x * kRecBlock + threadIdx.x;
    double ve = 0.0, vn = 0.0;
    [[maybe_unused]] double vj = (double)INFINITY, vc = 0.0;
    if (e < ne) {
        double2 Xn[NPE], Un[NPE];
        int32_t nd[NPE];
        gather_element<NPE>(X, U, conn, e, Xn, Un, nd);
        Sig3 ss[NPE];
#pragma unroll
        for (int k = 0; k < NPE; ++k)
            ss[k] = Sig3{nodal_stress[3 * (int64_t)nd[k]], nodal_stress[3 * (int64_t)nd[k] + 1], nodal_stress[3 * (int64_t)nd[k] + 2]};
        if constexpr (Law::kFinite) {
            vc = hyper_zz_element<NPE>(Xn, Un, ss, law, ve, vn, vj) ? 0.0 : 1.0;
        } else {
            Sig3 sg[NQ];
            double w[NQ], jq[NQ];
            element_points<NPE>(Xn, Un, law, sg, w, jq);
            zz_indicator<NPE>(ss, sg, w, law.m, ve, vn);
        }
        eta2[e] = ve;
        if (norm2) norm2[e] = vn;
    }
    const double te = block_sum(ve, red_e), tn = block_sum(vn, red_n);
    if constexpr (Law::kFinite) {
        __shared__ double red_j[kRecBlock / 64], red_c[kRecBlock / 64];
        const double tj = block_min(vj, red_j), tc = block_sum(vc, red_c);
        if (threadIdx.x == 0) {
            partials[2 * blockIdx.x] = make_double2(te, tn);
            partials[2 * blockIdx.x + 1] = make_double2(1.0 + tj, tc);
        }
    } else {
        if (threadIdx.x == 0) partials[blockIdx.x] = make_double2(te, tn);
    }
}

// totals = {sum eta_e^2, sum |u_h|_e^2} (FINITE: and {min j + 1, inverted elements}): thread t adds partials t, t + 256, ... in
// ascending index, then the block tree -- one fixed order for a given block count
template <bool FINITE>
__global__ __launch_bounds__(kRecBlock) void zz_finish_kernel(const double2 *__restrict__ partials, int64_t n,
                                                              double *__restrict__ totals) {
    __shared__ double red_e[kRecBlock / 64], red_n[kRecBlock / 64];
    double ve = 0.0, vn = 0.0;
    [[maybe_unused]] double vj = (double)INFINITY, vc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kRecBlock) {
        const double2 p = partials[FINITE ? 2 * i : i];
        ve += p.x; vn += p.y;
        if constexpr (FINITE) {
            const double2 r = partials[2 * i + 1];
            vj = fmin(vj, r.x); vc += r.y;
        }
    }
    const double te = block_sum(ve, red_e), tn = block_sum(vn, red_n);
    if (threadIdx.x == 0) { totals[0] = te; totals[1] = tn; }
    if constexpr (FINITE) {
        __shared__ double red_j[kRecBlock / 64], red_c[kRecBlock / 64];
        const double tj = block_min(vj, red_j), tc = block_sum(vc, red_c);
        if (threadIdx.x == 0) { totals[2] = tj; totals[3] = tc; }
    }
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

// the two launches of the frame for one law (no status check: the callers do that)
template <int NPE, class Law>
static void launch_recover(const double *X, const double *U, const int32_t *conn, int64_t nn, const int32_t *adj_ptr,
                           const int32_t *adj, const Law &law, double *nodal_stress, double *nodal_area, double *nodal_J,
                           void *stream) {
    const dim3 grid((unsigned)((nn + kRecBlock - 1) / kRecBlock));
    hipLaunchKernelGGL((stress_recover_kernel<NPE, Law>), grid, dim3(kRecBlock), 0, (hipStream_t)stream, (int32_t)nn,
                       (const double2 *)X, (const double2 *)U, conn, adj_ptr, adj, law, nodal_stress, nodal_area, nodal_J);
}

template <int NPE, class Law>
static void launch_zz(const double *X, const double *U, const int32_t *conn, int64_t ne, const double *nodal_stress,
                      const Law &law, double *eta2, double *norm2, double *partials, void *stream) {
    const int64_t nb = (ne + kRecBlock - 1) / kRecBlock;
    hipLaunchKernelGGL((zz_error_kernel<NPE, Law>), dim3((unsigned)nb), dim3(kRecBlock), 0, (hipStream_t)stream, ne,
                       (const double2 *)X, (const double2 *)U, conn, nodal_stress, law, eta2, norm2, (double2 *)partials);
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
    if (flags & HFEM_FLAG_PHYSICAL_GRAD)
        launch_recover<NPE>(X, U, conn, nn, adj_ptr, adj, LinearLaw<true>{m}, nodal_stress, nodal_area, nullptr, stream);
    else
        launch_recover<NPE>(X, U, conn, nn, adj_ptr, adj, LinearLaw<false>{m}, nodal_stress, nodal_area, nullptr, stream);
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
    if (flags & HFEM_FLAG_PHYSICAL_GRAD) launch_zz<NPE>(X, U, conn, ne, nodal_stress, LinearLaw<true>{m}, eta2, norm2, partials, stream);
    else launch_zz<NPE>(X, U, conn, ne, nodal_stress, LinearLaw<false>{m}, eta2, norm2, partials, stream);
    if (int rc = launch_status(who)) return rc;
    hipLaunchKernelGGL(zz_finish_kernel<false>, dim3(1), dim3(kRecBlock), 0, (hipStream_t)stream, (const double2 *)partials, nb, totals);
    return launch_status(who);
}

// ---- finite strain: the same launches with the Cauchy law; lame = {lambda, mu} on the host
static int cauchy_mat(const double *lame, CauchyLaw &law, const char *who) {
    if (!(lame[1] > 0.0) || !(lame[0] + lame[1] > 0.0)) {
        set_error(std::string(who) + ": lame is not positive definite (mu > 0 and lambda + mu > 0)");
        return -1;
    }
    law = cauchy_law(lame[0], lame[1]);
    return 0;
}

template <int NPE>
static int hyper_stress_recover(const char *who, int device, const double *X, const double *U, const int32_t *conn, int64_t ne,
                                int64_t nn, const int32_t *adj_ptr, const int32_t *adj, const double *lame,
                                double *nodal_stress, double *nodal_J, double *nodal_area, void *stream) {
    if (ne < 0 || nn < 0) { set_error(std::string(who) + ": negative count"); return -1; }
    if (ne == 0 || nn == 0) return 0;
    if (!(X && U && conn && adj_ptr && adj && lame && nodal_stress)) { set_error(std::string(who) + ": null pointer"); return -1; }
    if (ne >= ((int64_t)1 << 29) || nn > INT32_MAX - kRecBlock) {
        set_error(std::string(who) + ": fewer than 2^29 elements (adjacency entries are e << 2 | c) and int32 node ids");
        return -1;
    }
    CauchyLaw law;
    if (int rc = cauchy_mat(lame, law, who)) return rc;
    if (int rc = use_device(device)) return rc;
    launch_recover<NPE>(X, U, conn, nn, adj_ptr, adj, law, nodal_stress, nodal_area, nodal_J, stream);
    return launch_status(who);
}

template <int NPE>
static int hyper_zz_error(const char *who, int device, const double *X, const double *U, const int32_t *conn, int64_t ne,
                          const double *nodal_stress, const double *lame, double *eta2, double *norm2, double *partials,
                          double *totals, void *stream) {
    if (ne < 0) { set_error(std::string(who) + ": negative element count"); return -1; }
    if (ne == 0) return 0;
    if (!(X && U && conn && nodal_stress && lame && eta2 && partials && totals)) { set_error(std::string(who) + ": null pointer"); return -1; }
    if (ne >= ((int64_t)1 << 29)) { set_error(std::string(who) + ": fewer than 2^29 elements"); return -1; }
    CauchyLaw law;
    if (int rc = cauchy_mat(lame, law, who)) return rc;
    if (int rc = use_device(device)) return rc;
    const int64_t nb = (ne + kRecBlock - 1) / kRecBlock;
    launch_zz<NPE>(X, U, conn, ne, nodal_stress, law, eta2, norm2, partials, stream);
    if (int rc = launch_status(who)) return rc;
    hipLaunchKernelGGL(zz_finish_kernel<true>, dim3(1), dim3(kRecBlock), 0, (hipStream_t)stream, (const double2 *)partials, nb, totals);
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

extern "C" int hfem_tri3_hyper_stress_recover(int device, const double *X, const double *U, const int32_t *conn, int64_t ne,
                                              int64_t nn, const int32_t *adj_ptr, const int32_t *adj, const double *lame,
                                              double *nodal_stress, double *nodal_J, double *nodal_area, void *stream) {
    return hyper_stress_recover<3>("hfem_tri3_hyper_stress_recover", device, X, U, conn, ne, nn, adj_ptr, adj, lame,
                                   nodal_stress, nodal_J, nodal_area, stream);
}

extern "C" int hfem_quad4_hyper_stress_recover(int device, const double *X, const double *U, const int32_t *conn, int64_t ne,
                                               int64_t nn, const int32_t *adj_ptr, const int32_t *adj, const double *lame,
                                               double *nodal_stress, double *nodal_J, double *nodal_area, void *stream) {
    return hyper_stress_recover<4>("hfem_quad4_hyper_stress_recover", device, X, U, conn, ne, nn, adj_ptr, adj, lame,
                                   nodal_stress, nodal_J, nodal_area, stream);
}

extern "C" int hfem_tri3_hyper_zz_error(int device, const double *X, const double *U, const int32_t *conn, int64_t ne,
                                        const double *nodal_stress, const double *lame, double *eta2, double *norm2,
                                        double *partials, double *totals, void *stream) {
    return hyper_zz_error<3>("hfem_tri3_hyper_zz_error", device, X, U, conn, ne, nodal_stress, lame, eta2, norm2, partials,
                             totals, stream);
}

extern "C" int hfem_quad4_hyper_zz_error(int device, const double *X, const double *U, const int32_t *conn, int64_t ne,
                                         const double *nodal_stress, const double *lame, double *eta2, double *norm2,
                                         double *partials, double *totals, void *stream) {
    return hyper_zz_error<4>("hfem_quad4_hyper_zz_error", device, X, U, conn, ne, nodal_stress, lame, eta2, norm2, partials,
                             totals, stream);
}
