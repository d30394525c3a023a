// Per-point stress laws and the per-element parts of the nodal stress recovery and the ZZ indicator: what
// the kernels of csrc/recover.hip evaluate in one thread.  Plain C++ over double2 / make_double2 and <cmath> only, so that
// the very same text compiles for the host (tests/host/hyper_recover_san_main.cpp runs it under the sanitizers against the
// numbers of tests/hyper_zz_reference.py).
//
// A stress law turns the Jacobian J = [[a, b], [c, d]] (J[i][j] = d x_i / d xi_j) and G = [g0 g1] (columns du / d xi_j) of
// one point into sigma_h there:
//   LinearLaw<PHYS>  sigma_h = C (eps_xx, eps_yy, gamma_xy) of grad_u (PHYS: G J^-1, else the reference's G J^-T)
//   CauchyLaw        H = G J^-1, j = tr H + det H (= det F - 1), L = log1p(j),
//                    sigma_h = (mu (H + H^T + H H^T) + lambda L I) / (1 + j)          (= P F^T / det F, cancellation-free)
// Both carry the C the indicator's compliance S = C^-1 is taken of; for CauchyLaw that is the linearisation at F = I
// (c11 = c22 = lambda + 2 mu, c12 = lambda, c33 = mu).  A finite-strain point with j <= -1 (or NaN) is evaluated at j = 0,
// as the energy does, so nothing produces a NaN from a finite H; `j` returns the TRUE value and the caller masks the element.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "hfem_hyper_dev.h"

namespace hfem {

struct RecMat {                  // C and its inverse S (Voigt, engineering shear): by value
    double c11, c12, c22, c33;
    double s11, s12, s22, s33;
};

struct Sig3 {
    double xx, yy, xy;
};

__device__ __forceinline__ double s_form(const RecMat &m, const Sig3 &d) {   // d.S.d
    return m.s11 * d.xx * d.xx + 2.0 * m.s12 * d.xx * d.yy + m.s22 * d.yy * d.yy + m.s33 * d.xy * d.xy;
}

template <bool PHYS> struct LinearLaw {
    static constexpr bool kFinite = false;
    RecMat m;
    __device__ __forceinline__ Sig3 point(double a, double b0, double c0, double d, double2 g0, double2 g1, double &det,
                                          double &j) const {
        const double b = PHYS ? c0 : b0, c = PHYS ? b0 : c0;               // E_phys(a, b, c, d) = E_ref(a, c, b, d)
        det = a * d - b * c;
        const double inv = 1.0 / det;
        const double h00 = (g0.x * d - g1.x * b) * inv, h01 = (g1.x * a - g0.x * c) * inv;
        const double h10 = (g0.y * d - g1.y * b) * inv, h11 = (g1.y * a - g0.y * c) * inv;
        const double gam = h01 + h10;
        j = 0.0;
        return Sig3{m.c11 * h00 + m.c12 * h11, m.c12 * h00 + m.c22 * h11, m.c33 * gam};
    }
};

struct CauchyLaw {
    static constexpr bool kFinite = true;
    RecMat m;
    double lambda, mu;
    __device__ __forceinline__ Sig3 point(double a, double b, double c, double d, double2 g0, double2 g1, double &det,
                                          double &j) const {
        det = a * d - b * c;
        const double inv = hyper_rcp(det);
        const double ai = a * inv, bi = b * inv, ci = c * inv, di = d * inv;   // J^-1 = [[di, -bi], [-ci, ai]]
        const double h00 = g0.x * di - g1.x * ci, h01 = g1.x * ai - g0.x * bi;
        const double h10 = g0.y * di - g1.y * ci, h11 = g1.y * ai - g0.y * bi;
        j = (h00 + h11) + (h00 * h11 - h01 * h10);
        const double js = j > -1.0 ? j : 0.0;
        const double r = hyper_rcp(1.0 + js);
        const double lL = lambda * log1p(js);
        const double bxx = 2.0 * h00 + (h00 * h00 + h01 * h01);               // H + H^T + H H^T
        const double byy = 2.0 * h11 + (h10 * h10 + h11 * h11);
        const double bxy = (h01 + h10) + (h00 * h10 + h01 * h11);
        return Sig3{(mu * bxx + lL) * r, (mu * byy + lL) * r, mu * bxy * r};
    }
};

// C at F = I of the Neo-Hookean material and its inverse; needs mu > 0 and lambda + mu > 0 (the caller checks)
__host__ __device__ __forceinline__ CauchyLaw cauchy_law(double lambda, double mu) {
    CauchyLaw k;
    k.lambda = lambda; k.mu = mu;
    k.m.c11 = k.m.c22 = lambda + 2.0 * mu; k.m.c12 = lambda; k.m.c33 = mu;
    const double D = k.m.c11 * k.m.c22 - k.m.c12 * k.m.c12;
    k.m.s11 = k.m.c22 / D; k.m.s12 = -k.m.c12 / D; k.m.s22 = k.m.c11 / D; k.m.s33 = 1.0 / k.m.c33;
    return k;
}

__device__ __forceinline__ constexpr double rec_corner_xi(int k) { return (k == 1 || k == 2) ? 1.0 : -1.0; }
__device__ __forceinline__ constexpr double rec_corner_eta(int k) { return k >= 2 ? 1.0 : -1.0; }

template <int NPE> struct RecPoints { static constexpr int NQ = NPE == 3 ? 1 : 4; };

// sigma_h, the weights and j at the element's points: TRI3 the centroid with w = |det| / 2, QUAD4 the 2x2 Gauss points in the
// order (-,-) (+,-) (-,+) (+,+) with w_q = |det_q|; Xn, Un = the element's node rows in local order.  Returns whether every
// point has j > -1 (always true for a linear law).
template <int NPE, class Law>
__device__ __forceinline__ bool element_points(const double2 (&Xn)[NPE], const double2 (&Un)[NPE], const Law &law,
                                               Sig3 (&sg)[RecPoints<NPE>::NQ], double (&w)[RecPoints<NPE>::NQ],
                                               double (&jq)[RecPoints<NPE>::NQ]) {
    bool ok = true;
    if constexpr (NPE == 3) {
        double det;
        sg[0] = law.point(Xn[0].x - Xn[2].x, Xn[1].x - Xn[2].x, Xn[0].y - Xn[2].y, Xn[1].y - Xn[2].y,
                          make_double2(Un[0].x - Un[2].x, Un[0].y - Un[2].y),
                          make_double2(Un[1].x - Un[2].x, Un[1].y - Un[2].y), det, jq[0]);
        w[0] = 0.5 * fabs(det);
        if (Law::kFinite) ok = jq[0] > -1.0;
    } else {
        const double gp = 0.57735026918962576451;   // 1/sqrt(3)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double xi = (q & 1) ? gp : -gp, eta = (q & 2) ? gp : -gp;
            double D0[4], D1[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                D0[k] = 0.25 * rec_corner_xi(k) * (1.0 + rec_corner_eta(k) * eta);
                D1[k] = 0.25 * rec_corner_eta(k) * (1.0 + rec_corner_xi(k) * xi);
            }
            double a = 0.0, b = 0.0, c = 0.0, d = 0.0;
            double2 g0 = make_double2(0.0, 0.0), g1 = make_double2(0.0, 0.0);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                a += Xn[k].x * D0[k]; b += Xn[k].x * D1[k]; c += Xn[k].y * D0[k]; d += Xn[k].y * D1[k];
                g0.x += Un[k].x * D0[k]; g0.y += Un[k].y * D0[k]; g1.x += Un[k].x * D1[k]; g1.y += Un[k].y * D1[k];
            }
            double det;
            sg[q] = law.point(a, b, c, d, g0, g1, det, jq[q]);
            w[q] = fabs(det);
            if (Law::kFinite) ok = ok && jq[q] > -1.0;
        }
    }
    return ok;
}

// eta_e^2 = int_e (sigma* - sigma_h).S.(sigma* - sigma_h) and |u_h|_e^2 = int_e sigma_h.S.sigma_h of one element from the
// recovered stress ss at its nodes and sigma_h, w at its points.  TRI3: the exact integral of the linear d(x) = sum_k N_k d_k,
//   A/12 [sum_k d_k.S.d_k + (sum_k d_k).S.(sum_k d_k)],  A = w[0];  QUAD4: the 2x2 rule.
template <int NPE>
__device__ __forceinline__ void zz_indicator(const Sig3 (&ss)[NPE], const Sig3 (&sg)[RecPoints<NPE>::NQ],
                                             const double (&w)[RecPoints<NPE>::NQ], const RecMat &m, double &ve, double &vn) {
    ve = 0.0; vn = 0.0;
    if constexpr (NPE == 3) {
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
                const double N = 0.25 * (1.0 + rec_corner_xi(k) * xi) * (1.0 + rec_corner_eta(k) * eta);
                d.xx += N * ss[k].xx; d.yy += N * ss[k].yy; d.xy += N * ss[k].xy;
            }
            ve += w[q] * s_form(m, d);
            vn += w[q] * s_form(m, sg[q]);
        }
    }
}

// The finite-strain element of the indicator with the inversion rule applied: an element with a point at j <= -1 (or NaN)
// has eta_e^2 = +inf and adds 0 to |u_h|^2 (selects: a NaN in its sigma_h does not get through); jmin = min_q j_q with the
// true values (fmin: a NaN j is skipped, as in the energy's min J).
template <int NPE>
__device__ __forceinline__ bool hyper_zz_element(const double2 (&Xn)[NPE], const double2 (&Un)[NPE], const Sig3 (&ss)[NPE],
                                                 const CauchyLaw &law, double &ve, double &vn, double &jmin) {
    constexpr int NQ = RecPoints<NPE>::NQ;
    Sig3 sg[NQ];
    double w[NQ], jq[NQ];
    const bool ok = element_points<NPE>(Xn, Un, law, sg, w, jq);
    zz_indicator<NPE>(ss, sg, w, law.m, ve, vn);
    ve = ok ? ve : (double)INFINITY;
    vn = ok ? vn : 0.0;
    jmin = jq[0];
#pragma unroll
    for (int q = 1; q < NQ; ++q) jmin = fmin(jmin, jq[q]);
    return ok;
}

}  // namespace hfem
