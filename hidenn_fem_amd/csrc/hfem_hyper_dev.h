// Compressible Neo-Hookean TRI3 element, the per-thread part of its finishing reduction and its tangent
// (DESIGN 18).  Plain C++ over double2 / make_double2 and <cmath> only, so that the very same text compiles for the host
// (tests/host/hyper_san_main.cpp and hyper_tangent_san_main.cpp run it under the sanitizers against numbers of
// tests/hyper_reference.py and tests/newton_reference.py).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace hfem {

struct HyperConsts {
    double lambda, mu;           // Lame constants (plane="stress": the effective lambda E nu / (1 - nu^2))
    double W;                    // sum of the triangle weights
    double Bk[6];                // body-force table [3][2], EnergyLoss2D's
};

// 1 / x to ~1 ulp on the device: the hardware seed and two Newton steps (hfem_device.h's fast_rcp) instead of the IEEE
// division sequence (T1M: 22.9 -> 22.6 us per launch); the host build divides.
__device__ __forceinline__ double hyper_rcp(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    double r = __builtin_amdgcn_rcp(x);
    double e = __builtin_fma(-x, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-x, r, 1.0);
    return __builtin_fma(r, e, r);
#else
    return 1.0 / x;
#endif
}

// One element.  Jg = [X0 - X2, X1 - X2] (columns), G = [U0 - U2, U1 - U2]:
//   H = G Jg^-1 (the displacement gradient), F = I + H, j = tr H + det H = J - 1, L = log1p(j)
//   psi = mu (tr H + H:H / 2 - L) + lambda L^2 / 2
//   P = mu (H + H^T F^-T) + lambda L F^-T                       (first Piola-Kirchhoff; F^-T = adj(F)^T / (1 + j))
//   e = A psi - |det Jg| beta,  A = |det Jg| W,  beta = sum_k U_k . B_k
//   de/dG  = A P Jg^-T                                          (column a -> node a, minus the column sum -> node 2)
//   de/dJg = (A (psi I - H^T P) - |det Jg| beta I) Jg^-T        (likewise), and -|det Jg| B_k joins de/dU_k
// These H-based forms carry no cancellation: the textbook mu/2 (tr F^T F - 2) - mu ln J loses 1e-16 / strain^2.
// Inverted deformation (j <= -1, or NaN): e = +inf, all twelve gradient entries 0 -- selects on ordinary arithmetic (the
// element is evaluated at j = 0 instead, so nothing produces a NaN).  Jm1 returns the true j.
__device__ __forceinline__ double neo_hookean_element(const double2 X0, const double2 X1, const double2 X2, const double2 U0,
                                                      const double2 U1, const double2 U2, const HyperConsts &k,
                                                      double2 (&gx)[3], double2 (&gu)[3], double &Jm1) {
    const double a = X0.x - X2.x, b = X1.x - X2.x, c = X0.y - X2.y, d = X1.y - X2.y;
    const double det = a * d - b * c;
    const double inv = hyper_rcp(det);
    const double ai = a * inv, bi = b * inv, ci = c * inv, di = d * inv;      // Jg^-1 = [[di, -bi], [-ci, ai]]
    const double g0x = U0.x - U2.x, g0y = U0.y - U2.y, g1x = U1.x - U2.x, g1y = U1.y - U2.y;
    const double h00 = g0x * di - g1x * ci, h01 = g1x * ai - g0x * bi;
    const double h10 = g0y * di - g1y * ci, h11 = g1y * ai - g0y * bi;
    const double tr = h00 + h11;
    const double j = tr + (h00 * h11 - h01 * h10);
    Jm1 = j;
    const bool ok = j > -1.0;
    const double js = ok ? j : 0.0;
    const double L = log1p(js);
    const double r = hyper_rcp(1.0 + js);
    const double hh = h00 * h00 + h01 * h01 + h10 * h10 + h11 * h11;
    const double psi = k.mu * (tr + 0.5 * hh - L) + 0.5 * k.lambda * L * L;
    const double t00 = (1.0 + h11) * r, t01 = -h10 * r, t10 = -h01 * r, t11 = (1.0 + h00) * r;   // F^-T
    const double lL = k.lambda * L;
    const double p00 = k.mu * (h00 + h00 * t00 + h10 * t10) + lL * t00;
    const double p01 = k.mu * (h01 + h00 * t01 + h10 * t11) + lL * t01;
    const double p10 = k.mu * (h10 + h01 * t00 + h11 * t10) + lL * t10;
    const double p11 = k.mu * (h11 + h01 * t01 + h11 * t11) + lL * t11;
    const double ad = fabs(det), A = ad * k.W;
    const double beta = U0.x * k.Bk[0] + U0.y * k.Bk[1] + U1.x * k.Bk[2] + U1.y * k.Bk[3] + U2.x * k.Bk[4] + U2.y * k.Bk[5];
    const double e = A * psi - ad * beta;
    const double s = ok ? 1.0 : 0.0, sA = s * A, sad = s * ad;
    // de/dG = A P Jg^-T, Jg^-T = [[di, -ci], [-bi, ai]]
    const double dg0x = sA * (p00 * di - p01 * bi), dg0y = sA * (p10 * di - p11 * bi);
    const double dg1x = sA * (p01 * ai - p00 * ci), dg1y = sA * (p11 * ai - p10 * ci);
    gu[0] = make_double2(dg0x - sad * k.Bk[0], dg0y - sad * k.Bk[1]);
    gu[1] = make_double2(dg1x - sad * k.Bk[2], dg1y - sad * k.Bk[3]);
    gu[2] = make_double2(-(dg0x + dg1x) - sad * k.Bk[4], -(dg0y + dg1y) - sad * k.Bk[5]);
    // Q = A (psi I - H^T P) - |det| beta I, de/dJg = Q Jg^-T
    const double diag = sA * psi - sad * beta;
    const double q00 = diag - sA * (h00 * p00 + h10 * p10), q01 = -sA * (h00 * p01 + h10 * p11);
    const double q10 = -sA * (h01 * p00 + h11 * p10), q11 = diag - sA * (h01 * p01 + h11 * p11);
    const double da = q00 * di - q01 * bi, db = q01 * ai - q00 * ci;          // d/d(a, b): row 0 of Jg (x components)
    const double dc = q10 * di - q11 * bi, dd = q11 * ai - q10 * ci;          // d/d(c, d): row 1 (y components)
    gx[0] = make_double2(da, dc);
    gx[1] = make_double2(db, dd);
    gx[2] = make_double2(-(da + db), -(dc + dd));
    return ok ? e : (double)INFINITY;
}

// The tangent of one element at a linearisation point, in two pieces: the state, computed once, and its
// application to three rows of a direction p.  With T = F^-T and dH = dG Jg^-1, dG = [p0 - p2, p1 - p2]:
//   dP = mu dH + (mu - lambda L) T dH^T T + lambda (T : dH) T
//   q  = A dP Jg^-T                                            (column a -> node a, minus the column sum -> node 2)
// so that sum_k p_k . q_k = p^T K_e p.  Dead loads do not enter.  The inversion rule is neo_hookean_element's: an element
// with j <= -1 (or NaN) is evaluated at j = 0 and its six outputs are multiplied by 0 (sA = 0); j keeps the true value.
struct HyperTangent {
    double ai, bi, ci, di;       // Jg^-1 = [[di, -bi], [-ci, ai]]
    double t00, t01, t10, t11;   // T = F^-T
    double c;                    // mu - lambda L
    double sA;                   // A = |det Jg| W, 0 for an inverted element
    double j;                    // J - 1
};

__device__ __forceinline__ HyperTangent hyper_tangent_state(const double2 X0, const double2 X1, const double2 X2, const double2 U0,
                                                            const double2 U1, const double2 U2, const HyperConsts &k) {
    HyperTangent t;
    const double a = X0.x - X2.x, b = X1.x - X2.x, c = X0.y - X2.y, d = X1.y - X2.y;
    const double det = a * d - b * c;
    const double inv = hyper_rcp(det);
    t.ai = a * inv; t.bi = b * inv; t.ci = c * inv; t.di = d * inv;
    const double g0x = U0.x - U2.x, g0y = U0.y - U2.y, g1x = U1.x - U2.x, g1y = U1.y - U2.y;
    const double h00 = g0x * t.di - g1x * t.ci, h01 = g1x * t.ai - g0x * t.bi;
    const double h10 = g0y * t.di - g1y * t.ci, h11 = g1y * t.ai - g0y * t.bi;
    const double j = (h00 + h11) + (h00 * h11 - h01 * h10);
    t.j = j;
    const bool ok = j > -1.0;
    const double js = ok ? j : 0.0;
    const double r = hyper_rcp(1.0 + js);
    t.t00 = (1.0 + h11) * r; t.t01 = -h10 * r; t.t10 = -h01 * r; t.t11 = (1.0 + h00) * r;
    t.c = k.mu - k.lambda * log1p(js);
    t.sA = ok ? fabs(det) * k.W : 0.0;
    return t;
}

// q_k = sum_l K_e[k][l] p_l for the three corners; returns p^T K_e p.
__device__ __forceinline__ double hyper_tangent_apply(const HyperTangent &t, const HyperConsts &k, const double2 p0, const double2 p1,
                                                      const double2 p2, double2 (&q)[3]) {
    const double g0x = p0.x - p2.x, g0y = p0.y - p2.y, g1x = p1.x - p2.x, g1y = p1.y - p2.y;
    const double d00 = g0x * t.di - g1x * t.ci, d01 = g1x * t.ai - g0x * t.bi;         // dH
    const double d10 = g0y * t.di - g1y * t.ci, d11 = g1y * t.ai - g0y * t.bi;
    // M = T dH^T, then M T
    const double m00 = t.t00 * d00 + t.t01 * d01, m01 = t.t00 * d10 + t.t01 * d11;
    const double m10 = t.t10 * d00 + t.t11 * d01, m11 = t.t10 * d10 + t.t11 * d11;
    const double lt = k.lambda * (t.t00 * d00 + t.t01 * d01 + t.t10 * d10 + t.t11 * d11);
    const double s00 = k.mu * d00 + t.c * (m00 * t.t00 + m01 * t.t10) + lt * t.t00;
    const double s01 = k.mu * d01 + t.c * (m00 * t.t01 + m01 * t.t11) + lt * t.t01;
    const double s10 = k.mu * d10 + t.c * (m10 * t.t00 + m11 * t.t10) + lt * t.t10;
    const double s11 = k.mu * d11 + t.c * (m10 * t.t01 + m11 * t.t11) + lt * t.t11;
    // q = A dP Jg^-T, Jg^-T = [[di, -ci], [-bi, ai]]
    const double q0x = t.sA * (s00 * t.di - s01 * t.bi), q0y = t.sA * (s10 * t.di - s11 * t.bi);
    const double q1x = t.sA * (s01 * t.ai - s00 * t.ci), q1y = t.sA * (s11 * t.ai - s10 * t.ci);
    q[0] = make_double2(q0x, q0y);
    q[1] = make_double2(q1x, q1y);
    q[2] = make_double2(-(q0x + q1x), -(q0y + q1y));
    return g0x * q0x + g0y * q0y + g1x * q1x + g1y * q1y;
}

// The finishing launch's per-thread part over the tile partials work[3][n] = {energy, min J, inverted count}: thread tid of
// nthr takes tiles tid, tid + nthr, ... in ascending order (sum_partials_kernel's order for the energy).
__device__ __forceinline__ void hyper_finish_thread(const double *work, int n, int tid, int nthr, double &e, double &mj,
                                                    double &cnt) {
    e = 0.0; mj = (double)INFINITY; cnt = 0.0;
    for (int i = tid; i < n; i += nthr) {
        e += work[i];
        mj = fmin(mj, work[n + i]);
        cnt += work[2 * n + i];
    }
}

}  // namespace hfem
