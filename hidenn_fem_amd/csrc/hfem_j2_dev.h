// Small-strain J2 elastoplasticity of a TRI3 element in plane strain, linear isotropic hardening: the closed-form
// radial return against a committed state, the incremental potential, the consistent tangent as a stored record and its
// application to three rows of a direction.  Plain C++ over double2 / make_double2 and <cmath> (hfem_hyper_dev.h's rule: the
// same text compiles for the host), no dynamically indexed local array: the kernels of tri3_j2.hip compile without scratch.
//
// TRI3 has constant strain: one state point per element.  With Jg = [X0 - X2, X1 - X2] (columns), G = [U0 - U2, U1 - U2]:
//   H = G Jg^-1 (the displacement gradient, physical convention), eps = sym H, eps_zz = 0, A = |det Jg| W
//   tr = eps_xx + eps_yy,  s_tr = 2 mu (dev eps - eps^p_n)  (xx, yy, zz, xy; eps^p_zz = -eps^p_xx - eps^p_yy)
//   |s_tr| = sqrt(s_xx^2 + s_yy^2 + s_zz^2 + 2 s_xy^2),  f = |s_tr| - sqrt(2/3) (sigma_y + H alpha_n),  D = 2 mu + 2 H / 3
//   f <= 0: dgamma = 0;  f > 0: dgamma = f / D;  n = s_tr / |s_tr|
//   eps^p = eps^p_n + dgamma n,  alpha = alpha_n + sqrt(2/3) dgamma,  s = s_tr - 2 mu dgamma n,  sigma = kappa tr I + s
//   Psi = kappa tr^2 / 2 + |s_tr|^2 / (4 mu) - <f>^2 / (2 D)         (dPsi/deps = sigma)
//   theta = 1 - 2 mu dgamma / |s_tr|,  theta_bar = 1 / (1 + H / (3 mu)) - (1 - theta)   (elastic: 1 and 0)
//   dsigma = kappa tr(deps) I + 2 mu theta dev(deps) - 2 mu theta_bar (n : deps) n,  n : deps = n_xx de_xx + n_yy de_yy + 2 n_xy de_xy
// Only the in-plane dsigma enters the element force, so n_zz is not part of the tangent record.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "hfem_hyper_dev.h"

namespace hfem {

struct J2Consts {
    double mu, kappa;            // shear and bulk modulus (plane strain: kappa = lambda + 2 mu / 3)
    double sigma_y, hard;        // yield stress (> 0) and hardening modulus H (>= 0)
    double W;                    // sum of the triangle weights
};

// Jg^-1 = [[di, -bi], [-ci, ai]] and A = |det Jg| W of one element: what B depends on (the coordinates alone)
struct J2Geom {
    double ai, bi, ci, di, A;
};

__device__ __forceinline__ J2Geom j2_geom(const double2 X0, const double2 X1, const double2 X2, double W) {
    J2Geom g;
    const double a = X0.x - X2.x, b = X1.x - X2.x, c = X0.y - X2.y, d = X1.y - X2.y;
    const double det = a * d - b * c;
    const double inv = hyper_rcp(det);
    g.ai = a * inv; g.bi = b * inv; g.ci = c * inv; g.di = d * inv;
    g.A = fabs(det) * W;
    return g;
}

// eps = sym(G Jg^-1) of three corner rows: {eps_xx, eps_yy, eps_xy (tensor component)}
__device__ __forceinline__ void j2_strain(const J2Geom &g, const double2 U0, const double2 U1, const double2 U2, double &exx,
                                          double &eyy, double &exy) {
    const double g0x = U0.x - U2.x, g0y = U0.y - U2.y, g1x = U1.x - U2.x, g1y = U1.y - U2.y;
    const double h01 = g1x * g.ai - g0x * g.bi, h10 = g0y * g.di - g1y * g.ci;
    exx = g0x * g.di - g1x * g.ci;
    eyy = g1y * g.ai - g0y * g.bi;
    exy = 0.5 * (h01 + h10);
}

// A B^T sigma for an in-plane symmetric sigma: row a -> node a, minus the sum -> node 2
__device__ __forceinline__ void j2_force(const J2Geom &g, double sxx, double syy, double sxy, double2 (&q)[3]) {
    const double q0x = g.A * (sxx * g.di - sxy * g.bi), q0y = g.A * (sxy * g.di - syy * g.bi);
    const double q1x = g.A * (sxy * g.ai - sxx * g.ci), q1y = g.A * (syy * g.ai - sxy * g.ci);
    q[0] = make_double2(q0x, q0y);
    q[1] = make_double2(q1x, q1y);
    q[2] = make_double2(-(q0x + q1x), -(q0y + q1y));
}

// The result of one return map
struct J2Point {
    double sxx, syy, sxy, szz;   // stress
    double exx, eyy, exy, alpha; // the new plastic strain (tensor components) and accumulated plastic strain
    double psi;                  // the incremental potential
    double dgamma;               // 0 on the elastic branch
    double theta, theta_bar, nxx, nyy, nxy;   // the tangent record
};

__device__ __forceinline__ J2Point j2_return_map(double exx, double eyy, double exy, double pxx, double pyy, double pxy,
                                                 double alpha_n, const J2Consts &k) {
    J2Point r;
    const double rt23 = 0.81649658092772603273;             // sqrt(2/3)
    const double tr = exx + eyy, third = tr * (1.0 / 3.0), two_mu = 2.0 * k.mu;
    const double txx = two_mu * ((exx - third) - pxx), tyy = two_mu * ((eyy - third) - pyy);
    const double tzz = two_mu * (-third + (pxx + pyy)), txy = two_mu * (exy - pxy);
    const double nn = txx * txx + tyy * tyy + tzz * tzz + 2.0 * txy * txy;
    const double nrm = sqrt(nn);
    const double f = nrm - rt23 * (k.sigma_y + k.hard * alpha_n);
    const double D = two_mu + (2.0 / 3.0) * k.hard;
    const bool plastic = f > 0.0;
    const double dg = plastic ? f / D : 0.0;
    const double inrm = 1.0 / (nrm > 0.0 ? nrm : 1.0);      // nrm = 0 is elastic (sigma_y > 0): n = 0 there, never used
    const double nxx = txx * inrm, nyy = tyy * inrm, nzz = tzz * inrm, nxy = txy * inrm;
    const double back = two_mu * dg, ktr = k.kappa * tr;
    r.sxx = ktr + (txx - back * nxx);
    r.syy = ktr + (tyy - back * nyy);
    r.szz = ktr + (tzz - back * nzz);
    r.sxy = txy - back * nxy;
    r.exx = pxx + dg * nxx;
    r.eyy = pyy + dg * nyy;
    r.exy = pxy + dg * nxy;
    r.alpha = alpha_n + rt23 * dg;
    r.psi = 0.5 * k.kappa * tr * tr + nn / (4.0 * k.mu) - (plastic ? f * f / (2.0 * D) : 0.0);
    r.dgamma = dg;
    r.theta = plastic ? 1.0 - back * inrm : 1.0;
    r.theta_bar = plastic ? 1.0 / (1.0 + k.hard / (3.0 * k.mu)) - (1.0 - r.theta) : 0.0;
    r.nxx = nxx; r.nyy = nyy; r.nxy = nxy;
    return r;
}

// q_k = sum_l K_e[k][l] p_l of the stored linearisation {theta, theta_bar, n}; returns p^T K_e p
__device__ __forceinline__ double j2_tangent_apply(const J2Geom &g, const J2Consts &k, double theta, double theta_bar, double nxx,
                                                   double nyy, double nxy, const double2 p0, const double2 p1, const double2 p2,
                                                   double2 (&q)[3]) {
    double dxx, dyy, dxy;
    j2_strain(g, p0, p1, p2, dxx, dyy, dxy);
    const double tr = dxx + dyy, third = tr * (1.0 / 3.0), two_mu = 2.0 * k.mu;
    const double a = two_mu * theta, b = two_mu * theta_bar * (nxx * dxx + nyy * dyy + 2.0 * nxy * dxy), ktr = k.kappa * tr;
    const double sxx = ktr + a * (dxx - third) - b * nxx;
    const double syy = ktr + a * (dyy - third) - b * nyy;
    const double sxy = a * dxy - b * nxy;
    j2_force(g, sxx, syy, sxy, q);
    return g.A * (sxx * dxx + syy * dyy + 2.0 * sxy * dxy);
}

}  // namespace hfem

// ---------------------------------------------------------------- the J2 state handle (host side; tri3_j2.hip, cg.hip)
// Committed and trial state {eps^p_xx, eps^p_yy, eps^p_xy, alpha} and the stress {s_xx, s_yy, s_xy, s_zz} by global element id,
// [ne][4] fp64 each, and the device copy of the plan's elem_gid the update and linearisation launches read them through.
struct hfem_plan;
struct hfem_j2 {
    hfem_plan *plan = nullptr;
    int device = -1;
    int64_t ne = 0, n_slots = 0;
    int n_tiles = 0;
    hfem::J2Consts k{};
    int32_t *gid = nullptr;            // [n_tiles][elem_stride]
    double *committed = nullptr, *trial = nullptr, *stress = nullptr;   // one allocation: committed | trial | stress
    double *work = nullptr;            // the update launch's tile partials [3][n_tiles]
    size_t lds_update = 0;
};
