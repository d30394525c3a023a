// Compressible Neo-Hookean QUAD4 element: the finite-strain energy of hfem_hyper_dev.h at the 2x2 Gauss points
// of the bilinear quadrilateral, with its hand-derived gradients, and its tangent.  Plain C++ over double2 /
// make_double2 and <cmath> only, so that the very same text compiles for the host (tests/host/quad4_hyper_san_main.cpp and
// quad4_hyper_tangent_san_main.cpp run it under the sanitizers against the numbers of tests/quad4_hyper_reference.py and
// tests/quad4_newton_reference.py).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "hfem_hyper_dev.h"

namespace hfem {

struct Quad4HyperConsts {
    double lambda, mu;           // Lame constants (plane="stress": the effective lambda E nu / (1 - nu^2))
    double2 b[4];                // body force at the four Gauss points (reference coordinates), EnergyLoss2D._quad4_body's
};

// the four determinants of a cell inverted with ONE reciprocal (hfem_quad4_dev.h's rcp4 over hyper_rcp: host-compilable)
__device__ __forceinline__ void hyper_rcp4(const double (&dt)[4], double (&iv)[4]) {
    const double p01 = dt[0] * dt[1], p23 = dt[2] * dt[3];
    const double r = hyper_rcp(p01 * p23);
    const double r01 = r * p23, r23 = r * p01;                             // 1/(d0 d1), 1/(d2 d3)
    iv[0] = r01 * dt[1]; iv[1] = r01 * dt[0]; iv[2] = r23 * dt[3]; iv[3] = r23 * dt[2];
}

// One cell, corners counter-clockwise from (-1,-1) (either orientation works: |det J_q|), points q in the order
// (-,-) (+,-) (-,+) (+,+) at xi, eta = +-1/sqrt(3), weights 1.  In the bilinear coefficient form of quad4_element, for a nodal
// field v_0..v_3:  4 dv/dxi = c1 + eta c3,  4 dv/deta = c2 + xi c3,  4 v = c0 + xi c1 + eta c2 + xi eta c3  with
//   c0 = v0+v1+v2+v3,  c1 = (v1-v0)+(v2-v3),  c2 = (v3-v0)+(v2-v1),  c3 = (v2-v3)-(v1-v0).
// J_q = [[a, b], [c, d]] (columns dX/dxi, dX/deta) and G_q = [g0, g1] are taken on the UNSCALED coefficients: H = G J^-1 does
// not see the common factor 4 and |det| sees 16, so the point weight is 1/16.  Per point, neo_hookean_element's forms:
//   H = G J^-1,  j = tr H + det H (= det F - 1),  L = log1p(j),  psi = mu (tr H + H:H / 2 - L) + lambda L^2 / 2
//   P = mu (H + H^T F^-T) + lambda L F^-T,  A = |det J| / 16,  beta = b_q . u_h(xi_q)
//   e_q = A (psi - beta),  de/dG = A P J^-T,  de/dJ = A ((psi - beta) I - H^T P) J^-T,  de/du_h = -A b_q
// The cotangents are accumulated per COEFFICIENT, point by point (3 coefficients x 4 components live across the points, plus
// c0 of the displacement with a body force; the c3 part as +-u +-v, scaled by 1/sqrt(3) once), and spread to the corners
// with +-1 at the end.
// Inversion rule: a point with j_q <= -1 (or NaN) is evaluated at j = 0; a cell with such a point has energy +inf and all
// sixteen gradient entries 0 (selects on ordinary arithmetic: nothing produces a NaN).  jmin returns min_q j_q with the TRUE
// values, inverted whether the cell has such a point; jq (host checks only, NULL on the device) receives the four j_q.
template <bool HASB>
__device__ __forceinline__ double quad4_neo_hookean_element(const double2 (&Xn)[4], const double2 (&Un)[4],
                                                            const Quad4HyperConsts &k, double2 (&gx)[4], double2 (&gu)[4],
                                                            double &jmin, bool &inverted, double *jq = nullptr) {
    const double gp = 0.57735026918962576451;   // 1/sqrt(3)
    double c1[4], c2[4], c3[4];                  // components: x, y, ux, uy
    {
        const double v[4][4] = {{Xn[0].x, Xn[1].x, Xn[2].x, Xn[3].x}, {Xn[0].y, Xn[1].y, Xn[2].y, Xn[3].y},
                                {Un[0].x, Un[1].x, Un[2].x, Un[3].x}, {Un[0].y, Un[1].y, Un[2].y, Un[3].y}};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double s = v[i][1] - v[i][0], t = v[i][2] - v[i][3];
            c1[i] = s + t;
            c3[i] = t - s;
            c2[i] = (v[i][3] - v[i][0]) + (v[i][2] - v[i][1]);
        }
    }
    const double c0x = HASB ? (Un[0].x + Un[1].x) + (Un[2].x + Un[3].x) : 0.0;
    const double c0y = HASB ? (Un[0].y + Un[1].y) + (Un[2].y + Un[3].y) : 0.0;
    // J(xi, eta) is affine: a, c depend on eta only, b, d on xi only -- two values each; the four determinants first, one
    // reciprocal for all of them
    const double am = c1[0] - gp * c3[0], ap = c1[0] + gp * c3[0], cm = c1[1] - gp * c3[1], cp = c1[1] + gp * c3[1];
    const double bm = c2[0] - gp * c3[0], bp = c2[0] + gp * c3[0], dm = c2[1] - gp * c3[1], dp = c2[1] + gp * c3[1];
    const double dets[4] = {am * dm - bm * cm, am * dp - bp * cm, ap * dm - bm * cp, ap * dp - bp * cp};
    double invs[4];
    hyper_rcp4(dets, invs);
    double D1[4] = {0.0, 0.0, 0.0, 0.0}, D2[4] = {0.0, 0.0, 0.0, 0.0}, S3[4] = {0.0, 0.0, 0.0, 0.0};   // cotangents of c1, c2, c3 / gp
    double D0x = 0.0, D0y = 0.0;                                                                      // ... of c0 (ux, uy)
    double e = 0.0, jm = (double)INFINITY;
    bool all_ok = true;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double xi = (q & 1) ? gp : -gp, eta = (q & 2) ? gp : -gp;
        const double a = (q & 2) ? ap : am, b = (q & 1) ? bp : bm;
        const double c = (q & 2) ? cp : cm, d = (q & 1) ? dp : dm;
        const double inv = invs[q];
        const double ai = a * inv, bi = b * inv, ci = c * inv, di = d * inv;      // J^-1 = [[di, -bi], [-ci, ai]]
        const double g0x = c1[2] + eta * c3[2], g0y = c1[3] + eta * c3[3];
        const double g1x = c2[2] + xi * c3[2], g1y = c2[3] + xi * c3[3];
        const double h00 = g0x * di - g1x * ci, h01 = g1x * ai - g0x * bi;
        const double h10 = g0y * di - g1y * ci, h11 = g1y * ai - g0y * bi;
        const double tr = h00 + h11;
        const double j = tr + (h00 * h11 - h01 * h10);
        if (jq) jq[q] = j;
        jm = fmin(jm, j);
        const bool ok = j > -1.0;
        all_ok = all_ok && ok;
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
        const double A = 0.0625 * fabs(dets[q]);
        double w = psi;                                                            // psi - beta
        if (HASB) {
            const double bx = k.b[q].x, by = k.b[q].y;
            const double uhx = 0.25 * ((c0x + xi * c1[2]) + eta * (c2[2] + xi * c3[2]));
            const double uhy = 0.25 * ((c0y + xi * c1[3]) + eta * (c2[3] + xi * c3[3]));
            w -= bx * uhx + by * uhy;
            const double fx = -0.25 * A * bx, fy = -0.25 * A * by;                 // de/d(4 u_h)
            D0x += fx; D0y += fy;
            D1[2] += xi * fx; D1[3] += xi * fy;
            D2[2] += eta * fx; D2[3] += eta * fy;
            S3[2] += ((q & 1) == ((q & 2) >> 1) ? gp : -gp) * fx;                   // xi eta / gp
            S3[3] += ((q & 1) == ((q & 2) >> 1) ? gp : -gp) * fy;
        }
        e += A * w;
        // de/dG = A P J^-T, J^-T = [[di, -ci], [-bi, ai]]
        const double dg0x = A * (p00 * di - p01 * bi), dg0y = A * (p10 * di - p11 * bi);
        const double dg1x = A * (p01 * ai - p00 * ci), dg1y = A * (p11 * ai - p10 * ci);
        // Q = A ((psi - beta) I - H^T P), de/dJ = Q J^-T
        const double diag = A * w;
        const double q00 = diag - A * (h00 * p00 + h10 * p10), q01 = -A * (h00 * p01 + h10 * p11);
        const double q10 = -A * (h01 * p00 + h11 * p10), q11 = diag - A * (h01 * p01 + h11 * p11);
        const double da = q00 * di - q01 * bi, db = q01 * ai - q00 * ci;          // d/d(a, b): row 0 of J (x components)
        const double dc = q10 * di - q11 * bi, dd = q11 * ai - q10 * ci;          // d/d(c, d): row 1 (y components)
        const double u[4] = {da, dc, dg0x, dg0y}, v[4] = {db, dd, dg1x, dg1y};    // de/d(4 d./dxi), de/d(4 d./deta)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            D1[i] += u[i];
            D2[i] += v[i];
            S3[i] += ((q & 2) ? u[i] : -u[i]) + ((q & 1) ? v[i] : -v[i]);
        }
    }
    jmin = jm;
    inverted = !all_ok;
    double g[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double d1 = all_ok ? D1[i] : 0.0, d2 = all_ok ? D2[i] : 0.0, d3 = all_ok ? gp * S3[i] : 0.0;
        const double p = d1 + d2, m = d1 - d2;
        g[0][i] = d3 - p;
        g[1][i] = m - d3;
        g[2][i] = p + d3;
        g[3][i] = -m - d3;
    }
    const double d0x = all_ok ? D0x : 0.0, d0y = all_ok ? D0y : 0.0;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        gx[n] = make_double2(g[n][0], g[n][1]);
        gu[n] = HASB ? make_double2(g[n][2] + d0x, g[n][3] + d0y) : make_double2(g[n][2], g[n][3]);
    }
    return all_ok ? e : (double)INFINITY;
}

// The tangent of one cell at a linearisation point.  Per point, hyper_tangent_apply's forms on the state of
// quad4_neo_hookean_element, with T = F^-T, c = mu - lambda L and a direction p on the four corners (dG from p exactly as G
// from U):
//   dH = dG J^-1,  dP = mu dH + c T dH^T T + lambda (T : dH) T,  dq/d(dG) = A dP J^-T
// Dead loads do not enter.  A state is used once, so it is fused with its application point by point: across the points
// only the cotangents of c1, c2, c3 of the two components of p stay live (6 doubles), spread to the corners with +-1 at the
// end.  The inversion rule is the energy's at cell level (a point with j <= -1 or NaN is evaluated at j = 0; a cell with
// such a point has all its outputs 0, by selects on ordinary arithmetic); jmin carries the true min_q j_q.

// The state of one Gauss point both tangent forms share: J^-1 = [[di, -bi], [-ci, ai]], T, c, A (unscaled coefficients).
struct Quad4HyperPoint {
    double ai, bi, ci, di;
    double t00, t01, t10, t11;
    double c, A, j;
    bool ok;
};

// c_stored: NULL, or the point's c = mu - lambda L as an earlier evaluation of the SAME state returned it (the diag launch
// stores it per slot and point, the apply launches of that linearisation read it instead of calling log1p again).
__device__ __forceinline__ Quad4HyperPoint quad4_hyper_point(double a, double b, double c, double d, double det, double inv,
                                                             double g0x, double g0y, double g1x, double g1y, double lambda,
                                                             double mu, const double *c_stored = nullptr) {
    Quad4HyperPoint s;
    s.ai = a * inv; s.bi = b * inv; s.ci = c * inv; s.di = d * inv;
    const double h00 = g0x * s.di - g1x * s.ci, h01 = g1x * s.ai - g0x * s.bi;
    const double h10 = g0y * s.di - g1y * s.ci, h11 = g1y * s.ai - g0y * s.bi;
    s.j = (h00 + h11) + (h00 * h11 - h01 * h10);
    s.ok = s.j > -1.0;
    const double js = s.ok ? s.j : 0.0;
    const double r = hyper_rcp(1.0 + js);
    s.t00 = (1.0 + h11) * r; s.t01 = -h10 * r; s.t10 = -h01 * r; s.t11 = (1.0 + h00) * r;
    s.c = c_stored ? *c_stored : mu - lambda * log1p(js);
    s.A = 0.0625 * fabs(det);
    return s;
}

// q_k = sum_l K_e[k][l] p_l for the four corners; returns p^T K_e p = sum_k p_k . q_k.  jq (host checks only, NULL on the
// device) receives the four j_q; cq (may be NULL): the four c_q quad4_hyper_tangent_blocks returned for this cell and state.
__device__ __forceinline__ double quad4_hyper_tangent_apply(const double2 (&Xn)[4], const double2 (&Un)[4], const double2 (&Pn)[4],
                                                            const Quad4HyperConsts &k, double2 (&qn)[4], double &jmin,
                                                            bool &inverted, double *jq = nullptr, const double *cq = nullptr) {
    const double gp = 0.57735026918962576451;   // 1/sqrt(3)
    double c1[6], c2[6], c3[6];                  // components: x, y, ux, uy, px, py
    {
        const double v[6][4] = {{Xn[0].x, Xn[1].x, Xn[2].x, Xn[3].x}, {Xn[0].y, Xn[1].y, Xn[2].y, Xn[3].y},
                                {Un[0].x, Un[1].x, Un[2].x, Un[3].x}, {Un[0].y, Un[1].y, Un[2].y, Un[3].y},
                                {Pn[0].x, Pn[1].x, Pn[2].x, Pn[3].x}, {Pn[0].y, Pn[1].y, Pn[2].y, Pn[3].y}};
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const double s = v[i][1] - v[i][0], t = v[i][2] - v[i][3];
            c1[i] = s + t;
            c3[i] = t - s;
            c2[i] = (v[i][3] - v[i][0]) + (v[i][2] - v[i][1]);
        }
    }
    const double am = c1[0] - gp * c3[0], ap = c1[0] + gp * c3[0], cm = c1[1] - gp * c3[1], cp = c1[1] + gp * c3[1];
    const double bm = c2[0] - gp * c3[0], bp = c2[0] + gp * c3[0], dm = c2[1] - gp * c3[1], dp = c2[1] + gp * c3[1];
    const double dets[4] = {am * dm - bm * cm, am * dp - bp * cm, ap * dm - bm * cp, ap * dp - bp * cp};
    double invs[4];
    hyper_rcp4(dets, invs);
    double D1x = 0.0, D1y = 0.0, D2x = 0.0, D2y = 0.0, S3x = 0.0, S3y = 0.0;   // cotangents of c1, c2, c3 / gp (px, py)
    double jm = (double)INFINITY;
    bool all_ok = true;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double xi = (q & 1) ? gp : -gp, eta = (q & 2) ? gp : -gp;
        const Quad4HyperPoint s = quad4_hyper_point((q & 2) ? ap : am, (q & 1) ? bp : bm, (q & 2) ? cp : cm, (q & 1) ? dp : dm,
                                                    dets[q], invs[q], c1[2] + eta * c3[2], c1[3] + eta * c3[3],
                                                    c2[2] + xi * c3[2], c2[3] + xi * c3[3], k.lambda, k.mu,
                                                    cq ? cq + q : nullptr);
        if (jq) jq[q] = s.j;
        jm = fmin(jm, s.j);
        all_ok = all_ok && s.ok;
        const double g0x = c1[4] + eta * c3[4], g0y = c1[5] + eta * c3[5];
        const double g1x = c2[4] + xi * c3[4], g1y = c2[5] + xi * c3[5];
        const double d00 = g0x * s.di - g1x * s.ci, d01 = g1x * s.ai - g0x * s.bi;         // dH
        const double d10 = g0y * s.di - g1y * s.ci, d11 = g1y * s.ai - g0y * s.bi;
        // M = T dH^T, then M T
        const double m00 = s.t00 * d00 + s.t01 * d01, m01 = s.t00 * d10 + s.t01 * d11;
        const double m10 = s.t10 * d00 + s.t11 * d01, m11 = s.t10 * d10 + s.t11 * d11;
        const double lt = k.lambda * (s.t00 * d00 + s.t01 * d01 + s.t10 * d10 + s.t11 * d11);
        const double s00 = k.mu * d00 + s.c * (m00 * s.t00 + m01 * s.t10) + lt * s.t00;
        const double s01 = k.mu * d01 + s.c * (m00 * s.t01 + m01 * s.t11) + lt * s.t01;
        const double s10 = k.mu * d10 + s.c * (m10 * s.t00 + m11 * s.t10) + lt * s.t10;
        const double s11 = k.mu * d11 + s.c * (m10 * s.t01 + m11 * s.t11) + lt * s.t11;
        // dq/d(dG) = A dP J^-T, J^-T = [[di, -ci], [-bi, ai]]
        const double u0 = s.A * (s00 * s.di - s01 * s.bi), u1 = s.A * (s10 * s.di - s11 * s.bi);     // d/d(4 dp/dxi)
        const double v0 = s.A * (s01 * s.ai - s00 * s.ci), v1 = s.A * (s11 * s.ai - s10 * s.ci);     // d/d(4 dp/deta)
        D1x += u0; D1y += u1;
        D2x += v0; D2y += v1;
        S3x += ((q & 2) ? u0 : -u0) + ((q & 1) ? v0 : -v0);
        S3y += ((q & 2) ? u1 : -u1) + ((q & 1) ? v1 : -v1);
    }
    jmin = jm;
    inverted = !all_ok;
    double pq = 0.0;
    {
        const double d1[2] = {all_ok ? D1x : 0.0, all_ok ? D1y : 0.0}, d2[2] = {all_ok ? D2x : 0.0, all_ok ? D2y : 0.0};
        const double d3[2] = {all_ok ? gp * S3x : 0.0, all_ok ? gp * S3y : 0.0};
        double g[4][2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const double p = d1[i] + d2[i], m = d1[i] - d2[i];
            g[0][i] = d3[i] - p;
            g[1][i] = m - d3[i];
            g[2][i] = p + d3[i];
            g[3][i] = -m - d3[i];
        }
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            qn[n] = make_double2(g[n][0], g[n][1]);
            pq += Pn[n].x * g[n][0] + Pn[n].y * g[n][1];
        }
    }
    return pq;
}

// The four corner blocks {K_xx, K_xy, K_yy} of the same tangent in closed form: with n = 4 grad_xi N_a(xi_q) (entries
// +-(1 +- 1/sqrt(3))), w = J^-T n on the unscaled coefficients and t = T w,
//   K_aa = sum_q A [mu |w|^2 I + (c + lambda) t (x) t]
// (dH = e_i (x) w gives dP w = mu |w|^2 e_i + (c + lambda) t_i t).  Same inversion rule: twelve zeros for an inverted cell.
// cq_out (may be NULL) receives the four c_q = mu - lambda L_q, what quad4_hyper_tangent_apply takes as cq.
__device__ __forceinline__ void quad4_hyper_tangent_blocks(const double2 (&Xn)[4], const double2 (&Un)[4], const Quad4HyperConsts &k,
                                                           double (&blk)[4][3], double &jmin, bool &inverted,
                                                           double *cq_out = nullptr) {
    const double gp = 0.57735026918962576451;
    double c1[4], c2[4], c3[4];                  // components: x, y, ux, uy
    {
        const double v[4][4] = {{Xn[0].x, Xn[1].x, Xn[2].x, Xn[3].x}, {Xn[0].y, Xn[1].y, Xn[2].y, Xn[3].y},
                                {Un[0].x, Un[1].x, Un[2].x, Un[3].x}, {Un[0].y, Un[1].y, Un[2].y, Un[3].y}};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double s = v[i][1] - v[i][0], t = v[i][2] - v[i][3];
            c1[i] = s + t;
            c3[i] = t - s;
            c2[i] = (v[i][3] - v[i][0]) + (v[i][2] - v[i][1]);
        }
    }
    const double am = c1[0] - gp * c3[0], ap = c1[0] + gp * c3[0], cm = c1[1] - gp * c3[1], cp = c1[1] + gp * c3[1];
    const double bm = c2[0] - gp * c3[0], bp = c2[0] + gp * c3[0], dm = c2[1] - gp * c3[1], dp = c2[1] + gp * c3[1];
    const double dets[4] = {am * dm - bm * cm, am * dp - bp * cm, ap * dm - bm * cp, ap * dp - bp * cp};
    double invs[4];
    hyper_rcp4(dets, invs);
#pragma unroll
    for (int a = 0; a < 4; ++a) { blk[a][0] = 0.0; blk[a][1] = 0.0; blk[a][2] = 0.0; }
    double jm = (double)INFINITY;
    bool all_ok = true;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double xi = (q & 1) ? gp : -gp, eta = (q & 2) ? gp : -gp;
        const Quad4HyperPoint s = quad4_hyper_point((q & 2) ? ap : am, (q & 1) ? bp : bm, (q & 2) ? cp : cm, (q & 1) ? dp : dm,
                                                    dets[q], invs[q], c1[2] + eta * c3[2], c1[3] + eta * c3[3],
                                                    c2[2] + xi * c3[2], c2[3] + xi * c3[3], k.lambda, k.mu);
        jm = fmin(jm, s.j);
        all_ok = all_ok && s.ok;
        if (cq_out) cq_out[q] = s.c;
        const double Am = s.A * k.mu, Ac = s.A * (s.c + k.lambda);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const double xa = (a == 1 || a == 2) ? 1.0 : -1.0, ya = (a >= 2) ? 1.0 : -1.0;      // the corner's (xi_a, eta_a)
            const double n0 = xa * (1.0 + ya * eta), n1 = ya * (1.0 + xa * xi);
            const double w0 = s.di * n0 - s.ci * n1, w1 = s.ai * n1 - s.bi * n0;
            const double t0 = s.t00 * w0 + s.t01 * w1, t1 = s.t10 * w0 + s.t11 * w1;
            const double iso = Am * (w0 * w0 + w1 * w1);
            blk[a][0] += iso + Ac * t0 * t0;
            blk[a][1] += Ac * t0 * t1;
            blk[a][2] += iso + Ac * t1 * t1;
        }
    }
    jmin = jm;
    inverted = !all_ok;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        blk[a][0] = all_ok ? blk[a][0] : 0.0;
        blk[a][1] = all_ok ? blk[a][1] : 0.0;
        blk[a][2] = all_ok ? blk[a][2] : 0.0;
    }
}

}  // namespace hfem
