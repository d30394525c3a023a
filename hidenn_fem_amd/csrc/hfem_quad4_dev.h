// QUAD4 element closed forms shared by the energy kernels (quad4.hip) and the frozen-mesh solve (quad4_cg.hip;
// hfem_cg_dev.h for the unit-displacement columns of the diag and AMG assembly kernels).
#pragma once
#include <hip/hip_runtime.h>

#include "hfem_device.h"

namespace hfem {

struct JacGrad {          // dL/d(a,b,c,d), dL/dG0, dL/dG1
    double da, db, dc, dd;
    double2 dg0, dg1;
};

// energy density * |det| at one point with weight w, and its gradient w.r.t. (a..d, G0, G1)
// beta_w (body-force instances): w * b(xi_q).u_h(xi_q) of this point -- the density is w psi - beta_w; with the
// cotangents below it adds only the sign(det) (-beta_w) cof(J) term (u_h's own gradient is added by the caller).
// Cofactor form (round 3): with adj = [[d, -b], [-c, a]] the UNSCALED h^ = G adj^T = det H, eps^ = (h^00, h^11, h^01 + h^10),
// sigma^ = C eps^ and  w |det| psi = t2/2 (eps^ . sigma^)  with  t2 = w / |det| = copysign(w, det) / det.  Nothing is
// pre-scaled by 1/det (no a/det .. d/det), dE/dh^ = t2 sigma^, and the only trace of the 1/|det| factor in the backward
// is  dE/d det = -E / det.  51 fp64 operations per point with gradients (57 in the scaled form); `inv` = 1 / det comes
// from the caller, which inverts the four determinants of an element with ONE reciprocal.
template <bool GRAD>
__device__ __forceinline__ double jac_point(double a, double b, double c, double d, double2 g0, double2 g1, double det, double inv,
                                            double w, const Tri3Consts &k, JacGrad &o, double beta_w = 0.0, double *A_out = nullptr) {
    const double t2 = __builtin_copysign(w, det) * inv;                    // w / |det|  (sign through one v_bfi)
    const double h00 = g0.x * d - g1.x * b, h01 = g1.x * a - g0.x * c;
    const double h10 = g0.y * d - g1.y * b, h11 = g1.y * a - g0.y * c;
    const double gam = h01 + h10;
    const double sxx = k.c11 * h00 + k.c12 * h11, syy = k.c12 * h00 + k.c22 * h11, sxy = k.c33 * gam;
    const double hs = h00 * sxx + h11 * syy + gam * sxy;
    double e = (0.5 * t2) * hs;                                            // w |det| psi
    if (A_out) *A_out = fabs(det);
    if (GRAD) {
        const double p00 = t2 * sxx, p01 = t2 * sxy, p11 = t2 * syy;       // dE / d h^  (symmetric)
        o.dg0 = make_double2(p00 * d - p01 * c, p01 * d - p11 * c);
        o.dg1 = make_double2(p01 * a - p00 * b, p11 * a - p01 * b);
        double ddet = -e * inv;                                            // through t2 = w sign(det) / det
        if (A_out) ddet -= __builtin_copysign(1.0, det) * beta_w;          // body-force instances only: -sign(det) beta_w
        o.da = (p01 * g1.x + p11 * g1.y) + ddet * d;
        o.db = -(p00 * g1.x + p01 * g1.y) - ddet * c;
        o.dc = -(p01 * g0.x + p11 * g0.y) - ddet * b;
        o.dd = (p00 * g0.x + p01 * g0.y) + ddet * a;
    }
    if (A_out) e -= fabs(det) * beta_w;
    return e;
}

// the four determinants of an element inverted with ONE v_rcp_f64 (quarter-rate) + Newton: 1/d_i from 1/(d0 d1 d2 d3).
// A vanishing determinant makes all four results Inf / NaN -- the element's energy is NaN either way.
__device__ __forceinline__ void rcp4(const double (&dt)[4], double (&iv)[4]) {
    const double p01 = dt[0] * dt[1], p23 = dt[2] * dt[3];
    const double r = fast_rcp(p01 * p23);
    const double r01 = r * p23, r23 = r * p01;                             // 1/(d0 d1), 1/(d2 d3)
    iv[0] = r01 * dt[1]; iv[1] = r01 * dt[0]; iv[2] = r23 * dt[3]; iv[3] = r23 * dt[2];
}

// reference-square corner signs, CCW from (-1,-1): xi_k = {-1,1,1,-1}, eta_k = {-1,-1,1,1}
__device__ __forceinline__ constexpr double corner_xi(int k) { return (k == 1 || k == 2) ? 1.0 : -1.0; }
__device__ __forceinline__ constexpr double corner_eta(int k) { return k >= 2 ? 1.0 : -1.0; }

__device__ __forceinline__ void shape_derivs(double xi, double eta, double (&D0)[4], double (&D1)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        D0[k] = 0.25 * corner_xi(k) * (1.0 + corner_eta(k) * eta);
        D1[k] = 0.25 * corner_eta(k) * (1.0 + corner_xi(k) * xi);
    }
}

// Whole-element energy (2x2 Gauss, weights 1) and its gradient w.r.t. the four nodes, in the bilinear
// coefficient form.  For a nodal field v_0..v_3:  4 dv/dxi = a1 + eta a3,  4 dv/deta = a2 + xi a3  with
//   a1 = (v1-v0)+(v2-v3),  a2 = (v3-v0)+(v2-v1),  a3 = (v2-v3)-(v1-v0).
// H = G J^-T does not see the common factor 4 and |det| sees 16, so the points are evaluated on the unscaled
// coefficients with weight 1/16; cotangents are accumulated per coefficient (the a3 part as +-da +-db, scaled by
// 1/sqrt(3) once) and spread to the nodes with +-1 at the end.  ~370 fp64 instructions per element with
// gradients (the node-by-node D_N form above costs ~490).
// HASB: body force b(xi_q) at the four Gauss points (k.Bk... is the TRI3 table; QUAD4 takes Bq[q] = b at point q):
// e -= sum_q |det_q| u_h(q).b_q, dU_k -= sum_q |det_q| N_k(q) b_q, and the |det_q| dependence through jac_point.
// PHYS: the opt-in physical gradient convention, grad_u = G Jinv instead of the reference's G Jinv^T.  As for
// TRI3 (hfem_device.h), E_phys(a, b, c, d) = E_ref(a, c, b, d): b and c swap on the way into jac_point and their cotangents
// swap on the way out.
template <bool GRAD, bool HASB = false, bool PHYS = false>
__device__ __forceinline__ double quad4_element(const double2 (&Xn)[4], const double2 (&Un)[4], const Tri3Consts &k,
                                                double2 (&gx)[4], double2 (&gu)[4], const double2 *Bq = nullptr) {
    const double gp = 0.57735026918962576451;   // 1/sqrt(3)
    double a1[4], a2[4], a3[4];                  // components: x, y, ux, uy
    {
        const double v[4][4] = {{Xn[0].x, Xn[1].x, Xn[2].x, Xn[3].x}, {Xn[0].y, Xn[1].y, Xn[2].y, Xn[3].y},
                                {Un[0].x, Un[1].x, Un[2].x, Un[3].x}, {Un[0].y, Un[1].y, Un[2].y, Un[3].y}};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double s = v[i][1] - v[i][0], t = v[i][2] - v[i][3];
            a1[i] = s + t;
            a3[i] = t - s;
            a2[i] = (v[i][3] - v[i][0]) + (v[i][2] - v[i][1]);
        }
    }
    // Points in the order (-,-) (+,-) (-,+) (+,+).  With u_q = dE/d(4 dv/dxi) and v_q = dE/d(4 dv/deta) at point q:
    //   d a1 = sum u_q, d a2 = sum v_q, d a3 = gp ((u2+u3) - (u0+u1) + (v1+v3) - (v0+v2)); the pair sums are shared.
    double U[4][4], V[4][4];
    double2 gub[4] = {make_double2(0.0, 0.0), make_double2(0.0, 0.0), make_double2(0.0, 0.0), make_double2(0.0, 0.0)};
    double e = 0.0;
    // J(xi, eta) is affine: a, c depend on eta only, b, d on xi only -- two values each; the four determinants first, one
    // reciprocal for all of them
    const double am = a1[0] - gp * a3[0], ap = a1[0] + gp * a3[0], cm = a1[1] - gp * a3[1], cp = a1[1] + gp * a3[1];
    const double bm = a2[0] - gp * a3[0], bp = a2[0] + gp * a3[0], dm = a2[1] - gp * a3[1], dp = a2[1] + gp * a3[1];
    const double dets[4] = {am * dm - bm * cm, am * dp - bp * cm, ap * dm - bm * cp, ap * dp - bp * cp};
    double invs[4];
    rcp4(dets, invs);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double xi = (q & 1) ? gp : -gp, eta = (q & 2) ? gp : -gp;
        const double a = (q & 2) ? ap : am, b = (q & 1) ? bp : bm;
        const double c = (q & 2) ? cp : cm, d = (q & 1) ? dp : dm;
        const double2 g0 = make_double2(a1[2] + eta * a3[2], a1[3] + eta * a3[3]);
        const double2 g1 = make_double2(a2[2] + xi * a3[2], a2[3] + xi * a3[3]);
        JacGrad o;
        if (HASB) {
            // N_k(q) = (1 + xi_k xi)(1 + eta_k eta) / 4; the unscaled coefficients carry |det| x 16: weight 1/16
            double nk[4], uhx = 0.0, uhy = 0.0, A16;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                nk[j] = 0.25 * (1.0 + corner_xi(j) * xi) * (1.0 + corner_eta(j) * eta);
                uhx += nk[j] * Un[j].x;
                uhy += nk[j] * Un[j].y;
            }
            const double2 bq = Bq[q];
            e += jac_point<GRAD>(a, PHYS ? c : b, PHYS ? b : c, d, g0, g1, dets[q], invs[q], 0.0625, k, o, 0.0625 * (uhx * bq.x + uhy * bq.y), &A16);
            if (GRAD) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    gub[j].x -= (0.0625 * A16) * nk[j] * bq.x;
                    gub[j].y -= (0.0625 * A16) * nk[j] * bq.y;
                }
            }
        } else {
            e += jac_point<GRAD>(a, PHYS ? c : b, PHYS ? b : c, d, g0, g1, dets[q], invs[q], 0.0625, k, o);
        }
        if (GRAD) {
            U[q][0] = o.da; U[q][1] = PHYS ? o.db : o.dc; U[q][2] = o.dg0.x; U[q][3] = o.dg0.y;
            V[q][0] = PHYS ? o.dc : o.db; V[q][1] = o.dd; V[q][2] = o.dg1.x; V[q][3] = o.dg1.y;
        }
    }
    if (GRAD) {
        double g[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double u01 = U[0][i] + U[1][i], u23 = U[2][i] + U[3][i];
            const double v02 = V[0][i] + V[2][i], v13 = V[1][i] + V[3][i];
            const double d1 = u01 + u23, d2 = v02 + v13;
            const double d3 = gp * ((u23 - u01) + (v13 - v02)), p = d1 + d2, m = d1 - d2;
            g[0][i] = d3 - p;
            g[1][i] = m - d3;
            g[2][i] = p + d3;
            g[3][i] = -m - d3;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            gx[j] = make_double2(g[j][0], g[j][1]);
            gu[j] = HASB ? make_double2(g[j][2] + gub[j].x, g[j][3] + gub[j].y) : make_double2(g[j][2], g[j][3]);
        }
    }
    return e;
}

// The displacement half alone, for frozen coordinates (quad4_cg.hip: K p is dE/du at u = p with no forces): the same points
// and the same operations on (a, b, c, d, G0, G1) as quad4_element, without dE/d(a..d), the determinant cotangent or the
// coordinate columns of the spread -- 2 of the 4 columns, ~190 fp64 instructions per element.  Returns the element's strain
// energy (1/2 u_e^T K_e u_e); gu = K_e u_e.
template <bool PHYS>
__device__ __forceinline__ double quad4_element_u(const double2 (&Xn)[4], const double2 (&Un)[4], const Tri3Consts &k,
                                                  double2 (&gu)[4]) {
    const double gp = 0.57735026918962576451;   // 1/sqrt(3)
    double a1[4], a2[4], a3[4];                  // components: x, y, ux, uy
    {
        const double v[4][4] = {{Xn[0].x, Xn[1].x, Xn[2].x, Xn[3].x}, {Xn[0].y, Xn[1].y, Xn[2].y, Xn[3].y},
                                {Un[0].x, Un[1].x, Un[2].x, Un[3].x}, {Un[0].y, Un[1].y, Un[2].y, Un[3].y}};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double s = v[i][1] - v[i][0], t = v[i][2] - v[i][3];
            a1[i] = s + t;
            a3[i] = t - s;
            a2[i] = (v[i][3] - v[i][0]) + (v[i][2] - v[i][1]);
        }
    }
    const double am = a1[0] - gp * a3[0], ap = a1[0] + gp * a3[0], cm = a1[1] - gp * a3[1], cp = a1[1] + gp * a3[1];
    const double bm = a2[0] - gp * a3[0], bp = a2[0] + gp * a3[0], dm = a2[1] - gp * a3[1], dp = a2[1] + gp * a3[1];
    const double dets[4] = {am * dm - bm * cm, am * dp - bp * cm, ap * dm - bm * cp, ap * dp - bp * cp};
    double invs[4];
    rcp4(dets, invs);
    double U[4][2], V[4][2];                     // dE/d(4 du/dxi), dE/d(4 du/deta) at the four points
    double e = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double xi = (q & 1) ? gp : -gp, eta = (q & 2) ? gp : -gp;
        const double a = (q & 2) ? ap : am, b0 = (q & 1) ? bp : bm;
        const double c0 = (q & 2) ? cp : cm, d = (q & 1) ? dp : dm;
        const double b = PHYS ? c0 : b0, c = PHYS ? b0 : c0;               // E_phys(a, b, c, d) = E_ref(a, c, b, d)
        const double2 g0 = make_double2(a1[2] + eta * a3[2], a1[3] + eta * a3[3]);
        const double2 g1 = make_double2(a2[2] + xi * a3[2], a2[3] + xi * a3[3]);
        const double t2 = __builtin_copysign(0.0625, dets[q]) * invs[q];   // w / |det|, w = 1/16 on the unscaled coefficients
        const double h00 = g0.x * d - g1.x * b, h01 = g1.x * a - g0.x * c;
        const double h10 = g0.y * d - g1.y * b, h11 = g1.y * a - g0.y * c;
        const double gam = h01 + h10;
        const double sxx = k.c11 * h00 + k.c12 * h11, syy = k.c12 * h00 + k.c22 * h11, sxy = k.c33 * gam;
        e += (0.5 * t2) * (h00 * sxx + h11 * syy + gam * sxy);
        const double p00 = t2 * sxx, p01 = t2 * sxy, p11 = t2 * syy;
        U[q][0] = p00 * d - p01 * c; U[q][1] = p01 * d - p11 * c;
        V[q][0] = p01 * a - p00 * b; V[q][1] = p11 * a - p01 * b;
    }
    double g[4][2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const double u01 = U[0][i] + U[1][i], u23 = U[2][i] + U[3][i];
        const double v02 = V[0][i] + V[2][i], v13 = V[1][i] + V[3][i];
        const double d1 = u01 + u23, d2 = v02 + v13;
        const double d3 = gp * ((u23 - u01) + (v13 - v02)), p = d1 + d2, m = d1 - d2;
        g[0][i] = d3 - p;
        g[1][i] = m - d3;
        g[2][i] = p + d3;
        g[3][i] = -m - d3;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) gu[j] = make_double2(g[j][0], g[j][1]);
    return e;
}

}  // namespace hfem
