// Per-element closed forms of the mesh-validity kernels (mesh_guard.hip through hfem_mesh_dev.h): one
// description per element kind, Tri3 and Quad4, each giving the orientation sign, the measure, the reference crossing of the
// step bound, the two crossings of the det F-safe bound, det F, and the quality barrier with its per-node gradient.  Plain
// inline functions of corner rows, no wave intrinsics and no memory access: tests/host/hyper_mesh_san_main.cpp compiles this
// text against tests/host/hip_stub.  The build contracts multiply-adds inside an expression (-ffp-contract=on), so the
// grouping of every expression here is part of what the deterministic entry points return.
//
// Small strain.  s = the sign of the signed area on the reference rows R (the model's initial coordinates), so a
// clockwise-numbered mesh measures like its counter-clockwise copy.
//   TRI3   detJ = (x0-x2)(y1-y2) - (x1-x2)(y0-y2) (= 2 x the signed area), q = 2 sqrt(3) s detJ / sum |e|^2 (1 for an
//          equilateral triangle), ratio = detJ / detJ_ref, inverted: s detJ <= 0.
//   QUAD4  (local nodes counter-clockwise, indices mod 4) e_k = X_{k+1} - X_k, the corner cross product c_k = e_{k-1} x e_k
//          (detJ at corner k = c_k / 4; detJ of a bilinear cell is affine over the reference square, so the cell is valid
//          everywhere iff all four s c_k > 0), s = sign of c_0 + c_2 on R, q_k = 2 s c_k / (|e_{k-1}|^2 + |e_k|^2) (1 at a
//          right-angled corner with equal sides), q = min_k q_k, ratio = min_k c_k / c_k_ref, inverted: some s c_k <= 0.
//   bound  detJ(x + a d) (QUAD4: c_k(x + a d)) = A0 + A1 a + A2 a^2 exactly; the first a > 0 at which it keeps only eta of
//          its value is first_crossing (hfem_crossing_dev.h).  coefficients() is the only place A0, A1, A2 are formed.
//   barrier  Q = (w / (kBarrierTerms Ne)) sum (1/q - 1) over the elements (QUAD4: and their corners); finite for valid
//          elements only (the solver keeps every element valid).
// Finite strain.  A coordinate step x -> x + a d at FIXED nodal u moves the reference element, R(a) = detJ(X + a d) = A0 +
// A1 a + A2 a^2, and the deformed one, D(a) = detJ(X + u + a d) = B0 + B1 a + B2 a^2 (the same d: B2 = A2), so det F(a) =
// D(a) / R(a).
//   reference crossing   the first a > 0 with R(a) = eta R(0)                                        (the small-strain bound)
//   det F crossing       the first a > 0 with D(a) R(0) - eta D(0) R(a) = 0, i.e. det F(a) = eta det F(0): the exact quadratic
//                        (1 - eta) A0 B0 + (B1 A0 - eta B0 A1) a + (B2 A0 - eta B0 A2) a^2, which first_crossing solves as it
//                        stands with A0 B0 in the place of A0 (below the reference crossing R keeps its sign, so the division
//                        by R(a) R(0) changes nothing)
// The element's bound is the smaller of the two; an element whose state is invalid already (A0 B0 <= 0, or NaN) has bound 0.
// QUAD4: the same two crossings per corner, on c_k (reference cell) and c_k^def (deformed cell); the cell's bound is the
// minimum over its corners and its J the smallest corner ratio r_k = c_k^def / c_k.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "hfem_crossing_dev.h"

namespace hfem {
namespace {

__device__ __forceinline__ double2 add2(const double2 p, const double2 r) { return make_double2(p.x + r.x, p.y + r.y); }
__device__ __forceinline__ double2 sub2(const double2 p, const double2 r) { return make_double2(p.x - r.x, p.y - r.y); }
__device__ __forceinline__ double cross2(const double2 p, const double2 r) { return p.x * r.y - p.y * r.x; }
__device__ __forceinline__ double norm_sq(const double2 p) { return p.x * p.x + p.y * p.y; }
__device__ __forceinline__ double sign_of(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0); }

// The first a > 0 at which det F(a) = eta det F(0), from the coefficients of R and D (0: the state is invalid already).
__device__ __forceinline__ double det_f_crossing(double A0, double A1, double A2, double B0, double B1, double B2, double eta) {
    const double p0 = A0 * B0;
    if (!(p0 > 0.0)) return 0.0;                             // det F(0) <= 0, a flat reference element, or NaN
    return first_crossing(p0, B1 * A0 - eta * B0 * A1, B2 * A0 - eta * B0 * A2, eta);
}

// The smaller crossing; a NaN reference crossing (non-finite rows) loses the comparison, the det F crossing is 0 then.
__device__ __forceinline__ double smaller_crossing(double a_ref, double a_def) { return a_ref < a_def ? a_ref : a_def; }

// ---------------------------------------------------------------- TRI3
struct Tri3 {
    static constexpr int kNodes = 3;
    static constexpr double kBarrierTerms = 1.0;
    static constexpr double kTwoSqrt3 = 3.4641016151377545870548926830117;   // 2 sqrt(3)

    static __device__ __forceinline__ double det(const double2 X0, const double2 X1, const double2 X2) {
        return (X0.x - X2.x) * (X1.y - X2.y) - (X1.x - X2.x) * (X0.y - X2.y);
    }

    static __device__ __forceinline__ double edge_sq_sum(const double2 X0, const double2 X1, const double2 X2) {
        const double ax = X1.x - X0.x, ay = X1.y - X0.y, bx = X2.x - X1.x, by = X2.y - X1.y, cx = X0.x - X2.x, cy = X0.y - X2.y;
        return ax * ax + ay * ay + bx * bx + by * by + cx * cx + cy * cy;
    }

    static __device__ __forceinline__ double orientation(const double2 (&R)[3]) { return sign_of(det(R[0], R[1], R[2])); }

    // q and detJ / detJ_ref of the element -> inverted
    static __device__ __forceinline__ bool measure(const double2 (&X)[3], const double2 (&R)[3], double &q, double &ratio) {
        const double det_ref = det(R[0], R[1], R[2]);
        const double d = det(X[0], X[1], X[2]);
        const double s = sign_of(det_ref);
        q = kTwoSqrt3 * s * d / edge_sq_sum(X[0], X[1], X[2]);
        ratio = d / det_ref;
        return !(s * d > 0.0);
    }

    // detJ(x + a d) with J columns (x0 - x2, x1 - x2) and their directions
    static __device__ __forceinline__ void coefficients(const double2 X0, const double2 X1, const double2 X2, const double2 D0,
                                                        const double2 D1, const double2 D2, double &A0, double &A1, double &A2) {
        const double ax = X0.x - X2.x, ay = X0.y - X2.y, bx = X1.x - X2.x, by = X1.y - X2.y;
        const double dax = D0.x - D2.x, day = D0.y - D2.y, dbx = D1.x - D2.x, dby = D1.y - D2.y;
        A0 = ax * by - bx * ay;
        A1 = (ax * dby + dax * by) - (bx * day + dbx * ay);
        A2 = dax * dby - dbx * day;
    }

    static __device__ __forceinline__ double reference_crossing(const double2 (&X)[3], const double2 (&D)[3], double eta) {
        double A0, A1, A2;
        coefficients(X[0], X[1], X[2], D[0], D[1], D[2], A0, A1, A2);
        return first_crossing(A0, A1, A2, eta);
    }

    static __device__ __forceinline__ void hyper_crossings(const double2 (&X)[3], const double2 (&U)[3], const double2 (&D)[3],
                                                           double eta, double &a_ref, double &a_def) {
        double A0, A1, A2, B0, B1, B2;
        coefficients(X[0], X[1], X[2], D[0], D[1], D[2], A0, A1, A2);
        coefficients(add2(X[0], U[0]), add2(X[1], U[1]), add2(X[2], U[2]), D[0], D[1], D[2], B0, B1, B2);
        a_ref = first_crossing(A0, A1, A2, eta);
        a_def = det_f_crossing(A0, A1, A2, B0, B1, B2, eta);
    }

    // det F of the element = detJ(X + u) / detJ(X)
    static __device__ __forceinline__ double det_f(const double2 (&X)[3], const double2 (&U)[3]) {
        const double2 Y2 = add2(X[2], U[2]);
        return cross2(sub2(add2(X[0], U[0]), Y2), sub2(add2(X[1], U[1]), Y2)) / cross2(sub2(X[0], X[2]), sub2(X[1], X[2]));
    }

    // wscale (1/q - 1) and, if asked for, its gradient per node.  1/q = S / (2 sqrt(3) s det), S = sum |e|^2:
    //   d(1/q)/dX = (dS/dX det - S ddet/dX) / (2 sqrt(3) s det^2),   dS/dX0 = 2 (2 X0 - X1 - X2) (cyclic),
    //   ddet/d(x0, y0) = (y1 - y2, x2 - x1), d(x1, y1) = (y2 - y0, x0 - x2), d(x2, y2) = (y0 - y1, x1 - x0).
    static __device__ __forceinline__ double barrier(const double2 (&X)[3], const double2 (&R)[3], double wscale, bool want_grad,
                                                     double2 (&g)[3]) {
        const double2 X0 = X[0], X1 = X[1], X2 = X[2];
        const double s = orientation(R);
        const double d = det(X0, X1, X2), S = edge_sq_sum(X0, X1, X2);
        const double den = kTwoSqrt3 * s * d;
        if (want_grad) {
            const double f1 = wscale / den, f2 = -wscale * S / (den * d);   // d(wscale * S/den) = f1 dS + f2 ddet
            g[0] = make_double2(f1 * 2.0 * (2.0 * X0.x - X1.x - X2.x) + f2 * (X1.y - X2.y),
                                f1 * 2.0 * (2.0 * X0.y - X1.y - X2.y) + f2 * (X2.x - X1.x));
            g[1] = make_double2(f1 * 2.0 * (2.0 * X1.x - X2.x - X0.x) + f2 * (X2.y - X0.y),
                                f1 * 2.0 * (2.0 * X1.y - X2.y - X0.y) + f2 * (X0.x - X2.x));
            g[2] = make_double2(f1 * 2.0 * (2.0 * X2.x - X0.x - X1.x) + f2 * (X0.y - X1.y),
                                f1 * 2.0 * (2.0 * X2.y - X0.y - X1.y) + f2 * (X1.x - X0.x));
        }
        return wscale * (S / den - 1.0);
    }
};

// ---------------------------------------------------------------- QUAD4
struct Quad4 {
    static constexpr int kNodes = 4;
    static constexpr double kBarrierTerms = 4.0;

    // e_k = X_{k+1} - X_k
    static __device__ __forceinline__ void edges(const double2 (&X)[4], double2 (&E)[4]) {
#pragma unroll
        for (int k = 0; k < 4; ++k) E[k] = sub2(X[(k + 1) & 3], X[k]);
    }

    // s and the four reference cross products of a cell
    static __device__ __forceinline__ double reference_corners(const double2 (&R)[4], double (&cref)[4]) {
        double2 ER[4];
        edges(R, ER);
#pragma unroll
        for (int k = 0; k < 4; ++k) cref[k] = cross2(ER[(k + 3) & 3], ER[k]);
        return sign_of(cref[0] + cref[2]);
    }

    static __device__ __forceinline__ double orientation(const double2 (&R)[4]) {
        double cref[4];
        return reference_corners(R, cref);
    }

    // q = min_k q_k and min_k c_k / c_k_ref of the cell -> inverted; a NaN corner makes a value NaN, and it stays NaN
    static __device__ __forceinline__ bool measure(const double2 (&X)[4], const double2 (&R)[4], double &q, double &ratio) {
        double2 E[4];
        double cref[4];
        const double s = reference_corners(R, cref);
        edges(X, E);
        unsigned inv = 0;
        q = INFINITY;
        ratio = INFINITY;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double2 p = E[(k + 3) & 3], r = E[k];
            const double c = cross2(p, r);
            const double qk = 2.0 * s * c / (norm_sq(p) + norm_sq(r)), rk = c / cref[k];
            q = (qk < q || qk != qk) ? qk : q;
            ratio = (rk < ratio || rk != rk) ? rk : ratio;
            inv |= !(s * c > 0.0);
        }
        return inv != 0;
    }

    // c_k(x + a d) = (p + a dp) x (r + a dr) with p = e_{k-1}, r = e_k and their directions
    static __device__ __forceinline__ void coefficients(const double2 p, const double2 r, const double2 dp, const double2 dr,
                                                        double &A0, double &A1, double &A2) {
        A0 = cross2(p, r);
        A1 = cross2(p, dr) + cross2(dp, r);
        A2 = cross2(dp, dr);
    }

    // min over the corners; a NaN corner from non-finite rows loses every comparison
    static __device__ __forceinline__ double reference_crossing(const double2 (&X)[4], const double2 (&D)[4], double eta) {
        double2 E[4], DE[4];
        edges(X, E);
        edges(D, DE);
        double a = INFINITY;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            double A0, A1, A2;
            coefficients(E[(k + 3) & 3], E[k], DE[(k + 3) & 3], DE[k], A0, A1, A2);
            const double ak = first_crossing(A0, A1, A2, eta);
            a = ak < a ? ak : a;
        }
        return a;
    }

    static __device__ __forceinline__ void hyper_crossings(const double2 (&X)[4], const double2 (&U)[4], const double2 (&D)[4],
                                                           double eta, double &a_ref, double &a_def) {
        double2 Y[4], E[4], EY[4], DE[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) Y[k] = add2(X[k], U[k]);
        edges(X, E);
        edges(Y, EY);
        edges(D, DE);
        a_ref = INFINITY;
        a_def = INFINITY;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            double A0, A1, A2, B0, B1, B2;
            coefficients(E[(k + 3) & 3], E[k], DE[(k + 3) & 3], DE[k], A0, A1, A2);
            coefficients(EY[(k + 3) & 3], EY[k], DE[(k + 3) & 3], DE[k], B0, B1, B2);
            const double ar = first_crossing(A0, A1, A2, eta), ad = det_f_crossing(A0, A1, A2, B0, B1, B2, eta);
            a_ref = ar < a_ref ? ar : a_ref;
            a_def = ad < a_def ? ad : a_def;
        }
    }

    // The smallest corner ratio r_k = c_k^def / c_k of a cell; a NaN corner makes it NaN, and it stays NaN.
    static __device__ __forceinline__ double det_f(const double2 (&X)[4], const double2 (&U)[4]) {
        double2 Y[4], E[4], EY[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) Y[k] = add2(X[k], U[k]);
        edges(X, E);
        edges(Y, EY);
        double j = INFINITY;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double rk = cross2(EY[(k + 3) & 3], EY[k]) / cross2(E[(k + 3) & 3], E[k]);
            j = (rk < j || rk != rk) ? rk : j;
        }
        return j;
    }

    // wscale sum_k (1/q_k - 1) and, if asked for, its gradient per node.  Per corner k, with p = e_{k-1}, r = e_k:
    //   c = p x r, S = |p|^2 + |r|^2, 1/q_k = S / (2 s c):   d(1/q_k) = f1 dS + f2 dc,   f1 = 1 / (2 s c),  f2 = -S / (2 s c^2)
    //   dS/dp = 2 p, dS/dr = 2 r,   dc/dp = (r_y, -r_x),  dc/dr = (-p_y, p_x)
    //   G_p = f1 2 p + f2 (r_y, -r_x),  G_r = f1 2 r + f2 (-p_y, p_x):   dX_{k-1} -= G_p,  dX_k += G_p - G_r,  dX_{k+1} += G_r.
    static __device__ __forceinline__ double barrier(const double2 (&X)[4], const double2 (&R)[4], double wscale, bool want_grad,
                                                     double2 (&g)[4]) {
        double2 E[4];
        const double s = orientation(R);
        edges(X, E);
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = make_double2(0.0, 0.0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int km = (k + 3) & 3, kp = (k + 1) & 3;
            const double2 p = E[km], r = E[k];
            const double c = cross2(p, r), S = norm_sq(p) + norm_sq(r);
            const double den = 2.0 * s * c;
            v += wscale * (S / den - 1.0);
            if (want_grad) {
                const double f1 = 2.0 * wscale / den, f2 = -wscale * S / (den * c);
                const double2 Gp = make_double2(f1 * p.x + f2 * r.y, f1 * p.y - f2 * r.x);
                const double2 Gr = make_double2(f1 * r.x - f2 * p.y, f1 * r.y + f2 * p.x);
                g[km].x -= Gp.x; g[km].y -= Gp.y;
                g[k].x += Gp.x - Gr.x; g[k].y += Gp.y - Gr.y;
                g[kp].x += Gr.x; g[kp].y += Gr.y;
            }
        }
        return v;
    }
};

}  // namespace
}  // namespace hfem
