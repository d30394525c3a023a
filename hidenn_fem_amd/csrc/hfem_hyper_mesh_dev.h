// Per-element closed forms of the finite-strain mesh guard (tri3_hyper_mesh.hip, quad4_hyper_mesh.hip): the two
// crossings of the det F-safe step bound and the deformation measure J.  Plain inline functions of corner rows, no wave
// intrinsics and no memory access: tests/host/hyper_mesh_san_main.cpp compiles this text against tests/host/hip_stub.
//
// A coordinate step x -> x + a d at FIXED nodal u moves the reference element, R(a) = detJ(X + a d) = A0 + A1 a + A2 a^2, and
// the deformed one, D(a) = detJ(X + u + a d) = B0 + B1 a + B2 a^2 (the same d: B2 = A2), so det F(a) = D(a) / R(a).
//   reference crossing   the first a > 0 with R(a) = eta R(0)                      (the small-strain bound, first_crossing)
//   det F crossing       the first a > 0 with D(a) R(0) - eta D(0) R(a) = 0, i.e. det F(a) = eta det F(0): the exact quadratic
//                        (1 - eta) A0 B0 + (B1 A0 - eta B0 A1) a + (B2 A0 - eta B0 A2) a^2, which first_crossing solves as it
//                        stands with A0 B0 in the place of A0 (below the reference crossing R keeps its sign, so the division
//                        by R(a) R(0) changes nothing)
// The element's bound is the smaller of the two; an element whose state is invalid already (A0 B0 <= 0, or NaN) has bound 0.
// QUAD4: the same two crossings per corner, on the corner cross products c_k (reference cell) and c_k^def (deformed cell); the
// cell's bound is the minimum over its corners and its J the smallest corner ratio r_k = c_k^def / c_k.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "hfem_crossing_dev.h"

namespace hfem {
namespace {

__device__ __forceinline__ double2 add2(const double2 p, const double2 r) { return make_double2(p.x + r.x, p.y + r.y); }
__device__ __forceinline__ double2 sub2(const double2 p, const double2 r) { return make_double2(p.x - r.x, p.y - r.y); }
__device__ __forceinline__ double cross2(const double2 p, const double2 r) { return p.x * r.y - p.y * r.x; }

// The first a > 0 at which det F(a) = eta det F(0), from the coefficients of R and D (0: the state is invalid already).
__device__ __forceinline__ double det_f_crossing(double A0, double A1, double A2, double B0, double B1, double B2, double eta) {
    const double p0 = A0 * B0;
    if (!(p0 > 0.0)) return 0.0;                             // det F(0) <= 0, a flat reference element, or NaN
    return first_crossing(p0, B1 * A0 - eta * B0 * A1, B2 * A0 - eta * B0 * A2, eta);
}

// The smaller crossing; a NaN reference crossing (non-finite rows) loses the comparison, the det F crossing is 0 then.
__device__ __forceinline__ double smaller_crossing(double a_ref, double a_def) { return a_ref < a_def ? a_ref : a_def; }

// ---------------------------------------------------------------- TRI3
// detJ(x + a d) with J columns (x0 - x2, x1 - x2) and their directions: the expressions of tri3_step_bound_kernel
__device__ __forceinline__ void tri3_det_coefficients(const double2 X0, const double2 X1, const double2 X2, const double2 D0,
                                                      const double2 D1, const double2 D2, double &A0, double &A1, double &A2) {
    const double ax = X0.x - X2.x, ay = X0.y - X2.y, bx = X1.x - X2.x, by = X1.y - X2.y;
    const double dax = D0.x - D2.x, day = D0.y - D2.y, dbx = D1.x - D2.x, dby = D1.y - D2.y;
    A0 = ax * by - bx * ay;
    A1 = (ax * dby + dax * by) - (bx * day + dbx * ay);
    A2 = dax * dby - dbx * day;
}

__device__ __forceinline__ void tri3_hyper_crossings(const double2 (&X)[3], const double2 (&U)[3], const double2 (&D)[3],
                                                     double eta, double &a_ref, double &a_def) {
    double A0, A1, A2, B0, B1, B2;
    tri3_det_coefficients(X[0], X[1], X[2], D[0], D[1], D[2], A0, A1, A2);
    tri3_det_coefficients(add2(X[0], U[0]), add2(X[1], U[1]), add2(X[2], U[2]), D[0], D[1], D[2], B0, B1, B2);
    a_ref = first_crossing(A0, A1, A2, eta);
    a_def = det_f_crossing(A0, A1, A2, B0, B1, B2, eta);
}

// det F of the element = detJ(X + u) / detJ(X)
__device__ __forceinline__ double tri3_det_f(const double2 (&X)[3], const double2 (&U)[3]) {
    const double2 Y2 = add2(X[2], U[2]);
    return cross2(sub2(add2(X[0], U[0]), Y2), sub2(add2(X[1], U[1]), Y2)) / cross2(sub2(X[0], X[2]), sub2(X[1], X[2]));
}

// ---------------------------------------------------------------- QUAD4 (local nodes counter-clockwise, indices mod 4)
// e_k = X_{k+1} - X_k;  c_k = e_{k-1} x e_k (quad4_mesh.hip)
__device__ __forceinline__ void quad4_edges(const double2 (&X)[4], double2 (&E)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) E[k] = sub2(X[(k + 1) & 3], X[k]);
}

__device__ __forceinline__ void quad4_hyper_crossings(const double2 (&X)[4], const double2 (&U)[4], const double2 (&D)[4],
                                                      double eta, double &a_ref, double &a_def) {
    double2 Y[4], E[4], EY[4], DE[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) Y[k] = add2(X[k], U[k]);
    quad4_edges(X, E);
    quad4_edges(Y, EY);
    quad4_edges(D, DE);
    a_ref = INFINITY;
    a_def = INFINITY;
    // c_k(x + a d) = (e_{k-1} + a de_{k-1}) x (e_k + a de_k), on the reference and on the deformed cell
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double2 p = E[(k + 3) & 3], r = E[k], py = EY[(k + 3) & 3], ry = EY[k], dp = DE[(k + 3) & 3], dr = DE[k];
        const double A0 = cross2(p, r), A1 = cross2(p, dr) + cross2(dp, r), A2 = cross2(dp, dr);
        const double B0 = cross2(py, ry), B1 = cross2(py, dr) + cross2(dp, ry);
        const double ar = first_crossing(A0, A1, A2, eta), ad = det_f_crossing(A0, A1, A2, B0, B1, A2, eta);
        a_ref = ar < a_ref ? ar : a_ref;
        a_def = ad < a_def ? ad : a_def;
    }
}

// The smallest corner ratio r_k = c_k^def / c_k of a cell; a NaN corner makes it NaN, and it stays NaN.
__device__ __forceinline__ double quad4_corner_det_f(const double2 (&X)[4], const double2 (&U)[4]) {
    double2 Y[4], E[4], EY[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) Y[k] = add2(X[k], U[k]);
    quad4_edges(X, E);
    quad4_edges(Y, EY);
    double j = INFINITY;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double rk = cross2(EY[(k + 3) & 3], EY[k]) / cross2(E[(k + 3) & 3], E[k]);
        j = (rk < j || rk != rk) ? rk : j;
    }
    return j;
}

}  // namespace
}  // namespace hfem
