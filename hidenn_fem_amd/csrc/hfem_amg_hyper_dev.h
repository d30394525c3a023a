// One row of the assembled Neo-Hookean tangent K_T,ff: the body of amg_assemble_hyper_kernel (tri3_amg.hip),
// one call per free u row.  Plain C++ over double2 / make_double2 and the element headers only, so that the very same text
// compiles for the host (tests/host/amg_hyper_san_main.cpp runs it under the sanitizers with output buffers of exactly the
// pattern's size).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "hfem_hyper_dev.h"
#include "hfem_quad4_hyper_dev.h"

namespace hfem {

// A row by its row code (conn_x for coordinates, conn_u for displacements): a free row, or fixed row -1 - code.
__device__ __forceinline__ double2 coded_row(const double2 *free_rows, const double2 *fixed_rows, int32_t code) {
    return code >= 0 ? free_rows[code] : fixed_rows[-1 - code];
}

// Columns (a, x) and (a, y) of the element tangent at (X, U) -- by symmetry its rows (a, x) and (a, y).  The unit directions
// are formed by selects on `a`, never by an index into a local array.  The inversion rule is the element functions' own: an
// inverted element or cell gives zeros.
__device__ __forceinline__ void hyper_unit_columns(const double2 (&X)[3], const double2 (&U)[3], int a, double lambda, double mu,
                                                   double W, double2 (&gu)[3], double2 (&hu)[3]) {
    const double2 o = make_double2(0.0, 0.0), ex = make_double2(1.0, 0.0), ey = make_double2(0.0, 1.0);
    HyperConsts k{};
    k.lambda = lambda; k.mu = mu; k.W = W;
    const HyperTangent t = hyper_tangent_state(X[0], X[1], X[2], U[0], U[1], U[2], k);
    hyper_tangent_apply(t, k, a == 0 ? ex : o, a == 1 ? ex : o, a == 2 ? ex : o, gu);
    hyper_tangent_apply(t, k, a == 0 ? ey : o, a == 1 ? ey : o, a == 2 ? ey : o, hu);
}

__device__ __forceinline__ void hyper_unit_columns(const double2 (&X)[4], const double2 (&U)[4], int a, double lambda, double mu,
                                                   double, double2 (&gu)[4], double2 (&hu)[4]) {
    const double2 o = make_double2(0.0, 0.0), ex = make_double2(1.0, 0.0), ey = make_double2(0.0, 1.0);
    Quad4HyperConsts k{};
    k.lambda = lambda; k.mu = mu;
    const double2 Px[4] = {a == 0 ? ex : o, a == 1 ? ex : o, a == 2 ? ex : o, a == 3 ? ex : o};
    const double2 Py[4] = {a == 0 ? ey : o, a == 1 ? ey : o, a == 2 ? ey : o, a == 3 ? ey : o};
    double jmin;
    bool inverted;
    quad4_hyper_tangent_apply(X, U, Px, k, gu, jmin, inverted);
    quad4_hyper_tangent_apply(X, U, Py, k, hu, jmin, inverted);
}

// Row r of K_T,ff in 2x2 blocks: zero the row's blocks, then walk the row's element fan in ascending element order and add
// the corner's two rows of every K_e into the NPE fan slots of the entry (s < 0: a Dirichlet column, dropped).  Writes
// a_val[4 a_ptr[r] .. 4 a_ptr[r + 1]) only.
template <int NPE>
__device__ __forceinline__ void amg_hyper_row(int32_t r, const int32_t *fan_ptr, const int32_t *fan_elem, const int32_t *fan_corner,
                                              const int32_t *fan_slot, const int32_t *conn_x, const int32_t *conn_u,
                                              const double2 *x_free, const double2 *x_fixed, const double2 *u_free,
                                              const double2 *u_fixed, const int32_t *a_ptr, double *a_val, double lambda,
                                              double mu, double W) {
    for (int32_t s = a_ptr[r]; s < a_ptr[r + 1]; ++s) {
        double *p = a_val + 4 * (size_t)s;
        p[0] = 0.0; p[1] = 0.0; p[2] = 0.0; p[3] = 0.0;
    }
    for (int32_t f = fan_ptr[r]; f < fan_ptr[r + 1]; ++f) {
        const int32_t e = fan_elem[f], a = fan_corner[f];
        const int32_t *cx = conn_x + NPE * (size_t)e, *cu = conn_u + NPE * (size_t)e;
        double2 X[NPE], U[NPE], gu[NPE], hu[NPE];
#pragma unroll
        for (int b = 0; b < NPE; ++b) {
            X[b] = coded_row(x_free, x_fixed, cx[b]);
            U[b] = coded_row(u_free, u_fixed, cu[b]);
        }
        hyper_unit_columns(X, U, a, lambda, mu, W, gu, hu);
#pragma unroll
        for (int b = 0; b < NPE; ++b) {
            const int32_t s = fan_slot[NPE * (size_t)f + b];
            if (s < 0) continue;
            double *p = a_val + 4 * (size_t)s;
            p[0] += gu[b].x; p[1] += gu[b].y; p[2] += hu[b].x; p[3] += hu[b].y;
        }
    }
}

}  // namespace hfem
