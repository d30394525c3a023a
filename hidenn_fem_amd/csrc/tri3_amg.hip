// Smoothed-aggregation AMG for the frozen-mesh solve (TRI3 and QUAD4), gfx950 (MI355X): the numeric setup of the hierarchy
// whose patterns amg.cpp built, and the symmetric V-cycle that preconditions CG (cg.hip, hfem_cg_iterate_amg).  All fp64.
//
// Numeric setup (hfem_amg_setup, at every solver refresh):
//   amg_assemble_kernel   K_ff in 2x2 blocks, NPE = 3 | 4 corners per element: one thread per free row walks the row's element
//                         fan in ascending element order and adds that corner's 2 x 2 NPE rows of K_e (unit_columns,
//                         hfem_cg_dev.h: the closed forms of the CG apply at unit displacements, both gradient conventions)
//                         into the row's blocks through NPE fan slots per record.  No atomics: bit-deterministic.
//   amg_dinv_kernel       inverse of every (symmetrised) diagonal block; an all-zero row counts as an identity row.
//   amg_power_*           lambda_max(D^-1 A) by kAmgPowerIters power steps from a fixed start; lambda_hat = 1.1 x estimate.
//   amg_tentative_kernel  one thread per aggregate: modified Gram-Schmidt of the aggregate's near-null-space rows (2k x 3 on
//                         the fine level: translations and the rotation (-y, x) at the current coordinates; 3k x 3 below);
//                         R becomes the next level's near-null space.  A column below 1e-10 of the first column's norm is 0.
//   amg_smooth_p_kernel   P = (I - omega D^-1 A) P_tent, omega = 4 / (3 lambda_hat); one thread per row.
//   amg_ap_kernel, amg_rap_kernel   A_c = R (A P): row-wise numeric products into the precomputed patterns (slot by binary
//                         search), each output row summed in a fixed order.
//   amg_coarse_scatter_kernel       the coarsest A into a dense matrix for the host-side inverse.
// Tangent setup (hfem_amg_setup_hyper, at a Newton linearisation): the same numeric setup on the assembled
// Neo-Hookean tangent K_T,ff at (x, u):
//   amg_assemble_hyper_kernel   amg_assemble_kernel's walk with the element tangent (hfem_amg_hyper_dev.h: U gathered through
//                         conn_u, the two unit directions at the corner by selects, state + two applies for TRI3, two fused
//                         applies for QUAD4).  An inverted element or cell contributes zeros, so the matrix is exactly the
//                         operator hfem_cg_apply applies on a hyper handle.  No atomics: bit-deterministic.
//   amg_ns0_kernel        with u_free: the rotation column at the deformed position, (-(y + v), x + u).
// Shifted setup (hfem_amg_setup_shifted, a Newmark step of implicit dynamics): the same numeric setup on
// A_ff = c_K K_ff + c_M M_ff, assembled by the Mass instance of amg_assemble_kernel.  Scaled setup (hfem_amg_setup_scaled;
// DESIGN 30): the same on K(w)_ff = sum_e w_e K_e,ff, assembled by its Scaled instance.
// Everything from setup_level down is shared.  One handle may be set up by either entry point, in any order: pointers and
// patterns never change, only values do, so a captured hfem_cg_iterate_amg graph stays valid across re-setups of either kind.
// V-cycle (amg_cycle): Chebyshev degree 2 on D^-1 A over [lambda_hat / 30, lambda_hat], the same polynomial before and after
// the coarse correction (a symmetric positive-definite M), block SpMV with the recurrence fused (amg_cheb_kernel), R and P
// products, and a dense GEMV with the coarsest inverse.  Every cycle launch returns at once when the CG status record says
// halted, so iterations replayed behind the last one do nothing.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>

#include "hfem_amg.h"
#include "hfem_amg_hyper_dev.h"
#include "hfem_cg_dev.h"
#include "hfem_device.h"
#include "hfem_plan_dev.h"

namespace hfem {
namespace {

constexpr int kBlock = 256, kRedBlocks = 256;
// per-level coefficient record (device doubles)
enum { kLam = 0, kInvTheta, kC1, kC2, kOmega, kScale, kNorm, kCoefN = 8 };

__device__ __forceinline__ bool halted(const double *st) { return st && st[kHalted] != 0.0; }

__device__ __forceinline__ int32_t find_slot(const int32_t *__restrict__ col, int32_t lo, int32_t hi, int32_t key) {
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (col[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------- assembly (fine level, 2x2 blocks)
// Mass: A_ff = c_K K_ff + c_M M_ff (implicit dynamics): the same walk, k scaled by c_K on the host, plus the
// corner's mass row (dyn_mass_row, hfem_cg_dev.h) on xx and yy of every block.  Scaled: K(w)_ff = sum_e w_e K_e,ff (a design
// iteration or a multi-material solve): the same walk, the element's four block entries times its weight, read by
// global element id from w_elem.  Only the Mass instance reads dm, only the Scaled one w_elem.
template <int NPE, bool PHYS, ElemOp OP>
__global__ __launch_bounds__(kBlock) void amg_assemble_kernel(int32_t n, const int32_t *__restrict__ fan_ptr,
                                                              const int32_t *__restrict__ fan_elem,
                                                              const int32_t *__restrict__ fan_corner,
                                                              const int32_t *__restrict__ fan_slot,
                                                              const int32_t *__restrict__ conn_x,
                                                              const double2 *__restrict__ x_free,
                                                              const double2 *__restrict__ x_fixed,
                                                              const int32_t *__restrict__ a_ptr, double *__restrict__ a_val,
                                                              Tri3Consts k, DynMass dm, const double *__restrict__ w_elem) {
    const int32_t r = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (r >= n) return;
    for (int32_t s = a_ptr[r]; s < a_ptr[r + 1]; ++s)
        *reinterpret_cast<double4 *>(a_val + 4 * (size_t)s) = make_double4(0.0, 0.0, 0.0, 0.0);
    for (int32_t f = fan_ptr[r]; f < fan_ptr[r + 1]; ++f) {
        const int32_t e = fan_elem[f], a = fan_corner[f];
        const int32_t *cx = conn_x + NPE * (size_t)e;
        double w = 0.0;                                        // the element's weight (Scaled only)
        if constexpr (OP == ElemOp::Scaled) w = w_elem[e];
        double2 X[NPE], gu[NPE], hu[NPE];
        double mrow[NPE];                                      // M_e[a][.] (Mass only)
#pragma unroll
        for (int b = 0; b < NPE; ++b) X[b] = x_row(x_free, x_fixed, cx[b]);
        unit_columns<PHYS>(X, a, k, gu, hu);                   // column (a, x) and (a, y) of K_e = rows (a, x) and (a, y)
        if constexpr (OP == ElemOp::Mass) dyn_mass_row(X, a, dm, mrow);
#pragma unroll
        for (int b = 0; b < NPE; ++b) {
            const int32_t s = fan_slot[NPE * (size_t)f + b];
            if (s < 0) continue;
            double4 *p = reinterpret_cast<double4 *>(a_val + 4 * (size_t)s);
            double4 v = *p;
            if constexpr (OP == ElemOp::Scaled) {
                v.x += w * gu[b].x; v.y += w * gu[b].y; v.z += w * hu[b].x; v.w += w * hu[b].y;
            } else {
                double xx = gu[b].x, yy = hu[b].y;
                if constexpr (OP == ElemOp::Mass) { xx += mrow[b]; yy += mrow[b]; }   // never "+ 0.0" in the plain instance
                v.x += xx; v.y += gu[b].y; v.z += hu[b].x; v.w += yy;
            }
            *p = v;
        }
    }
}

// K_T,ff of the Neo-Hookean energy at (x, u): one thread per free row runs amg_hyper_row (hfem_amg_hyper_dev.h)
template <int NPE>
__global__ __launch_bounds__(kBlock) void amg_assemble_hyper_kernel(int32_t n, const int32_t *__restrict__ fan_ptr,
                                                                    const int32_t *__restrict__ fan_elem,
                                                                    const int32_t *__restrict__ fan_corner,
                                                                    const int32_t *__restrict__ fan_slot,
                                                                    const int32_t *__restrict__ conn_x,
                                                                    const int32_t *__restrict__ conn_u,
                                                                    const double2 *__restrict__ x_free,
                                                                    const double2 *__restrict__ x_fixed,
                                                                    const double2 *__restrict__ u_free,
                                                                    const double2 *__restrict__ u_fixed,
                                                                    const int32_t *__restrict__ a_ptr, double *__restrict__ a_val,
                                                                    double lambda, double mu, double W) {
    const int32_t r = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (r >= n) return;
    amg_hyper_row<NPE>(r, fan_ptr, fan_elem, fan_corner, fan_slot, conn_x, conn_u, x_free, x_fixed, u_free, u_fixed, a_ptr, a_val,
                       lambda, mu, W);
}

// ---------------------------------------------------------------- diagonal block inverses
template <int BS>
__global__ __launch_bounds__(kBlock) void amg_dinv_kernel(int32_t n, const int32_t *__restrict__ a_diag,
                                                          const double *__restrict__ a_val, double *__restrict__ dinv) {
    const int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (i >= n) return;
    double D[BS][BS];
    const int32_t s = a_diag[i];
#pragma unroll
    for (int r = 0; r < BS; ++r)
#pragma unroll
        for (int c = 0; c < BS; ++c)
            D[r][c] = s < 0 ? 0.0 : 0.5 * (a_val[(size_t)s * BS * BS + r * BS + c] + a_val[(size_t)s * BS * BS + c * BS + r]);
#pragma unroll
    for (int r = 0; r < BS; ++r)
        if (D[r][r] == 0.0) D[r][r] = 1.0;                 // an all-zero row (dropped near-null-space column) acts as identity
    double I[BS][BS];
    bool ok;
    if constexpr (BS == 2) {
        const double det = D[0][0] * D[1][1] - D[0][1] * D[1][0];
        ok = det > 0.0 && isfinite(det);
        const double inv = 1.0 / det;
        I[0][0] = D[1][1] * inv; I[0][1] = -D[0][1] * inv; I[1][0] = -D[1][0] * inv; I[1][1] = D[0][0] * inv;
    } else {
        const double c00 = D[1][1] * D[2][2] - D[1][2] * D[2][1], c01 = D[1][2] * D[2][0] - D[1][0] * D[2][2],
                     c02 = D[1][0] * D[2][1] - D[1][1] * D[2][0];
        const double det = D[0][0] * c00 + D[0][1] * c01 + D[0][2] * c02;
        ok = det > 0.0 && isfinite(det);
        const double inv = 1.0 / det;
        I[0][0] = c00 * inv; I[1][0] = c01 * inv; I[2][0] = c02 * inv;
        I[0][1] = (D[0][2] * D[2][1] - D[0][1] * D[2][2]) * inv;
        I[1][1] = (D[0][0] * D[2][2] - D[0][2] * D[2][0]) * inv;
        I[2][1] = (D[0][1] * D[2][0] - D[0][0] * D[2][1]) * inv;
        I[0][2] = (D[0][1] * D[1][2] - D[0][2] * D[1][1]) * inv;
        I[1][2] = (D[0][2] * D[1][0] - D[0][0] * D[1][2]) * inv;
        I[2][2] = (D[0][0] * D[1][1] - D[0][1] * D[1][0]) * inv;
    }
#pragma unroll
    for (int r = 0; r < BS; ++r)
#pragma unroll
        for (int c = 0; c < BS; ++c)
            dinv[(size_t)i * BS * BS + r * BS + c] = ok ? 0.5 * (I[r][c] + I[c][r]) : (r == c ? 1.0 : 0.0);
}

// ---------------------------------------------------------------- lambda_max(D^-1 A): power iteration
__global__ __launch_bounds__(kBlock) void amg_power_init_kernel(int64_t m, double *__restrict__ v, double *__restrict__ part) {
    __shared__ double red[kBlock / 64];
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += (int64_t)gridDim.x * kBlock) {
        const uint32_t h = (uint32_t)(i + 1) * 2654435761u;
        const double x = (double)(h >> 8) * (1.0 / 16777216.0) - 0.5;
        v[i] = x;
        acc += x * x;
    }
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// w = D^-1 A (scale v), partial sums of |w|^2
template <int BS>
__global__ __launch_bounds__(kBlock) void amg_power_kernel(int32_t n, const int32_t *__restrict__ a_ptr,
                                                           const int32_t *__restrict__ a_col, const double *__restrict__ a_val,
                                                           const double *__restrict__ dinv, const double *__restrict__ v,
                                                           double *__restrict__ w, const double *__restrict__ coef,
                                                           double *__restrict__ part) {
    __shared__ double red[kBlock / 64];
    const double sc = coef[kScale];
    double acc = 0.0;
    for (int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x); i < n; i += (int32_t)(gridDim.x * kBlock)) {
        double t[BS];
#pragma unroll
        for (int r = 0; r < BS; ++r) t[r] = 0.0;
        for (int32_t s = a_ptr[i]; s < a_ptr[i + 1]; ++s) {
            const int32_t j = a_col[s];
            const double *A = a_val + (size_t)s * BS * BS;
#pragma unroll
            for (int r = 0; r < BS; ++r)
#pragma unroll
                for (int c = 0; c < BS; ++c) t[r] = __builtin_fma(A[r * BS + c], v[(size_t)j * BS + c], t[r]);
        }
        const double *Di = dinv + (size_t)i * BS * BS;
#pragma unroll
        for (int r = 0; r < BS; ++r) {
            double y = 0.0;
#pragma unroll
            for (int c = 0; c < BS; ++c) y = __builtin_fma(Di[r * BS + c], t[c], y);
            y *= sc;
            w[(size_t)i * BS + r] = y;
            acc += y * y;
        }
    }
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// one block: fixed-order sum of the partials; first = scale of the start vector, else the estimate and the cycle coefficients
__global__ __launch_bounds__(kBlock) void amg_power_finish_kernel(const double *__restrict__ part, int nb, double *coef, int first) {
    __shared__ double red[kBlock / 64];
    double a = 0.0;
    for (int i = threadIdx.x; i < nb; i += kBlock) a += part[i];
    const double ss = block_sum(a, red);
    if (threadIdx.x != 0) return;
    const double nrm = sqrt(ss);
    coef[kScale] = nrm > 0.0 ? 1.0 / nrm : 0.0;
    if (first) return;
    coef[kNorm] = nrm;
    const double lam = 1.1 * nrm;
    const double lo = lam / 30.0, theta = 0.5 * (lam + lo), delta = 0.5 * (lam - lo);
    const double sigma = theta / delta, rho0 = 1.0 / sigma, rho1 = 1.0 / (2.0 * sigma - rho0);
    coef[kLam] = lam;
    coef[kInvTheta] = 1.0 / theta;
    coef[kC1] = rho1 * rho0;
    coef[kC2] = 2.0 * rho1 / delta;
    coef[kOmega] = 4.0 / (3.0 * lam);
}

// ---------------------------------------------------------------- near-null space and tentative prolongator
// fine level: rows [[1, 0, -y], [0, 1, x]] of every free u row at the current coordinates; with u_free (the tangent setup)
// at the deformed position, [[1, 0, -(y + v)], [0, 1, x + u]]
__global__ __launch_bounds__(kBlock) void amg_ns0_kernel(int32_t n, const int32_t *__restrict__ row_x,
                                                         const double2 *__restrict__ x_free, const double2 *__restrict__ x_fixed,
                                                         const double2 *__restrict__ u_free, double *__restrict__ ns) {
    const int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (i >= n) return;
    double2 X = x_row(x_free, x_fixed, row_x[i]);
    if (u_free) {
        const double2 U = u_free[i];
        X.x += U.x; X.y += U.y;
    }
    double *o = ns + (size_t)i * 6;
    o[0] = 1.0; o[1] = 0.0; o[2] = -X.y;
    o[3] = 0.0; o[4] = 1.0; o[5] = X.x;
}

// Q (into ptent, the aggregate's member rows) and R (into ns_next, 3x3 row-major) of the modified Gram-Schmidt QR of the
// aggregate's near-null-space rows.  Columns are processed one pass over the members at a time (no local arrays).
template <int BS>
__global__ __launch_bounds__(kBlock) void amg_tentative_kernel(int32_t n_agg, const int32_t *__restrict__ agg_ptr,
                                                               const int32_t *__restrict__ agg_rows, const double *__restrict__ ns,
                                                               double *__restrict__ q, double *__restrict__ ns_next) {
    const int32_t I = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (I >= n_agg) return;
    const int32_t b = agg_ptr[I], e = agg_ptr[I + 1];
    auto Q = [&](int32_t t, int k, int c) -> double & { return q[(size_t)agg_rows[t] * BS * 3 + k * 3 + c]; };
    double n0 = 0.0;
    for (int32_t t = b; t < e; ++t)
#pragma unroll
        for (int k = 0; k < BS; ++k) {
            const double *src = ns + (size_t)agg_rows[t] * BS * 3 + k * 3;
            Q(t, k, 0) = src[0]; Q(t, k, 1) = src[1]; Q(t, k, 2) = src[2];
            n0 += src[0] * src[0];
        }
    n0 = sqrt(n0);
    const double tol = 1e-10 * n0;
    const double s0 = n0 > 0.0 ? 1.0 / n0 : 0.0;
    double r01 = 0.0, r02 = 0.0;
    for (int32_t t = b; t < e; ++t)
#pragma unroll
        for (int k = 0; k < BS; ++k) {
            const double v = Q(t, k, 0) * s0;
            Q(t, k, 0) = v;
            r01 += v * Q(t, k, 1);
        }
    // column 1
    double n1 = 0.0;
    for (int32_t t = b; t < e; ++t)
#pragma unroll
        for (int k = 0; k < BS; ++k) {
            const double v = __builtin_fma(-r01, Q(t, k, 0), Q(t, k, 1));
            Q(t, k, 1) = v;
            n1 += v * v;
            r02 += Q(t, k, 0) * Q(t, k, 2);
        }
    n1 = sqrt(n1);
    const bool keep1 = n1 > tol && n1 > 0.0;
    const double s1 = keep1 ? 1.0 / n1 : 0.0;
    // column 2 against q0, then q1 (modified Gram-Schmidt)
    double r12 = 0.0;
    for (int32_t t = b; t < e; ++t)
#pragma unroll
        for (int k = 0; k < BS; ++k) {
            const double v1 = Q(t, k, 1) * s1;
            Q(t, k, 1) = v1;
            const double v2 = __builtin_fma(-r02, Q(t, k, 0), Q(t, k, 2));
            Q(t, k, 2) = v2;
            r12 += v1 * v2;
        }
    double n2 = 0.0;
    for (int32_t t = b; t < e; ++t)
#pragma unroll
        for (int k = 0; k < BS; ++k) {
            const double v = __builtin_fma(-r12, Q(t, k, 1), Q(t, k, 2));
            Q(t, k, 2) = v;
            n2 += v * v;
        }
    n2 = sqrt(n2);
    const bool keep2 = n2 > tol && n2 > 0.0;
    const double s2 = keep2 ? 1.0 / n2 : 0.0;
    for (int32_t t = b; t < e; ++t)
#pragma unroll
        for (int k = 0; k < BS; ++k) Q(t, k, 2) *= s2;
    double *R = ns_next + (size_t)I * 9;
    R[0] = n0; R[1] = r01; R[2] = r02;
    R[3] = 0.0; R[4] = keep1 ? n1 : 0.0; R[5] = keep1 ? r12 : 0.0;
    R[6] = 0.0; R[7] = 0.0; R[8] = keep2 ? n2 : 0.0;
}

// ---------------------------------------------------------------- smoothed prolongator and Galerkin product
// P_i = [agg(i)] T_i - omega D_i^-1 sum_j A_ij T_j, T = P_tent (one BS x 3 block per row)
template <int BS>
__global__ __launch_bounds__(kBlock) void amg_smooth_p_kernel(int32_t n, const int32_t *__restrict__ a_ptr,
                                                              const int32_t *__restrict__ a_col, const double *__restrict__ a_val,
                                                              const double *__restrict__ dinv, const int32_t *__restrict__ agg,
                                                              const double *__restrict__ tent, const int32_t *__restrict__ p_ptr,
                                                              const int32_t *__restrict__ p_col, double *__restrict__ p_val,
                                                              const double *__restrict__ coef) {
    const int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (i >= n) return;
    constexpr int PB = BS * 3;
    const int32_t p0 = p_ptr[i], p1 = p_ptr[i + 1];
    for (int32_t s = p0; s < p1; ++s)
#pragma unroll
        for (int m = 0; m < PB; ++m) p_val[(size_t)s * PB + m] = 0.0;
    for (int32_t t = a_ptr[i]; t < a_ptr[i + 1]; ++t) {
        const int32_t j = a_col[t];
        const int32_t s = find_slot(p_col, p0, p1, agg[j]);
        const double *A = a_val + (size_t)t * BS * BS, *T = tent + (size_t)j * PB;
        double *o = p_val + (size_t)s * PB;
#pragma unroll
        for (int r = 0; r < BS; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double acc = o[r * 3 + c];
#pragma unroll
                for (int l = 0; l < BS; ++l) acc = __builtin_fma(A[r * BS + l], T[l * 3 + c], acc);
                o[r * 3 + c] = acc;
            }
    }
    const double w = coef[kOmega];
    const int32_t ai = agg[i];
    const double *Di = dinv + (size_t)i * BS * BS, *Ti = tent + (size_t)i * PB;
    for (int32_t s = p0; s < p1; ++s) {
        double *o = p_val + (size_t)s * PB;
        double m[PB];
#pragma unroll
        for (int x = 0; x < PB; ++x) m[x] = o[x];
        const bool own = p_col[s] == ai;
#pragma unroll
        for (int r = 0; r < BS; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double acc = 0.0;
#pragma unroll
                for (int l = 0; l < BS; ++l) acc = __builtin_fma(Di[r * BS + l], m[l * 3 + c], acc);
                o[r * 3 + c] = (own ? Ti[r * 3 + c] : 0.0) - w * acc;
            }
    }
}

// AP_i = sum_j A_ij P_j (BS x 3 blocks)
template <int BS>
__global__ __launch_bounds__(kBlock) void amg_ap_kernel(int32_t n, const int32_t *__restrict__ a_ptr, const int32_t *__restrict__ a_col,
                                                        const double *__restrict__ a_val, const int32_t *__restrict__ p_ptr,
                                                        const int32_t *__restrict__ p_col, const double *__restrict__ p_val,
                                                        const int32_t *__restrict__ ap_ptr, const int32_t *__restrict__ ap_col,
                                                        double *__restrict__ ap_val) {
    const int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (i >= n) return;
    constexpr int PB = BS * 3;
    const int32_t q0 = ap_ptr[i], q1 = ap_ptr[i + 1];
    for (int32_t s = q0; s < q1; ++s)
#pragma unroll
        for (int m = 0; m < PB; ++m) ap_val[(size_t)s * PB + m] = 0.0;
    for (int32_t t = a_ptr[i]; t < a_ptr[i + 1]; ++t) {
        const int32_t j = a_col[t];
        const double *A = a_val + (size_t)t * BS * BS;
        for (int32_t u = p_ptr[j]; u < p_ptr[j + 1]; ++u) {
            const int32_t s = find_slot(ap_col, q0, q1, p_col[u]);
            const double *P = p_val + (size_t)u * PB;
            double *o = ap_val + (size_t)s * PB;
#pragma unroll
            for (int r = 0; r < BS; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    double acc = o[r * 3 + c];
#pragma unroll
                    for (int l = 0; l < BS; ++l) acc = __builtin_fma(A[r * BS + l], P[l * 3 + c], acc);
                    o[r * 3 + c] = acc;
                }
        }
    }
}

// A_c,I = sum_{j in R row I} P_jI^T AP_j (3 x 3 blocks)
template <int BS>
__global__ __launch_bounds__(kBlock) void amg_rap_kernel(int32_t nc, const int32_t *__restrict__ r_ptr, const int32_t *__restrict__ r_col,
                                                         const int32_t *__restrict__ r_pidx, const double *__restrict__ p_val,
                                                         const int32_t *__restrict__ ap_ptr, const int32_t *__restrict__ ap_col,
                                                         const double *__restrict__ ap_val, const int32_t *__restrict__ c_ptr,
                                                         const int32_t *__restrict__ c_col, double *__restrict__ c_val) {
    const int32_t I = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (I >= nc) return;
    constexpr int PB = BS * 3;
    const int32_t c0 = c_ptr[I], c1 = c_ptr[I + 1];
    for (int32_t s = c0; s < c1; ++s)
#pragma unroll
        for (int m = 0; m < 9; ++m) c_val[(size_t)s * 9 + m] = 0.0;
    for (int32_t t = r_ptr[I]; t < r_ptr[I + 1]; ++t) {
        const int32_t j = r_col[t];
        const double *P = p_val + (size_t)r_pidx[t] * PB;
        for (int32_t u = ap_ptr[j]; u < ap_ptr[j + 1]; ++u) {
            const int32_t s = find_slot(c_col, c0, c1, ap_col[u]);
            const double *M = ap_val + (size_t)u * PB;
            double *o = c_val + (size_t)s * 9;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    double acc = o[r * 3 + c];
#pragma unroll
                    for (int l = 0; l < BS; ++l) acc = __builtin_fma(P[l * 3 + r], M[l * 3 + c], acc);
                    o[r * 3 + c] = acc;
                }
        }
    }
}

// coarsest A into a dense row-major N x N matrix (zeroed beforehand); an all-zero row gets a 1 on its diagonal
template <int BS>
__global__ __launch_bounds__(kBlock) void amg_coarse_scatter_kernel(int32_t n, const int32_t *__restrict__ a_ptr,
                                                                    const int32_t *__restrict__ a_col, const double *__restrict__ a_val,
                                                                    double *__restrict__ dense) {
    const int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (i >= n) return;
    const size_t N = (size_t)n * BS;
#pragma unroll
    for (int r = 0; r < BS; ++r) {
        bool zero = true;
        for (int32_t s = a_ptr[i]; s < a_ptr[i + 1]; ++s)
#pragma unroll
            for (int c = 0; c < BS; ++c) {
                const double v = a_val[(size_t)s * BS * BS + r * BS + c];
                dense[((size_t)i * BS + r) * N + (size_t)a_col[s] * BS + c] = v;
                zero = zero && v == 0.0;
            }
        if (zero) dense[((size_t)i * BS + r) * (N + 1)] = 1.0;
    }
}

// ---------------------------------------------------------------- V-cycle kernels
// One Chebyshev step fused into the block SpMV: r = b - A x_in (x_in NULL: 0); r_out = r (optional); with x_out:
// d = c1 d + c2 D^-1 r (step 0: c1 = 0, c2 = 1 / theta) and x_out = x_in + d.
template <int BS>
__global__ __launch_bounds__(kBlock) void amg_cheb_kernel(int32_t n, const int32_t *__restrict__ a_ptr,
                                                          const int32_t *__restrict__ a_col, const double *__restrict__ a_val,
                                                          const double *__restrict__ dinv, const double *__restrict__ x_in,
                                                          const double *__restrict__ b, double *__restrict__ d,
                                                          double *__restrict__ x_out, double *__restrict__ r_out,
                                                          const double *__restrict__ coef, int step, const double *st) {
    if (halted(st)) return;
    const int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (i >= n) return;
    double r[BS];
#pragma unroll
    for (int k = 0; k < BS; ++k) r[k] = b[(size_t)i * BS + k];
    if (x_in) {
        for (int32_t s = a_ptr[i]; s < a_ptr[i + 1]; ++s) {
            const int32_t j = a_col[s];
            const double *A = a_val + (size_t)s * BS * BS;
            double xj[BS];
#pragma unroll
            for (int c = 0; c < BS; ++c) xj[c] = x_in[(size_t)j * BS + c];
#pragma unroll
            for (int k = 0; k < BS; ++k)
#pragma unroll
                for (int c = 0; c < BS; ++c) r[k] = __builtin_fma(-A[k * BS + c], xj[c], r[k]);
        }
    }
    if (r_out)
#pragma unroll
        for (int k = 0; k < BS; ++k) r_out[(size_t)i * BS + k] = r[k];
    if (!x_out) return;
    const double c1 = step ? coef[kC1] : 0.0, c2 = step ? coef[kC2] : coef[kInvTheta];
    const double *Di = dinv + (size_t)i * BS * BS;
#pragma unroll
    for (int k = 0; k < BS; ++k) {
        double z = 0.0;
#pragma unroll
        for (int c = 0; c < BS; ++c) z = __builtin_fma(Di[k * BS + c], r[c], z);
        double dk = c2 * z;
        if (step) dk = __builtin_fma(c1, d[(size_t)i * BS + k], dk);
        d[(size_t)i * BS + k] = dk;
        x_out[(size_t)i * BS + k] = (x_in ? x_in[(size_t)i * BS + k] : 0.0) + dk;
    }
}

// b_c,I = sum_{j in R row I} P_jI^T r_j
template <int BS>
__global__ __launch_bounds__(kBlock) void amg_restrict_kernel(int32_t nc, const int32_t *__restrict__ r_ptr,
                                                              const int32_t *__restrict__ r_col, const int32_t *__restrict__ r_pidx,
                                                              const double *__restrict__ p_val, const double *__restrict__ r,
                                                              double *__restrict__ bc, const double *st) {
    if (halted(st)) return;
    const int32_t I = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (I >= nc) return;
    double y0 = 0.0, y1 = 0.0, y2 = 0.0;
    for (int32_t t = r_ptr[I]; t < r_ptr[I + 1]; ++t) {
        const double *P = p_val + (size_t)r_pidx[t] * BS * 3, *v = r + (size_t)r_col[t] * BS;
#pragma unroll
        for (int l = 0; l < BS; ++l) {
            const double vl = v[l];
            y0 = __builtin_fma(P[l * 3], vl, y0);
            y1 = __builtin_fma(P[l * 3 + 1], vl, y1);
            y2 = __builtin_fma(P[l * 3 + 2], vl, y2);
        }
    }
    bc[(size_t)I * 3] = y0; bc[(size_t)I * 3 + 1] = y1; bc[(size_t)I * 3 + 2] = y2;
}

// x_i += sum_K P_iK x_c,K
template <int BS>
__global__ __launch_bounds__(kBlock) void amg_prolong_kernel(int32_t n, const int32_t *__restrict__ p_ptr,
                                                             const int32_t *__restrict__ p_col, const double *__restrict__ p_val,
                                                             const double *__restrict__ xc, double *__restrict__ x, const double *st) {
    if (halted(st)) return;
    const int32_t i = (int32_t)(blockIdx.x * kBlock + threadIdx.x);
    if (i >= n) return;
    double y[BS];
#pragma unroll
    for (int k = 0; k < BS; ++k) y[k] = x[(size_t)i * BS + k];
    for (int32_t s = p_ptr[i]; s < p_ptr[i + 1]; ++s) {
        const double *P = p_val + (size_t)s * BS * 3, *v = xc + (size_t)p_col[s] * 3;
        const double v0 = v[0], v1 = v[1], v2 = v[2];
#pragma unroll
        for (int k = 0; k < BS; ++k)
            y[k] = __builtin_fma(P[k * 3 + 2], v2, __builtin_fma(P[k * 3 + 1], v1, __builtin_fma(P[k * 3], v0, y[k])));
    }
#pragma unroll
    for (int k = 0; k < BS; ++k) x[(size_t)i * BS + k] = y[k];
}

// x = Ainv b on the coarsest level: one wave per row, lanes strided over the columns, fixed-order wave sum
__global__ __launch_bounds__(kBlock) void amg_coarse_gemv_kernel(int32_t N, const double *__restrict__ ainv,
                                                                 const double *__restrict__ b, double *__restrict__ x,
                                                                 const double *st) {
    if (halted(st)) return;
    const int32_t row = (int32_t)(blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    if (row >= N) return;
    const double *a = ainv + (size_t)row * N;
    double acc = 0.0;
    for (int32_t c = lane; c < N; c += 64) acc = __builtin_fma(a[c], b[c], acc);
    acc = wave_sum(acc);
    if (lane == 0) x[row] = acc;
}

inline dim3 grid_of(int64_t n) { return dim3((unsigned)std::max<int64_t>(1, (n + kBlock - 1) / kBlock)); }

}  // namespace
}  // namespace hfem

// ---------------------------------------------------------------- host side
namespace {
struct DevLevel {
    int32_t n = 0, bs = 2, n_agg = 0;
    int64_t a_nnz = 0, p_nnz = 0, ap_nnz = 0;
    int32_t *a_ptr = nullptr, *a_col = nullptr, *a_diag = nullptr;
    int32_t *agg = nullptr, *agg_ptr = nullptr, *agg_rows = nullptr, *p_ptr = nullptr, *p_col = nullptr;
    int32_t *r_ptr = nullptr, *r_col = nullptr, *r_pidx = nullptr, *ap_ptr = nullptr, *ap_col = nullptr;
    double *a_val = nullptr, *dinv = nullptr, *ns = nullptr, *tent = nullptr, *p_val = nullptr, *ap_val = nullptr;
    double *x0 = nullptr, *x1 = nullptr, *x2 = nullptr, *d = nullptr, *res = nullptr, *b = nullptr, *coef = nullptr;
};
}  // namespace

struct hfem_amg {
    int device = -1;
    bool phys = false;
    int32_t n_u = 0, npe = 3;              // npe: corners per element of the fine level's fan (3 TRI3, 4 QUAD4)
    int64_t conn_x_fixed = 0, conn_u_fixed = 0;   // corners that read a fixed x / u row (the hyper entry points' null checks)
    int32_t *fan_ptr = nullptr, *fan_elem = nullptr, *fan_corner = nullptr, *fan_slot = nullptr, *conn_x = nullptr,
            *conn_u = nullptr, *row_x = nullptr;
    std::vector<DevLevel> lv;
    int64_t n_coarse = 0;                  // dofs of the coarsest level
    const double *coarse_inv = nullptr;    // caller-owned N x N inverse (hfem_amg_set_coarse)
    double *part = nullptr;
    std::vector<void *> allocs;
    bool built = false, ready = false;     // hfem_amg_setup[_hyper] ran / and a coarse inverse is bound
};

namespace {
using hfem::kBlock;
using hfem::grid_of;

template <class T>
int upload(hfem_amg *a, T **dst, const std::vector<T> &src) {
    *dst = nullptr;
    const size_t bytes = std::max<size_t>(src.size(), 1) * sizeof(T);
    HFEM_HIP_CHECK(hipMalloc((void **)dst, bytes));
    a->allocs.push_back(*dst);
    if (!src.empty()) HFEM_HIP_CHECK(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

int alloc(hfem_amg *a, double **dst, int64_t count) {
    HFEM_HIP_CHECK(hipMalloc((void **)dst, (size_t)std::max<int64_t>(count, 1) * sizeof(double)));
    a->allocs.push_back(*dst);
    HFEM_HIP_CHECK(hipMemset(*dst, 0, (size_t)std::max<int64_t>(count, 1) * sizeof(double)));
    return 0;
}

void release(hfem_amg *a) {
    for (void *p : a->allocs) (void)hipFree(p);
    a->allocs.clear();
}

template <int BS>
void cheb(const DevLevel &L, const double *x_in, const double *b, double *x_out, double *r_out, int step, const double *st,
          hipStream_t s) {
    hipLaunchKernelGGL(hfem::amg_cheb_kernel<BS>, grid_of(L.n), dim3(kBlock), 0, s, L.n, L.a_ptr, L.a_col, L.a_val, L.dinv,
                       x_in, b, L.d, x_out, r_out, L.coef, step, st);
}

// xout = M_l b (recursive V-cycle from level l)
template <int BS>
void cycle_level(const hfem_amg *a, size_t l, const double *b, double *xout, const double *st, hipStream_t s);

void cycle(const hfem_amg *a, size_t l, const double *b, double *xout, const double *st, hipStream_t s) {
    if (l + 1 == a->lv.size()) {
        const int32_t N = (int32_t)a->n_coarse;
        hipLaunchKernelGGL(hfem::amg_coarse_gemv_kernel, dim3((unsigned)((N + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0, s,
                           N, a->coarse_inv, b, xout, st);
        return;
    }
    if (a->lv[l].bs == 2) cycle_level<2>(a, l, b, xout, st, s);
    else cycle_level<3>(a, l, b, xout, st, s);
}

template <int BS>
void cycle_level(const hfem_amg *a, size_t l, const double *b, double *xout, const double *st, hipStream_t s) {
    const DevLevel &L = a->lv[l], &C = a->lv[l + 1];
    cheb<BS>(L, nullptr, b, L.x1, nullptr, 0, st, s);           // pre-smoothing from 0
    cheb<BS>(L, L.x1, b, L.x2, nullptr, 1, st, s);
    cheb<BS>(L, L.x2, b, nullptr, L.res, 0, st, s);             // residual
    hipLaunchKernelGGL(hfem::amg_restrict_kernel<BS>, grid_of(C.n), dim3(kBlock), 0, s, C.n, L.r_ptr, L.r_col, L.r_pidx, L.p_val,
                       L.res, C.b, st);
    cycle(a, l + 1, C.b, C.x0, st, s);
    hipLaunchKernelGGL(hfem::amg_prolong_kernel<BS>, grid_of(L.n), dim3(kBlock), 0, s, L.n, L.p_ptr, L.p_col, L.p_val, C.x0, L.x2, st);
    cheb<BS>(L, L.x2, b, L.x1, nullptr, 0, st, s);              // post-smoothing: the same polynomial
    cheb<BS>(L, L.x1, b, xout, nullptr, 1, st, s);
}

template <int BS>
void setup_level(hfem_amg *a, size_t l, hipStream_t s) {
    DevLevel &L = a->lv[l];
    hipLaunchKernelGGL(hfem::amg_dinv_kernel<BS>, grid_of(L.n), dim3(kBlock), 0, s, L.n, L.a_diag, L.a_val, L.dinv);
    if (l + 1 == a->lv.size()) return;
    DevLevel &C = a->lv[l + 1];
    const int64_t m = (int64_t)L.n * BS;
    hipLaunchKernelGGL(hfem::amg_power_init_kernel, dim3(hfem::kRedBlocks), dim3(kBlock), 0, s, m, L.x1, a->part);
    hipLaunchKernelGGL(hfem::amg_power_finish_kernel, dim3(1), dim3(kBlock), 0, s, a->part, hfem::kRedBlocks, L.coef, 1);
    for (int it = 0; it < hfem::kAmgPowerIters; ++it) {
        double *v = (it & 1) ? L.x2 : L.x1, *w = (it & 1) ? L.x1 : L.x2;
        hipLaunchKernelGGL(hfem::amg_power_kernel<BS>, dim3(hfem::kRedBlocks), dim3(kBlock), 0, s, L.n, L.a_ptr, L.a_col, L.a_val,
                           L.dinv, v, w, L.coef, a->part);
        hipLaunchKernelGGL(hfem::amg_power_finish_kernel, dim3(1), dim3(kBlock), 0, s, a->part, hfem::kRedBlocks, L.coef, 0);
    }
    hipLaunchKernelGGL(hfem::amg_tentative_kernel<BS>, grid_of(L.n_agg), dim3(kBlock), 0, s, L.n_agg, L.agg_ptr, L.agg_rows, L.ns,
                       L.tent, C.ns);
    hipLaunchKernelGGL(hfem::amg_smooth_p_kernel<BS>, grid_of(L.n), dim3(kBlock), 0, s, L.n, L.a_ptr, L.a_col, L.a_val, L.dinv,
                       L.agg, L.tent, L.p_ptr, L.p_col, L.p_val, L.coef);
    hipLaunchKernelGGL(hfem::amg_ap_kernel<BS>, grid_of(L.n), dim3(kBlock), 0, s, L.n, L.a_ptr, L.a_col, L.a_val, L.p_ptr, L.p_col,
                       L.p_val, L.ap_ptr, L.ap_col, L.ap_val);
    hipLaunchKernelGGL(hfem::amg_rap_kernel<BS>, grid_of(C.n), dim3(kBlock), 0, s, C.n, L.r_ptr, L.r_col, L.r_pidx, L.p_val,
                       L.ap_ptr, L.ap_col, L.ap_val, C.a_ptr, C.a_col, C.a_val);
}

hfem::Tri3Consts consts(const double mat[4], double W) { return hfem::make_consts(mat, W, nullptr); }

// the coefficients of the shifted operator c_k K_ff + c_m M_ff (c_m includes the density)
struct Shift {
    double c_k, c_m;
    bool lumped;
};

// sh: the shifted operator, the Mass instance; w_elem (device, one weight per element by global id): K(w)_ff, the Scaled
// instance; neither: K_ff.  Never both (no entry point passes both).
void assemble(hfem_amg *a, const double *x_free, const double *x_fixed, const double mat[4], double W, const Shift *sh,
              const double *w_elem, hipStream_t s) {
    const DevLevel &L = a->lv[0];
    const bool quad = a->npe == 4;
    hfem::Tri3Consts k = consts(mat, quad ? 1.0 : W);        // QUAD4: the 2x2 rule's weights are 1, W is not read
    hfem::DynMass dm;
    if (sh) {
        k = hfem::scaled_consts(k, sh->c_k);
        dm = hfem::dyn_mass(quad, sh->c_m, sh->lumped);
    }
#define HFEM_AMG_ASM(NPE, PH, OP)                                                                                             \
    hipLaunchKernelGGL((hfem::amg_assemble_kernel<NPE, PH, hfem::ElemOp::OP>), grid_of(L.n), dim3(kBlock), 0, s, L.n,         \
                       a->fan_ptr, a->fan_elem, a->fan_corner, a->fan_slot, a->conn_x, (const double2 *)x_free,               \
                       (const double2 *)x_fixed, L.a_ptr, L.a_val, k, dm, w_elem)
#define HFEM_AMG_P(NPE, PH)                                                                                                   \
    do {                                                                                                                      \
        if (sh) HFEM_AMG_ASM(NPE, PH, Mass);                                                                                  \
        else if (w_elem) HFEM_AMG_ASM(NPE, PH, Scaled);                                                                       \
        else HFEM_AMG_ASM(NPE, PH, Plain);                                                                                    \
    } while (0)
    if (quad && a->phys) HFEM_AMG_P(4, true);
    else if (quad) HFEM_AMG_P(4, false);
    else if (a->phys) HFEM_AMG_P(3, true);
    else HFEM_AMG_P(3, false);
#undef HFEM_AMG_P
#undef HFEM_AMG_ASM
}

void assemble_hyper(hfem_amg *a, const double *x_free, const double *x_fixed, const double *u_free, const double *u_fixed,
                    const double lame[2], double W, hipStream_t s) {
    const DevLevel &L = a->lv[0];
#define HFEM_AMG_ASM_HYPER(NPE)                                                                                               \
    hipLaunchKernelGGL((hfem::amg_assemble_hyper_kernel<NPE>), grid_of(L.n), dim3(kBlock), 0, s, L.n, a->fan_ptr, a->fan_elem, \
                       a->fan_corner, a->fan_slot, a->conn_x, a->conn_u, (const double2 *)x_free, (const double2 *)x_fixed,    \
                       (const double2 *)u_free, (const double2 *)u_fixed, L.a_ptr, L.a_val, lame[0], lame[1], W)
    if (a->npe == 4) HFEM_AMG_ASM_HYPER(4);                   // QUAD4: the 2x2 rule's weights are 1, W is not read
    else HFEM_AMG_ASM_HYPER(3);
#undef HFEM_AMG_ASM_HYPER
}

// the numeric hierarchy on the fine level's assembled values and near-null space, and the dense coarsest matrix
int setup_levels(hfem_amg *a, double *coarse_out, hipStream_t s, const char *what) {
    for (size_t l = 0; l < a->lv.size(); ++l) {
        if (a->lv[l].bs == 2) setup_level<2>(a, l, s);
        else setup_level<3>(a, l, s);
    }
    const DevLevel &Lc = a->lv.back();
    HFEM_HIP_CHECK(hipMemsetAsync(coarse_out, 0, (size_t)a->n_coarse * a->n_coarse * sizeof(double), s));
    if (Lc.bs == 2)
        hipLaunchKernelGGL(hfem::amg_coarse_scatter_kernel<2>, grid_of(Lc.n), dim3(kBlock), 0, s, Lc.n, Lc.a_ptr, Lc.a_col,
                           Lc.a_val, coarse_out);
    else
        hipLaunchKernelGGL(hfem::amg_coarse_scatter_kernel<3>, grid_of(Lc.n), dim3(kBlock), 0, s, Lc.n, Lc.a_ptr, Lc.a_col,
                           Lc.a_val, coarse_out);
    if (int rc = hfem::launch_status(what)) return rc;
    a->built = true;
    return 0;
}

int create(hfem_amg *a, const hfem_amg_host *h) {
    if (upload(a, &a->fan_ptr, h->fan_ptr) || upload(a, &a->fan_elem, h->fan_elem) || upload(a, &a->fan_corner, h->fan_corner) ||
        upload(a, &a->fan_slot, h->fan_slot) || upload(a, &a->conn_x, h->conn_x) || upload(a, &a->conn_u, h->conn_u) ||
        upload(a, &a->row_x, h->row_x))
        return -1;
    a->lv.resize(h->levels.size());
    for (size_t l = 0; l < h->levels.size(); ++l) {
        const hfem::AmgLevel &H = h->levels[l];
        DevLevel &L = a->lv[l];
        const int64_t bs = H.bs, m = (int64_t)H.n * bs;
        L.n = H.n; L.bs = H.bs; L.n_agg = H.n_agg;
        L.a_nnz = (int64_t)H.a_col.size(); L.p_nnz = (int64_t)H.p_col.size(); L.ap_nnz = (int64_t)H.ap_col.size();
        if (upload(a, &L.a_ptr, H.a_ptr) || upload(a, &L.a_col, H.a_col) || upload(a, &L.a_diag, H.a_diag) ||
            alloc(a, &L.a_val, L.a_nnz * bs * bs) || alloc(a, &L.dinv, m * bs) || alloc(a, &L.coef, hfem::kCoefN) ||
            alloc(a, &L.x0, m) || alloc(a, &L.x1, m) || alloc(a, &L.x2, m) || alloc(a, &L.d, m) || alloc(a, &L.res, m) ||
            alloc(a, &L.b, m) || alloc(a, &L.ns, m * 3))
            return -1;
        if (l + 1 < h->levels.size() &&
            (upload(a, &L.agg, H.agg) || upload(a, &L.agg_ptr, H.agg_ptr) || upload(a, &L.agg_rows, H.agg_rows) ||
             upload(a, &L.p_ptr, H.p_ptr) || upload(a, &L.p_col, H.p_col) || upload(a, &L.r_ptr, H.r_ptr) ||
             upload(a, &L.r_col, H.r_col) || upload(a, &L.r_pidx, H.r_pidx) || upload(a, &L.ap_ptr, H.ap_ptr) ||
             upload(a, &L.ap_col, H.ap_col) || alloc(a, &L.tent, m * 3) || alloc(a, &L.p_val, L.p_nnz * bs * 3) ||
             alloc(a, &L.ap_val, L.ap_nnz * bs * 3)))
            return -1;
    }
    a->n_coarse = (int64_t)a->lv.back().n * a->lv.back().bs;
    return alloc(a, &a->part, hfem::kRedBlocks);
}
}  // namespace

namespace hfem {
void amg_cycle(const hfem_amg *a, const double *r, double *z, const double *st, void *s) {
    cycle(a, 0, r, z, st, (hipStream_t)s);
}
int64_t amg_rows(const hfem_amg *a) { return a->n_u; }
int amg_device(const hfem_amg *a) { return a->device; }
bool amg_ready(const hfem_amg *a) { return a->ready; }
}  // namespace hfem

extern "C" int hfem_amg_create(int device, const hfem_amg_host *host, int32_t flags, hfem_amg **out) {
    HFEM_ARG_CHECK(host && out, "null pointer");
    *out = nullptr;
    HFEM_ARG_CHECK(device >= 0, "device must be >= 0");
    HFEM_ARG_CHECK((flags & ~HFEM_FLAG_PHYSICAL_GRAD) == 0, "flags: only HFEM_FLAG_PHYSICAL_GRAD");
    HFEM_ARG_CHECK(!host->levels.empty(), "empty hierarchy");
    HFEM_ARG_CHECK(host->levels.back().n * (int64_t)host->levels.back().bs <= 8 * hfem::kAmgMaxCoarseDofs,
                   "the coarsest level is too large for a dense solve (the mesh graph does not coarsen)");
    if (int rc = hfem::use_device(device)) return rc;
    std::unique_ptr<hfem_amg> a(new hfem_amg);
    a->device = device; a->phys = (flags & HFEM_FLAG_PHYSICAL_GRAD) != 0; a->n_u = host->n_u; a->npe = host->npe;
    for (int32_t c : host->conn_x) a->conn_x_fixed += c < 0;
    for (int32_t c : host->conn_u) a->conn_u_fixed += c < 0;
    if (create(a.get(), host)) {
        release(a.get());
        return -1;
    }
    *out = a.release();
    return 0;
}

extern "C" int hfem_amg_destroy(hfem_amg *a) {
    if (!a) return 0;
    if (a->device >= 0) (void)hipSetDevice(a->device);
    release(a);
    delete a;
    return 0;
}

extern "C" int hfem_amg_assemble(hfem_amg *a, const double *x_free, const double *x_fixed, const double mat[4], double W,
                                 void *stream) {
    HFEM_ARG_CHECK(a && x_free && mat, "null pointer");
    if (int rc = hfem::use_device(a->device)) return rc;
    assemble(a, x_free, x_fixed, mat, W, nullptr, nullptr, (hipStream_t)stream);
    return hfem::launch_status("hfem_amg_assemble");
}

extern "C" int hfem_amg_setup(hfem_amg *a, const double *x_free, const double *x_fixed, const double mat[4], double W,
                              double *coarse_out, void *stream) {
    HFEM_ARG_CHECK(a && x_free && mat && coarse_out, "null pointer");
    if (int rc = hfem::use_device(a->device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    assemble(a, x_free, x_fixed, mat, W, nullptr, nullptr, s);
    hipLaunchKernelGGL(hfem::amg_ns0_kernel, grid_of(a->n_u), dim3(kBlock), 0, s, a->n_u, a->row_x, (const double2 *)x_free,
                       (const double2 *)x_fixed, (const double2 *)nullptr, a->lv[0].ns);
    return setup_levels(a, coarse_out, s, "hfem_amg_setup");
}

static int check_shift(const char *who, double c_k, double c_m) {
    if (!(std::isfinite(c_k) && std::isfinite(c_m) && c_k >= 0.0 && c_m >= 0.0 && (c_k > 0.0 || c_m > 0.0))) {
        hfem::set_error(std::string(who) + ": c_k and c_m must be finite, >= 0 and not both zero");
        return -1;
    }
    return 0;
}

extern "C" int hfem_amg_assemble_shifted(hfem_amg *a, const double *x_free, const double *x_fixed, const double mat[4], double W,
                                         double c_k, double c_m, int32_t lumped, void *stream) {
    if (int rc = check_shift(__func__, c_k, c_m)) return rc;
    HFEM_ARG_CHECK(a && x_free && mat, "null pointer");
    HFEM_ARG_CHECK(a->conn_x_fixed == 0 || x_fixed, "the mesh has fixed coordinate rows: x_fixed must be given");
    if (int rc = hfem::use_device(a->device)) return rc;
    const Shift sh{c_k, c_m, lumped != 0};
    assemble(a, x_free, x_fixed, mat, W, &sh, nullptr, (hipStream_t)stream);
    return hfem::launch_status("hfem_amg_assemble_shifted");
}

extern "C" int hfem_amg_setup_shifted(hfem_amg *a, const double *x_free, const double *x_fixed, const double mat[4], double W,
                                      double c_k, double c_m, int32_t lumped, double *coarse_out, void *stream) {
    if (int rc = check_shift(__func__, c_k, c_m)) return rc;
    HFEM_ARG_CHECK(a && x_free && mat && coarse_out, "null pointer");
    HFEM_ARG_CHECK(a->conn_x_fixed == 0 || x_fixed, "the mesh has fixed coordinate rows: x_fixed must be given");
    if (int rc = hfem::use_device(a->device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const Shift sh{c_k, c_m, lumped != 0};
    assemble(a, x_free, x_fixed, mat, W, &sh, nullptr, s);
    hipLaunchKernelGGL(hfem::amg_ns0_kernel, grid_of(a->n_u), dim3(kBlock), 0, s, a->n_u, a->row_x, (const double2 *)x_free,
                       (const double2 *)x_fixed, (const double2 *)nullptr, a->lv[0].ns);
    return setup_levels(a, coarse_out, s, "hfem_amg_setup_shifted");
}

// The pair on K(w) = sum_e w_e K_e: the hierarchy's patterns and aggregates are the mesh's; only the values are rebuilt.
extern "C" int hfem_amg_assemble_scaled(hfem_amg *a, const double *x_free, const double *x_fixed, const double mat[4], double W,
                                        const double *w_elem, void *stream) {
    HFEM_ARG_CHECK(a && x_free && mat, "null pointer");
    HFEM_ARG_CHECK(w_elem, "w_elem must be given (one weight per element)");
    HFEM_ARG_CHECK(a->conn_x_fixed == 0 || x_fixed, "the mesh has fixed coordinate rows: x_fixed must be given");
    if (int rc = hfem::use_device(a->device)) return rc;
    assemble(a, x_free, x_fixed, mat, W, nullptr, w_elem, (hipStream_t)stream);
    return hfem::launch_status("hfem_amg_assemble_scaled");
}

extern "C" int hfem_amg_setup_scaled(hfem_amg *a, const double *x_free, const double *x_fixed, const double mat[4], double W,
                                     const double *w_elem, double *coarse_out, void *stream) {
    HFEM_ARG_CHECK(a && x_free && mat && coarse_out, "null pointer");
    HFEM_ARG_CHECK(w_elem, "w_elem must be given (one weight per element)");
    HFEM_ARG_CHECK(a->conn_x_fixed == 0 || x_fixed, "the mesh has fixed coordinate rows: x_fixed must be given");
    if (int rc = hfem::use_device(a->device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    assemble(a, x_free, x_fixed, mat, W, nullptr, w_elem, s);
    hipLaunchKernelGGL(hfem::amg_ns0_kernel, grid_of(a->n_u), dim3(kBlock), 0, s, a->n_u, a->row_x, (const double2 *)x_free,
                       (const double2 *)x_fixed, (const double2 *)nullptr, a->lv[0].ns);
    return setup_levels(a, coarse_out, s, "hfem_amg_setup_scaled");
}

extern "C" int hfem_amg_assemble_hyper(hfem_amg *a, const double *x_free, const double *x_fixed, const double *u_free,
                                       const double *u_fixed, const double lame[2], double W, void *stream) {
    HFEM_ARG_CHECK(a && x_free && u_free && lame, "null pointer");
    HFEM_ARG_CHECK(a->conn_u_fixed == 0 || u_fixed, "the mesh has Dirichlet rows: u_fixed must be given");
    HFEM_ARG_CHECK(a->conn_x_fixed == 0 || x_fixed, "the mesh has fixed coordinate rows: x_fixed must be given");
    if (int rc = hfem::use_device(a->device)) return rc;
    assemble_hyper(a, x_free, x_fixed, u_free, u_fixed, lame, W, (hipStream_t)stream);
    return hfem::launch_status("hfem_amg_assemble_hyper");
}

extern "C" int hfem_amg_setup_hyper(hfem_amg *a, const double *x_free, const double *x_fixed, const double *u_free,
                                    const double *u_fixed, const double lame[2], double W, double *coarse_out, void *stream) {
    HFEM_ARG_CHECK(a && x_free && u_free && lame && coarse_out, "null pointer");
    HFEM_ARG_CHECK(a->conn_u_fixed == 0 || u_fixed, "the mesh has Dirichlet rows: u_fixed must be given");
    HFEM_ARG_CHECK(a->conn_x_fixed == 0 || x_fixed, "the mesh has fixed coordinate rows: x_fixed must be given");
    if (int rc = hfem::use_device(a->device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    assemble_hyper(a, x_free, x_fixed, u_free, u_fixed, lame, W, s);
    hipLaunchKernelGGL(hfem::amg_ns0_kernel, grid_of(a->n_u), dim3(kBlock), 0, s, a->n_u, a->row_x, (const double2 *)x_free,
                       (const double2 *)x_fixed, (const double2 *)u_free, a->lv[0].ns);
    return setup_levels(a, coarse_out, s, "hfem_amg_setup_hyper");
}

extern "C" int hfem_amg_set_coarse(hfem_amg *a, const double *coarse_inv) {
    HFEM_ARG_CHECK(a && coarse_inv, "null pointer");
    HFEM_ARG_CHECK(a->built, "hfem_amg_setup has not run");
    a->coarse_inv = coarse_inv;
    a->ready = true;
    return 0;
}

extern "C" int hfem_amg_vcycle(hfem_amg *a, const double *r, double *z, void *stream) {
    HFEM_ARG_CHECK(a && r && z, "null pointer");
    HFEM_ARG_CHECK(a->ready, "hfem_amg_setup / hfem_amg_set_coarse have not run");
    HFEM_ARG_CHECK(r != z, "r and z must differ");
    if (int rc = hfem::use_device(a->device)) return rc;
    hfem::amg_cycle(a, r, z, nullptr, stream);
    return hfem::launch_status("hfem_amg_vcycle");
}

extern "C" int hfem_amg_values(hfem_amg *a, int32_t level, int32_t which, double *out, int64_t *n_out, void *stream) {
    HFEM_ARG_CHECK(a && n_out, "null pointer");
    HFEM_ARG_CHECK(level >= 0 && level < (int32_t)a->lv.size(), "level out of range");
    const DevLevel &L = a->lv[level];
    const bool last = level + 1 == (int32_t)a->lv.size();
    const int64_t bs = L.bs;
    const double *src = nullptr;
    int64_t n = 0;
    switch (which) {
        case 0: src = L.a_val; n = L.a_nnz * bs * bs; break;
        case 1: src = L.dinv; n = (int64_t)L.n * bs * bs; break;
        case 2: src = L.coef; n = hfem::kCoefN; break;
        case 3: src = L.ns; n = (int64_t)L.n * bs * 3; break;
        case 4: src = last ? nullptr : L.tent; n = last ? 0 : (int64_t)L.n * bs * 3; break;
        case 5: src = last ? nullptr : L.p_val; n = last ? 0 : L.p_nnz * bs * 3; break;
        default: HFEM_ARG_CHECK(false, "which out of range");
    }
    *n_out = n;
    if (out && n) {
        if (int rc = hfem::use_device(a->device)) return rc;
        HFEM_HIP_CHECK(hipMemcpyAsync(out, src, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    }
    return 0;
}
