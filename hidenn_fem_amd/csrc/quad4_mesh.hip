// Mesh validity for r-adaptivity on QUAD4, gfx950 (MI355X): the bilinear-cell twins of tri3_mesh.hip -- element measure, the
// inversion-safe step bound and the opt-in quality barrier (hidenn_fem_amd/radapt.py, Quad4RAdaptiveSolver).
//
// One thread per element over the int32 connectivity [ne][4] (caller numbering, local nodes counter-clockwise as in
// hfem_quad4_dev.h: xi_k = {-1,1,1,-1}, eta_k = {-1,-1,1,1}); corner rows through the x row map (x_src[n] >= 0: x_free row,
// < 0: x_fixed row -1 - x_src[n]), so any storage row order works.  Rows are fp64 or fp32 (T); all arithmetic is fp64.
// Neighbour indices are mod 4.  With the edge vectors e_k = X_{k+1} - X_k, the corner cross product is
//   c_k = (X_{k+1} - X_k) x (X_{k-1} - X_k) = e_{k-1} x e_k,         detJ at corner k = c_k / 4.
// detJ(xi, eta) of a bilinear cell is affine in (xi, eta) (the xi eta terms of x_xi y_eta and x_eta y_xi cancel), so inside
// the cell it is the bilinear interpolant of the four corner values: the cell is valid everywhere iff all four s c_k > 0,
// and if every c_k keeps a share eta of its value, so does detJ at every Gauss point.
// s = sign of c_0 + c_2 (twice the signed area) on the reference rows x_ref (the model's initial coordinates), so a
// clockwise-numbered mesh measures like its counter-clockwise copy.
//   q_k = 2 s c_k / (|e_{k-1}|^2 + |e_k|^2)   (1 at a right-angled corner with equal sides),   q = min_k q_k
//   quad4_mesh_measure_kernel    q and min_k c_k / c_k_ref per element (optional outputs); min q, min ratio and the count of
//                                inverted elements (some s c_k <= 0) by monotone-key atomic min / integer atomic add, then a
//                                one-thread finish that turns the keys into doubles.  Order-independent: deterministic.
//   quad4_step_bound_kernel      c_k(x + a d) = A0 + A1 a + A2 a^2 exactly, per corner; the smallest a > 0 at which some
//                                corner has c_k(a) = eta c_k(0) (+inf if none), min over the elements by a 64-bit atomic min
//                                on the bit pattern of the non-negative double.  Deterministic, capturable (no host sync).
//   quad4_quality_barrier_kernel Q = (w / (4 Ne)) sum_e sum_k (1/q_ek - 1) and its gradient w.r.t. the free rows,
//                                ACCUMULATED with fp64 atomics (not deterministic in the last bits).
// Shared with tri3_mesh.hip (hfem_mesh_dev.h): the row access, the keys, the reductions, first_crossing(), the one-thread
// init launch before each reduction (the sentinel) and the filtered atomics.
// Gather-bound: per element 16 B of connectivity, four x_src words and four (measure, barrier: eight) coordinate rows; no
// LDS beyond the reduction words, no per-thread array that survives unrolling (no scratch).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "hfem_mesh_dev.h"

namespace hfem {
namespace {

__device__ __forceinline__ double cross2(const double2 p, const double2 r) { return p.x * r.y - p.y * r.x; }
__device__ __forceinline__ double2 sub2(const double2 p, const double2 r) { return make_double2(p.x - r.x, p.y - r.y); }
__device__ __forceinline__ double norm_sq(const double2 p) { return p.x * p.x + p.y * p.y; }

// e_k = X_{k+1} - X_k
__device__ __forceinline__ void edges4(const double2 (&X)[4], double2 (&E)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) E[k] = sub2(X[(k + 1) & 3], X[k]);
}

template <typename T>
__device__ __forceinline__ void load_corners(const int32_t *__restrict__ conn, const int32_t *__restrict__ x_src, int64_t e,
                                             const typename MeshRow<T>::type *__restrict__ x_free,
                                             const typename MeshRow<T>::type *__restrict__ x_fixed, int32_t (&n)[4],
                                             int32_t (&src)[4], double2 (&X)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) n[k] = conn[4 * e + k];          // dword loads: the caller's pointer need not be 16-byte aligned
#pragma unroll
    for (int k = 0; k < 4; ++k) src[k] = x_src[n[k]];
#pragma unroll
    for (int k = 0; k < 4; ++k) X[k] = corner<T>(x_free, x_fixed, src[k]);
}

// s and the four reference cross products of an element
template <typename T>
__device__ __forceinline__ double reference_corners(const typename MeshRow<T>::type *__restrict__ x_ref, const int32_t (&n)[4],
                                                    double (&cref)[4]) {
    double2 R[4], ER[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const typename MeshRow<T>::type r = x_ref[n[k]];
        R[k] = make_double2((double)r.x, (double)r.y);
    }
    edges4(R, ER);
#pragma unroll
    for (int k = 0; k < 4; ++k) cref[k] = cross2(ER[(k + 3) & 3], ER[k]);
    return sign_of(cref[0] + cref[2]);
}

template <typename T>
__global__ __launch_bounds__(kMeshBlock) void quad4_mesh_measure_kernel(
    int64_t ne, const int32_t *__restrict__ conn, const int32_t *__restrict__ x_src,
    const typename MeshRow<T>::type *__restrict__ x_free, const typename MeshRow<T>::type *__restrict__ x_fixed,
    const typename MeshRow<T>::type *__restrict__ x_ref, double *__restrict__ q_out, double *__restrict__ ratio_out,
    unsigned long long *summary) {
    __shared__ unsigned long long red[kMeshBlock / 64];
    const int64_t e = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    unsigned long long kq = ~0ull, kr = ~0ull;
    unsigned inv = 0;
    if (e < ne) {
        int32_t n[4], src[4];
        double2 X[4], E[4];
        double cref[4];
        load_corners<T>(conn, x_src, e, x_free, x_fixed, n, src, X);
        const double s = reference_corners<T>(x_ref, n, cref);
        edges4(X, E);
        double q = INFINITY, ratio = INFINITY;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double2 p = E[(k + 3) & 3], r = E[k];
            const double c = cross2(p, r);
            const double qk = 2.0 * s * c / (norm_sq(p) + norm_sq(r)), rk = c / cref[k];
            q = (qk < q || qk != qk) ? qk : q;          // a NaN corner makes the element's value NaN, and it stays NaN
            ratio = (rk < ratio || rk != rk) ? rk : ratio;
            inv |= !(s * c > 0.0);
        }
        if (q_out) q_out[e] = q;
        if (ratio_out) ratio_out[e] = ratio;
        kq = dkey(q);
        kr = dkey(ratio);
    }
    mesh_measure_reduce(kq, kr, inv, red, summary);
}

// ---------------------------------------------------------------- step bound (closed form: first_crossing, hfem_mesh_dev.h)
template <typename T>
__global__ __launch_bounds__(kMeshBlock) void quad4_step_bound_kernel(
    int64_t ne, const int32_t *__restrict__ conn, const int32_t *__restrict__ x_src,
    const typename MeshRow<T>::type *__restrict__ x_free, const typename MeshRow<T>::type *__restrict__ x_fixed,
    const double2 *__restrict__ d, double eta, double *alpha) {
    __shared__ unsigned long long red[kMeshBlock / 64];
    const int64_t e = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    double a = INFINITY;
    if (e < ne) {
        int32_t n[4], src[4];
        double2 X[4], D[4], E[4], DE[4];
        load_corners<T>(conn, x_src, e, x_free, x_fixed, n, src, X);
#pragma unroll
        for (int k = 0; k < 4; ++k) D[k] = src[k] >= 0 ? d[src[k]] : make_double2(0.0, 0.0);
        edges4(X, E);
        edges4(D, DE);
        // c_k(x + a d) = (e_{k-1} + a de_{k-1}) x (e_k + a de_k)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double2 p = E[(k + 3) & 3], r = E[k], dp = DE[(k + 3) & 3], dr = DE[k];
            const double ak = first_crossing(cross2(p, r), cross2(p, dr) + cross2(dp, r), cross2(dp, dr), eta);
            a = ak < a ? ak : a;
        }
    }
    // a >= 0 (or +inf; a NaN corner from non-finite rows loses every comparison above): the u64 order of the bits is numeric
    const unsigned long long k = block_min_u64((unsigned long long)__double_as_longlong(a), red);
    if (threadIdx.x == 0) atomic_min_filtered(reinterpret_cast<unsigned long long *>(alpha), k);
}

// ---------------------------------------------------------------- quality barrier
// Per corner k, with p = e_{k-1} = X_k - X_{k-1}, r = e_k = X_{k+1} - X_k:  c = p x r, S = |p|^2 + |r|^2,
//   1/q_k = S / (2 s c):   d(1/q_k) = (dS c - S dc) / (2 s c^2) = f1 dS + f2 dc,   f1 = 1 / (2 s c),  f2 = -S / (2 s c^2)
//   dS/dp = 2 p, dS/dr = 2 r,   dc/dp = (r_y, -r_x),  dc/dr = (-p_y, p_x)
//   G_p = f1 2 p + f2 (r_y, -r_x),  G_r = f1 2 r + f2 (-p_y, p_x):   dX_{k-1} -= G_p,  dX_k += G_p - G_r,  dX_{k+1} += G_r.
// The four corners' parts are summed per node in registers: eight atomics per element.  Finite for valid elements only (the
// solver keeps every element valid).
template <typename T>
__global__ __launch_bounds__(kMeshBlock) void quad4_quality_barrier_kernel(
    int64_t ne, const int32_t *__restrict__ conn, const int32_t *__restrict__ x_src,
    const typename MeshRow<T>::type *__restrict__ x_free, const typename MeshRow<T>::type *__restrict__ x_fixed,
    const typename MeshRow<T>::type *__restrict__ x_ref, double wscale, double *value, double *grad) {
    __shared__ double red[kMeshBlock / 64];
    const int64_t e = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    double v = 0.0;
    if (e < ne) {
        int32_t n[4], src[4];
        double2 X[4], E[4];
        double cref[4];
        load_corners<T>(conn, x_src, e, x_free, x_fixed, n, src, X);
        const double s = reference_corners<T>(x_ref, n, cref);
        edges4(X, E);
        double2 g[4] = {make_double2(0.0, 0.0), make_double2(0.0, 0.0), make_double2(0.0, 0.0), make_double2(0.0, 0.0)};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int km = (k + 3) & 3, kp = (k + 1) & 3;
            const double2 p = E[km], r = E[k];
            const double c = cross2(p, r), S = norm_sq(p) + norm_sq(r);
            const double den = 2.0 * s * c;
            v += wscale * (S / den - 1.0);
            if (grad) {
                const double f1 = 2.0 * wscale / den, f2 = -wscale * S / (den * c);
                const double2 Gp = make_double2(f1 * p.x + f2 * r.y, f1 * p.y - f2 * r.x);
                const double2 Gr = make_double2(f1 * r.x - f2 * p.y, f1 * r.y + f2 * p.x);
                g[km].x -= Gp.x; g[km].y -= Gp.y;
                g[k].x += Gp.x - Gr.x; g[k].y += Gp.y - Gr.y;
                g[kp].x += Gr.x; g[kp].y += Gr.y;
            }
        }
        if (grad) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (src[k] >= 0) {
                    __hip_atomic_fetch_add(grad + 2 * (int64_t)src[k], g[k].x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_fetch_add(grad + 2 * (int64_t)src[k] + 1, g[k].y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
        }
    }
    const double tot = block_sum(v, red);
    if (threadIdx.x == 0 && value) __hip_atomic_fetch_add(value, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <typename T>
int quad4_mesh_measure(int device, const int32_t *conn, int64_t ne, const int32_t *x_src, const T *x_free, const T *x_fixed,
                       const T *x_ref, double *q_out, double *ratio_out, double *summary_out, void *stream) {
    HFEM_ARG_CHECK(summary_out && x_free, "null pointer");
    HFEM_ARG_CHECK(ne >= 0 && ne < ((int64_t)1 << 31), "ne must be in [0, 2^31)");
    HFEM_ARG_CHECK(ne == 0 || (conn && x_src && x_ref), "null pointer");
    if (int rc = use_device(device)) return rc;
    typedef typename MeshRow<T>::type R;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *sm = reinterpret_cast<unsigned long long *>(summary_out);
    hipLaunchKernelGGL(mesh_measure_init_kernel, dim3(1), dim3(1), 0, s, sm);
    if (ne > 0)
        hipLaunchKernelGGL(quad4_mesh_measure_kernel<T>, dim3(mesh_blocks(ne)), dim3(kMeshBlock), 0, s, ne, conn, x_src,
                           (const R *)x_free, (const R *)x_fixed, (const R *)x_ref, q_out, ratio_out, sm);
    hipLaunchKernelGGL(mesh_measure_finish_kernel, dim3(1), dim3(1), 0, s, sm);
    return launch_status("hfem_quad4_mesh_measure");
}

template <typename T>
int quad4_step_bound(int device, const int32_t *conn, int64_t ne, const int32_t *x_src, const T *x_free, const T *x_fixed,
                     const double *d, double eta, double *alpha_out, void *stream) {
    HFEM_ARG_CHECK(alpha_out && x_free && d, "null pointer");
    HFEM_ARG_CHECK(ne >= 0 && ne < ((int64_t)1 << 31), "ne must be in [0, 2^31)");
    HFEM_ARG_CHECK(ne == 0 || (conn && x_src), "null pointer");
    HFEM_ARG_CHECK(eta > 0.0 && eta < 1.0, "eta must be in (0, 1)");
    if (int rc = use_device(device)) return rc;
    typedef typename MeshRow<T>::type R;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(step_bound_init_kernel, dim3(1), dim3(1), 0, s, alpha_out);
    if (ne > 0)
        hipLaunchKernelGGL(quad4_step_bound_kernel<T>, dim3(mesh_blocks(ne)), dim3(kMeshBlock), 0, s, ne, conn, x_src,
                           (const R *)x_free, (const R *)x_fixed, (const double2 *)d, eta, alpha_out);
    return launch_status("hfem_quad4_step_bound");
}

template <typename T>
int quad4_quality_barrier(int device, const int32_t *conn, int64_t ne, const int32_t *x_src, const T *x_free,
                          const T *x_fixed, const T *x_ref, double weight, double *value_acc, double *grad_acc, void *stream) {
    HFEM_ARG_CHECK(x_free && (value_acc || grad_acc), "null pointer");
    HFEM_ARG_CHECK(ne >= 0 && ne < ((int64_t)1 << 31), "ne must be in [0, 2^31)");
    HFEM_ARG_CHECK(ne == 0 || (conn && x_src && x_ref), "null pointer");
    HFEM_ARG_CHECK(weight >= 0.0 && std::isfinite(weight), "weight must be finite and >= 0");
    if (ne == 0) return 0;
    if (int rc = use_device(device)) return rc;
    typedef typename MeshRow<T>::type R;
    hipLaunchKernelGGL(quad4_quality_barrier_kernel<T>, dim3(mesh_blocks(ne)), dim3(kMeshBlock), 0, (hipStream_t)stream, ne,
                       conn, x_src, (const R *)x_free, (const R *)x_fixed, (const R *)x_ref, weight / (4.0 * (double)ne),
                       value_acc, grad_acc);
    return launch_status("hfem_quad4_quality_barrier");
}

}  // namespace
}  // namespace hfem

#define HFEM_QUAD4_MESH_ABI(SUFFIX, T)                                                                                        \
    extern "C" int hfem_quad4_mesh_measure##SUFFIX(int device, const int32_t *conn, int64_t ne, const int32_t *x_src,          \
                                                   const T *x_free, const T *x_fixed, const T *x_ref, double *q_out,            \
                                                   double *ratio_out, double *summary_out, void *stream) {                      \
        return hfem::quad4_mesh_measure<T>(device, conn, ne, x_src, x_free, x_fixed, x_ref, q_out, ratio_out, summary_out,     \
                                           stream);                                                                            \
    }                                                                                                                          \
    extern "C" int hfem_quad4_step_bound##SUFFIX(int device, const int32_t *conn, int64_t ne, const int32_t *x_src,            \
                                                 const T *x_free, const T *x_fixed, const double *d, double eta,               \
                                                 double *alpha_out, void *stream) {                                            \
        return hfem::quad4_step_bound<T>(device, conn, ne, x_src, x_free, x_fixed, d, eta, alpha_out, stream);                 \
    }                                                                                                                          \
    extern "C" int hfem_quad4_quality_barrier##SUFFIX(int device, const int32_t *conn, int64_t ne, const int32_t *x_src,       \
                                                      const T *x_free, const T *x_fixed, const T *x_ref, double weight,        \
                                                      double *value_acc, double *grad_acc, void *stream) {                     \
        return hfem::quad4_quality_barrier<T>(device, conn, ne, x_src, x_free, x_fixed, x_ref, weight, value_acc, grad_acc,    \
                                              stream);                                                                         \
    }

HFEM_QUAD4_MESH_ABI(, double)
HFEM_QUAD4_MESH_ABI(_f32, float)
#undef HFEM_QUAD4_MESH_ABI
