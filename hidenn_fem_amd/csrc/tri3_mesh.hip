// Mesh validity for r-adaptivity on TRI3, gfx950 (MI355X): element measure, the inversion-safe step bound and the opt-in
// quality barrier (hidenn_fem_amd/radapt.py).  No reference counterpart: the reference's example 4 moves the nodes with
// L-BFGS and nothing keeps an element from turning inside out (its alternating-scheme sketch calls a mesh_quality_loss it
// never defines).
//
// One thread per element over the int32 connectivity (caller numbering); corner rows come through the x row map
// (x_src[n] >= 0: x_free row, < 0: x_fixed row -1 - x_src[n]), so any storage row order works.  Rows are fp64 or fp32 (T);
// all arithmetic is fp64.  With J = [[x0-x2, x1-x2], [y0-y2, y1-y2]] (src/models.py:336-343):
//   detJ = (x0-x2)(y1-y2) - (x1-x2)(y0-y2)    (= 2 x the signed area, either gradient convention)
//   q    = 2 sqrt(3) s detJ / (|e1|^2 + |e2|^2 + |e3|^2)   (= 4 sqrt(3) s A / sum |e|^2; 1 for an equilateral triangle)
// s = sign of detJ on the reference rows x_ref (the model's initial coordinates), so q is in (0, 1] for a valid element and
// <= 0 for an inverted one, whatever the orientation of the mesh.
//   tri3_mesh_measure_kernel   q and detJ / detJ_ref per element (optional outputs); min q, min ratio and the count of
//                              inverted elements (s detJ <= 0) by monotone-key atomic min / integer atomic add, then a
//                              one-thread finish that turns the keys into doubles.  Order-independent: deterministic.
//   tri3_step_bound_kernel     detJ(x + a d) = A0 + A1 a + A2 a^2 exactly; the smallest a > 0 with detJ(a) = eta detJ(0)
//                              (+inf if none), min over the elements by a 64-bit atomic min on the bit pattern of the
//                              non-negative double (monotone).  Deterministic, capturable (no host sync).
//   tri3_quality_barrier_kernel  Q = (w / Ne) sum (1/q - 1) and its gradient w.r.t. the free rows, ACCUMULATED with fp64
//                              atomics (not deterministic in the last bits).
// The row access, the keys, the reductions and first_crossing() are shared with quad4_mesh.hip (hfem_mesh_dev.h).
// Each launch that reduces into a caller scalar is preceded by a one-thread init launch on the same stream (the sentinel).
// Atomic filters: a workgroup reads the running minimum first and only issues its atomic when it improves on it, so the
// single-address atomics do not serialise the tail of a launch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "hfem_mesh_dev.h"

namespace hfem {
namespace {

constexpr double kTwoSqrt3 = 3.4641016151377545870548926830117;   // 2 sqrt(3)

__device__ __forceinline__ double det3(const double2 X0, const double2 X1, const double2 X2) {
    return (X0.x - X2.x) * (X1.y - X2.y) - (X1.x - X2.x) * (X0.y - X2.y);
}

__device__ __forceinline__ double edge_sq_sum(const double2 X0, const double2 X1, const double2 X2) {
    const double ax = X1.x - X0.x, ay = X1.y - X0.y, bx = X2.x - X1.x, by = X2.y - X1.y, cx = X0.x - X2.x, cy = X0.y - X2.y;
    return ax * ax + ay * ay + bx * bx + by * by + cx * cx + cy * cy;
}

template <typename T>
__global__ __launch_bounds__(kMeshBlock) void tri3_mesh_measure_kernel(
    int64_t ne, const int32_t *__restrict__ conn, const int32_t *__restrict__ x_src,
    const typename MeshRow<T>::type *__restrict__ x_free, const typename MeshRow<T>::type *__restrict__ x_fixed,
    const typename MeshRow<T>::type *__restrict__ x_ref, double *__restrict__ q_out, double *__restrict__ ratio_out,
    unsigned long long *summary) {
    __shared__ unsigned long long red[kMeshBlock / 64];
    const int64_t e = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    unsigned long long kq = ~0ull, kr = ~0ull;
    unsigned inv = 0;
    if (e < ne) {
        const int32_t n0 = conn[3 * e], n1 = conn[3 * e + 1], n2 = conn[3 * e + 2];
        const double2 X0 = corner<T>(x_free, x_fixed, x_src[n0]), X1 = corner<T>(x_free, x_fixed, x_src[n1]),
                      X2 = corner<T>(x_free, x_fixed, x_src[n2]);
        const typename MeshRow<T>::type r0 = x_ref[n0], r1 = x_ref[n1], r2 = x_ref[n2];
        const double det_ref = det3(make_double2(r0.x, r0.y), make_double2(r1.x, r1.y), make_double2(r2.x, r2.y));
        const double det = det3(X0, X1, X2);
        const double s = sign_of(det_ref);
        const double q = kTwoSqrt3 * s * det / edge_sq_sum(X0, X1, X2);
        const double ratio = det / det_ref;
        if (q_out) q_out[e] = q;
        if (ratio_out) ratio_out[e] = ratio;
        kq = dkey(q);
        kr = dkey(ratio);
        inv = !(s * det > 0.0);
    }
    mesh_measure_reduce(kq, kr, inv, red, summary);
}

// ---------------------------------------------------------------- step bound (closed form: first_crossing, hfem_mesh_dev.h)
template <typename T>
__global__ __launch_bounds__(kMeshBlock) void tri3_step_bound_kernel(
    int64_t ne, const int32_t *__restrict__ conn, const int32_t *__restrict__ x_src,
    const typename MeshRow<T>::type *__restrict__ x_free, const typename MeshRow<T>::type *__restrict__ x_fixed,
    const double2 *__restrict__ d, double eta, double *alpha) {
    __shared__ unsigned long long red[kMeshBlock / 64];
    const int64_t e = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    double a = INFINITY;
    if (e < ne) {
        const int32_t s0 = x_src[conn[3 * e]], s1 = x_src[conn[3 * e + 1]], s2 = x_src[conn[3 * e + 2]];
        const double2 X0 = corner<T>(x_free, x_fixed, s0), X1 = corner<T>(x_free, x_fixed, s1),
                      X2 = corner<T>(x_free, x_fixed, s2);
        const double2 zero = make_double2(0.0, 0.0);
        const double2 D0 = s0 >= 0 ? d[s0] : zero, D1 = s1 >= 0 ? d[s1] : zero, D2 = s2 >= 0 ? d[s2] : zero;
        // detJ(x + a d) with J columns (x0 - x2, x1 - x2) and their directions
        const double ax = X0.x - X2.x, ay = X0.y - X2.y, bx = X1.x - X2.x, by = X1.y - X2.y;
        const double dax = D0.x - D2.x, day = D0.y - D2.y, dbx = D1.x - D2.x, dby = D1.y - D2.y;
        const double A0 = ax * by - bx * ay;
        const double A1 = (ax * dby + dax * by) - (bx * day + dbx * ay);
        const double A2 = dax * dby - dbx * day;
        a = first_crossing(A0, A1, A2, eta);
    }
    // a >= 0 (or NaN from non-finite rows, whose pattern sorts above +inf): the u64 order of the bits is the numeric order
    const unsigned long long k = block_min_u64((unsigned long long)__double_as_longlong(a), red);
    if (threadIdx.x == 0) atomic_min_filtered(reinterpret_cast<unsigned long long *>(alpha), k);
}

// ---------------------------------------------------------------- quality barrier
// 1/q = S / (2 sqrt(3) s det), S = sum |e|^2:  d(1/q)/dX = (dS/dX det - S ddet/dX) / (2 sqrt(3) s det^2),
//   dS/dX0 = 2 (2 X0 - X1 - X2) (cyclic),  ddet/d(x0, y0) = (y1 - y2, x2 - x1), d(x1, y1) = (y2 - y0, x0 - x2),
//   d(x2, y2) = (y0 - y1, x1 - x0).   Finite for valid elements only (the solver keeps every element valid).
template <typename T>
__global__ __launch_bounds__(kMeshBlock) void tri3_quality_barrier_kernel(
    int64_t ne, const int32_t *__restrict__ conn, const int32_t *__restrict__ x_src,
    const typename MeshRow<T>::type *__restrict__ x_free, const typename MeshRow<T>::type *__restrict__ x_fixed,
    const typename MeshRow<T>::type *__restrict__ x_ref, double wscale, double *value, double *grad) {
    __shared__ double red[kMeshBlock / 64];
    const int64_t e = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    double v = 0.0;
    if (e < ne) {
        const int32_t n0 = conn[3 * e], n1 = conn[3 * e + 1], n2 = conn[3 * e + 2];
        const int32_t s0 = x_src[n0], s1 = x_src[n1], s2 = x_src[n2];
        const double2 X0 = corner<T>(x_free, x_fixed, s0), X1 = corner<T>(x_free, x_fixed, s1),
                      X2 = corner<T>(x_free, x_fixed, s2);
        const typename MeshRow<T>::type r0 = x_ref[n0], r1 = x_ref[n1], r2 = x_ref[n2];
        const double s = sign_of(det3(make_double2(r0.x, r0.y), make_double2(r1.x, r1.y), make_double2(r2.x, r2.y)));
        const double det = det3(X0, X1, X2), S = edge_sq_sum(X0, X1, X2);
        const double den = kTwoSqrt3 * s * det;
        v = wscale * (S / den - 1.0);
        if (grad) {
            const double f1 = wscale / den, f2 = -wscale * S / (den * det);   // d(w/Ne * S/den) = f1 dS + f2 ddet
            const double2 g0 = make_double2(f1 * 2.0 * (2.0 * X0.x - X1.x - X2.x) + f2 * (X1.y - X2.y),
                                            f1 * 2.0 * (2.0 * X0.y - X1.y - X2.y) + f2 * (X2.x - X1.x));
            const double2 g1 = make_double2(f1 * 2.0 * (2.0 * X1.x - X2.x - X0.x) + f2 * (X2.y - X0.y),
                                            f1 * 2.0 * (2.0 * X1.y - X2.y - X0.y) + f2 * (X0.x - X2.x));
            const double2 g2 = make_double2(f1 * 2.0 * (2.0 * X2.x - X0.x - X1.x) + f2 * (X0.y - X1.y),
                                            f1 * 2.0 * (2.0 * X2.y - X0.y - X1.y) + f2 * (X1.x - X0.x));
            const int32_t ss[3] = {s0, s1, s2};
            const double2 gg[3] = {g0, g1, g2};
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if (ss[c] >= 0) {
                    __hip_atomic_fetch_add(grad + 2 * (int64_t)ss[c], gg[c].x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_fetch_add(grad + 2 * (int64_t)ss[c] + 1, gg[c].y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
        }
    }
    const double tot = block_sum(v, red);
    if (threadIdx.x == 0 && value) __hip_atomic_fetch_add(value, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <typename T>
int mesh_measure(int device, const int32_t *conn, int64_t ne, const int32_t *x_src, const T *x_free, const T *x_fixed,
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
        hipLaunchKernelGGL(tri3_mesh_measure_kernel<T>, dim3(mesh_blocks(ne)), dim3(kMeshBlock), 0, s, ne, conn, x_src,
                           (const R *)x_free, (const R *)x_fixed, (const R *)x_ref, q_out, ratio_out, sm);
    hipLaunchKernelGGL(mesh_measure_finish_kernel, dim3(1), dim3(1), 0, s, sm);
    return launch_status("hfem_tri3_mesh_measure");
}

template <typename T>
int step_bound(int device, const int32_t *conn, int64_t ne, const int32_t *x_src, const T *x_free, const T *x_fixed,
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
        hipLaunchKernelGGL(tri3_step_bound_kernel<T>, dim3(mesh_blocks(ne)), dim3(kMeshBlock), 0, s, ne, conn, x_src,
                           (const R *)x_free, (const R *)x_fixed, (const double2 *)d, eta, alpha_out);
    return launch_status("hfem_tri3_step_bound");
}

template <typename T>
int quality_barrier(int device, const int32_t *conn, int64_t ne, const int32_t *x_src, const T *x_free, const T *x_fixed,
                    const T *x_ref, double weight, double *value_acc, double *grad_acc, void *stream) {
    HFEM_ARG_CHECK(x_free && (value_acc || grad_acc), "null pointer");
    HFEM_ARG_CHECK(ne >= 0 && ne < ((int64_t)1 << 31), "ne must be in [0, 2^31)");
    HFEM_ARG_CHECK(ne == 0 || (conn && x_src && x_ref), "null pointer");
    HFEM_ARG_CHECK(weight >= 0.0 && std::isfinite(weight), "weight must be finite and >= 0");
    if (ne == 0) return 0;
    if (int rc = use_device(device)) return rc;
    typedef typename MeshRow<T>::type R;
    hipLaunchKernelGGL(tri3_quality_barrier_kernel<T>, dim3(mesh_blocks(ne)), dim3(kMeshBlock), 0, (hipStream_t)stream, ne,
                       conn, x_src, (const R *)x_free, (const R *)x_fixed, (const R *)x_ref, weight / (double)ne, value_acc,
                       grad_acc);
    return launch_status("hfem_tri3_quality_barrier");
}

}  // namespace
}  // namespace hfem

#define HFEM_MESH_ABI(SUFFIX, T)                                                                                              \
    extern "C" int hfem_tri3_mesh_measure##SUFFIX(int device, const int32_t *conn, int64_t ne, const int32_t *x_src,           \
                                                  const T *x_free, const T *x_fixed, const T *x_ref, double *q_out,             \
                                                  double *ratio_out, double *summary_out, void *stream) {                       \
        return hfem::mesh_measure<T>(device, conn, ne, x_src, x_free, x_fixed, x_ref, q_out, ratio_out, summary_out, stream);  \
    }                                                                                                                          \
    extern "C" int hfem_tri3_step_bound##SUFFIX(int device, const int32_t *conn, int64_t ne, const int32_t *x_src,             \
                                                const T *x_free, const T *x_fixed, const double *d, double eta,                \
                                                double *alpha_out, void *stream) {                                             \
        return hfem::step_bound<T>(device, conn, ne, x_src, x_free, x_fixed, d, eta, alpha_out, stream);                       \
    }                                                                                                                          \
    extern "C" int hfem_tri3_quality_barrier##SUFFIX(int device, const int32_t *conn, int64_t ne, const int32_t *x_src,        \
                                                     const T *x_free, const T *x_fixed, const T *x_ref, double weight,         \
                                                     double *value_acc, double *grad_acc, void *stream) {                      \
        return hfem::quality_barrier<T>(device, conn, ne, x_src, x_free, x_fixed, x_ref, weight, value_acc, grad_acc, stream); \
    }

HFEM_MESH_ABI(, double)
HFEM_MESH_ABI(_f32, float)
#undef HFEM_MESH_ABI
