// Mesh validity for r-adaptivity at finite strain on QUAD4, gfx950 (MI355X): the bilinear-cell twins of
// tri3_hyper_mesh.hip -- the det F-safe step bound and the deformation measure (hidenn_fem_amd/radapt.py,
// Quad4HyperRAdaptiveSolver).
//
// One thread per element over the int32 connectivity [ne][4] (caller numbering, local nodes counter-clockwise as in
// quad4_mesh.hip); coordinate rows through the x row map, displacement rows through the u row map of the same convention
// (src >= 0: the free row, < 0: the fixed row -1 - src).  Rows are fp64 or fp32 (T); all arithmetic is fp64.  Per corner k the
// reference cell has c_k = e_{k-1} x e_k and the deformed cell (rows X + u) c_k^def; detJ of a bilinear cell is affine over
// the reference square, so at any point of the cell det F is a mean of the corner ratios r_k = c_k^def / c_k with positive
// weights (hfem_hyper_mesh_dev.h holds the closed forms):
//   quad4_hyper_step_bound_kernel     per corner the smaller of the reference crossing c_k(a) = eta c_k(0) and the det F
//                                     crossing r_k(a) = eta r_k(0) at fixed u, min over the corners and the elements (64-bit
//                                     atomic min on the bit pattern of the non-negative double).  Below it every corner keeps
//                                     eta of c_k and of r_k: det F at every point of a cell stays at or above eta times the
//                                     cell's smallest corner det F before the step.  Deterministic, capturable.
//   quad4_deformation_measure_kernel  J = min_k r_k per element (optional output); min J and the count of elements with
//                                     J <= 0 or NaN, reduced as the TRI3 measure reduces.  Deterministic.
// Gather-bound: per element 16 B of connectivity, eight map words and eight (bound: up to twelve) rows; no LDS beyond the
// reduction words, no per-thread array that survives unrolling (no scratch).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "hfem_hyper_mesh_dev.h"
#include "hfem_mesh_dev.h"

namespace hfem {
namespace {

// the four corner rows X and displacement rows U of element e, and the x row map entries of its nodes
template <typename T>
__device__ __forceinline__ void load_corner_rows(const int32_t *__restrict__ conn, int64_t e, const int32_t *__restrict__ x_src,
                                                 const typename MeshRow<T>::type *__restrict__ x_free,
                                                 const typename MeshRow<T>::type *__restrict__ x_fixed,
                                                 const int32_t *__restrict__ u_src,
                                                 const typename MeshRow<T>::type *__restrict__ u_free,
                                                 const typename MeshRow<T>::type *__restrict__ u_fixed, int32_t (&src)[4],
                                                 double2 (&X)[4], double2 (&U)[4]) {
    int32_t n[4], us[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) n[k] = conn[4 * e + k];          // dword loads: the caller's pointer need not be 16-byte aligned
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        src[k] = x_src[n[k]];
        us[k] = u_src[n[k]];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        X[k] = corner<T>(x_free, x_fixed, src[k]);
        U[k] = corner<T>(u_free, u_fixed, us[k]);
    }
}

template <typename T>
__global__ __launch_bounds__(kMeshBlock) void quad4_hyper_step_bound_kernel(
    int64_t ne, const int32_t *__restrict__ conn, const int32_t *__restrict__ x_src,
    const typename MeshRow<T>::type *__restrict__ x_free, const typename MeshRow<T>::type *__restrict__ x_fixed,
    const int32_t *__restrict__ u_src, const typename MeshRow<T>::type *__restrict__ u_free,
    const typename MeshRow<T>::type *__restrict__ u_fixed, const double2 *__restrict__ d, double eta, double *alpha) {
    __shared__ unsigned long long red[kMeshBlock / 64];
    const int64_t e = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    double a = INFINITY;
    if (e < ne) {
        int32_t src[4];
        double2 X[4], U[4], D[4];
        load_corner_rows<T>(conn, e, x_src, x_free, x_fixed, u_src, u_free, u_fixed, src, X, U);
#pragma unroll
        for (int k = 0; k < 4; ++k) D[k] = src[k] >= 0 ? d[src[k]] : make_double2(0.0, 0.0);
        double a_ref, a_def;
        quad4_hyper_crossings(X, U, D, eta, a_ref, a_def);
        a = smaller_crossing(a_ref, a_def);
    }
    // a >= 0 (or +inf): the u64 order of the bits is the numeric order
    const unsigned long long k = block_min_u64((unsigned long long)__double_as_longlong(a), red);
    if (threadIdx.x == 0) atomic_min_filtered(reinterpret_cast<unsigned long long *>(alpha), k);
}

template <typename T>
__global__ __launch_bounds__(kMeshBlock) void quad4_deformation_measure_kernel(
    int64_t ne, const int32_t *__restrict__ conn, const int32_t *__restrict__ x_src,
    const typename MeshRow<T>::type *__restrict__ x_free, const typename MeshRow<T>::type *__restrict__ x_fixed,
    const int32_t *__restrict__ u_src, const typename MeshRow<T>::type *__restrict__ u_free,
    const typename MeshRow<T>::type *__restrict__ u_fixed, double *__restrict__ j_out, unsigned long long *summary) {
    __shared__ unsigned long long red[kMeshBlock / 64];
    const int64_t e = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    unsigned long long kj = ~0ull;
    unsigned inv = 0;
    if (e < ne) {
        int32_t src[4];
        double2 X[4], U[4];
        load_corner_rows<T>(conn, e, x_src, x_free, x_fixed, u_src, u_free, u_fixed, src, X, U);
        const double j = quad4_corner_det_f(X, U);
        if (j_out) j_out[e] = j;
        kj = dkey(j);
        inv = !(j > 0.0);
    }
    deformation_measure_reduce(kj, inv, red, summary);
}

template <typename T>
int quad4_hyper_step_bound(int device, const int32_t *conn, int64_t ne, const int32_t *x_src, const T *x_free,
                           const T *x_fixed, const int32_t *u_src, const T *u_free, const T *u_fixed, const double *d,
                           double eta, double *alpha_out, void *stream) {
    HFEM_ARG_CHECK(alpha_out && x_free && d && (u_free || u_fixed), "null pointer");
    HFEM_ARG_CHECK(ne >= 0 && ne < ((int64_t)1 << 31), "ne must be in [0, 2^31)");
    HFEM_ARG_CHECK(ne == 0 || (conn && x_src && u_src), "null pointer");
    HFEM_ARG_CHECK(eta > 0.0 && eta < 1.0, "eta must be in (0, 1)");
    if (int rc = use_device(device)) return rc;
    typedef typename MeshRow<T>::type R;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(step_bound_init_kernel, dim3(1), dim3(1), 0, s, alpha_out);
    if (ne > 0)
        hipLaunchKernelGGL(quad4_hyper_step_bound_kernel<T>, dim3(mesh_blocks(ne)), dim3(kMeshBlock), 0, s, ne, conn, x_src,
                           (const R *)x_free, (const R *)x_fixed, u_src, (const R *)u_free, (const R *)u_fixed,
                           (const double2 *)d, eta, alpha_out);
    return launch_status("hfem_quad4_hyper_step_bound");
}

template <typename T>
int quad4_deformation_measure(int device, const int32_t *conn, int64_t ne, const int32_t *x_src, const T *x_free,
                              const T *x_fixed, const int32_t *u_src, const T *u_free, const T *u_fixed, double *j_out,
                              double *summary_out, void *stream) {
    HFEM_ARG_CHECK(summary_out && x_free && (u_free || u_fixed), "null pointer");
    HFEM_ARG_CHECK(ne >= 0 && ne < ((int64_t)1 << 31), "ne must be in [0, 2^31)");
    HFEM_ARG_CHECK(ne == 0 || (conn && x_src && u_src), "null pointer");
    if (int rc = use_device(device)) return rc;
    typedef typename MeshRow<T>::type R;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *sm = reinterpret_cast<unsigned long long *>(summary_out);
    hipLaunchKernelGGL(deformation_measure_init_kernel, dim3(1), dim3(1), 0, s, sm);
    if (ne > 0)
        hipLaunchKernelGGL(quad4_deformation_measure_kernel<T>, dim3(mesh_blocks(ne)), dim3(kMeshBlock), 0, s, ne, conn, x_src,
                           (const R *)x_free, (const R *)x_fixed, u_src, (const R *)u_free, (const R *)u_fixed, j_out, sm);
    hipLaunchKernelGGL(deformation_measure_finish_kernel, dim3(1), dim3(1), 0, s, sm);
    return launch_status("hfem_quad4_deformation_measure");
}

}  // namespace
}  // namespace hfem

#define HFEM_QUAD4_HYPER_MESH_ABI(SUFFIX, T)                                                                                  \
    extern "C" int hfem_quad4_hyper_step_bound##SUFFIX(int device, const int32_t *conn, int64_t ne, const int32_t *x_src,      \
                                                       const T *x_free, const T *x_fixed, const int32_t *u_src,                \
                                                       const T *u_free, const T *u_fixed, const double *d, double eta,         \
                                                       double *alpha_out, void *stream) {                                      \
        return hfem::quad4_hyper_step_bound<T>(device, conn, ne, x_src, x_free, x_fixed, u_src, u_free, u_fixed, d, eta,      \
                                               alpha_out, stream);                                                             \
    }                                                                                                                          \
    extern "C" int hfem_quad4_deformation_measure##SUFFIX(int device, const int32_t *conn, int64_t ne, const int32_t *x_src,   \
                                                          const T *x_free, const T *x_fixed, const int32_t *u_src,             \
                                                          const T *u_free, const T *u_fixed, double *j_out,                    \
                                                          double *summary_out, void *stream) {                                 \
        return hfem::quad4_deformation_measure<T>(device, conn, ne, x_src, x_free, x_fixed, u_src, u_free, u_fixed, j_out,    \
                                                  summary_out, stream);                                                        \
    }

HFEM_QUAD4_HYPER_MESH_ABI(, double)
HFEM_QUAD4_HYPER_MESH_ABI(_f32, float)
#undef HFEM_QUAD4_HYPER_MESH_ABI
