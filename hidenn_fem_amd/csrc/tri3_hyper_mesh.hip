// Mesh validity for r-adaptivity at finite strain on TRI3, gfx950 (MI355X): the det F-safe step bound and the deformation
// measure (hidenn_fem_amd/radapt.py, HyperRAdaptiveSolver).  The finite-strain siblings of tri3_mesh.hip's step
// bound and measure, launched the same way.
//
// One thread per element over the int32 connectivity (caller numbering); coordinate rows through the x row map (x_src[n] >= 0:
// x_free row, < 0: x_fixed row -1 - x_src[n]), displacement rows through the u row map of the same convention (u_src[n] >= 0:
// u_free row, < 0: u_fixed row -1 - u_src[n]), so any storage row order works.  Rows are fp64 or fp32 (T); all arithmetic is
// fp64.  The per-element closed forms are those of hfem_hyper_mesh_dev.h:
//   tri3_hyper_step_bound_kernel      the smaller of the reference crossing detJ(x + a d) = eta detJ(x) and the det F crossing
//                                     det F(a) = eta det F(0) at fixed u (both exact quadratics; 0 for an element that is
//                                     invalid already), min over the elements by a 64-bit atomic min on the bit pattern of
//                                     the non-negative double.  Deterministic, capturable (no host sync).
//   tri3_deformation_measure_kernel   J = det F = detJ(X + u) / detJ(X) per element (optional output); min J by monotone-key
//                                     atomic min and the count of elements with J <= 0 or NaN by integer atomic add, then a
//                                     one-thread finish that turns the words into doubles.  Order-independent: deterministic.
// The row access, the keys, the reductions and the one-thread init launch before each reduction are hfem_mesh_dev.h's.
// Gather-bound like the small-strain bound, with three more row reads and three more map words per element.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "hfem_hyper_mesh_dev.h"
#include "hfem_mesh_dev.h"

namespace hfem {
namespace {

template <typename T>
__global__ __launch_bounds__(kMeshBlock) void tri3_hyper_step_bound_kernel(
    int64_t ne, const int32_t *__restrict__ conn, const int32_t *__restrict__ x_src,
    const typename MeshRow<T>::type *__restrict__ x_free, const typename MeshRow<T>::type *__restrict__ x_fixed,
    const int32_t *__restrict__ u_src, const typename MeshRow<T>::type *__restrict__ u_free,
    const typename MeshRow<T>::type *__restrict__ u_fixed, const double2 *__restrict__ d, double eta, double *alpha) {
    __shared__ unsigned long long red[kMeshBlock / 64];
    const int64_t e = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    double a = INFINITY;
    if (e < ne) {
        const int32_t n0 = conn[3 * e], n1 = conn[3 * e + 1], n2 = conn[3 * e + 2];
        const int32_t s0 = x_src[n0], s1 = x_src[n1], s2 = x_src[n2];
        const double2 zero = make_double2(0.0, 0.0);
        const double2 X[3] = {corner<T>(x_free, x_fixed, s0), corner<T>(x_free, x_fixed, s1), corner<T>(x_free, x_fixed, s2)};
        const double2 U[3] = {corner<T>(u_free, u_fixed, u_src[n0]), corner<T>(u_free, u_fixed, u_src[n1]),
                              corner<T>(u_free, u_fixed, u_src[n2])};
        const double2 D[3] = {s0 >= 0 ? d[s0] : zero, s1 >= 0 ? d[s1] : zero, s2 >= 0 ? d[s2] : zero};
        double a_ref, a_def;
        tri3_hyper_crossings(X, U, D, eta, a_ref, a_def);
        a = smaller_crossing(a_ref, a_def);
    }
    // a >= 0 (or +inf): the u64 order of the bits is the numeric order
    const unsigned long long k = block_min_u64((unsigned long long)__double_as_longlong(a), red);
    if (threadIdx.x == 0) atomic_min_filtered(reinterpret_cast<unsigned long long *>(alpha), k);
}

template <typename T>
__global__ __launch_bounds__(kMeshBlock) void tri3_deformation_measure_kernel(
    int64_t ne, const int32_t *__restrict__ conn, const int32_t *__restrict__ x_src,
    const typename MeshRow<T>::type *__restrict__ x_free, const typename MeshRow<T>::type *__restrict__ x_fixed,
    const int32_t *__restrict__ u_src, const typename MeshRow<T>::type *__restrict__ u_free,
    const typename MeshRow<T>::type *__restrict__ u_fixed, double *__restrict__ j_out, unsigned long long *summary) {
    __shared__ unsigned long long red[kMeshBlock / 64];
    const int64_t e = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    unsigned long long kj = ~0ull;
    unsigned inv = 0;
    if (e < ne) {
        const int32_t n0 = conn[3 * e], n1 = conn[3 * e + 1], n2 = conn[3 * e + 2];
        const double2 X[3] = {corner<T>(x_free, x_fixed, x_src[n0]), corner<T>(x_free, x_fixed, x_src[n1]),
                              corner<T>(x_free, x_fixed, x_src[n2])};
        const double2 U[3] = {corner<T>(u_free, u_fixed, u_src[n0]), corner<T>(u_free, u_fixed, u_src[n1]),
                              corner<T>(u_free, u_fixed, u_src[n2])};
        const double j = tri3_det_f(X, U);
        if (j_out) j_out[e] = j;
        kj = dkey(j);
        inv = !(j > 0.0);
    }
    deformation_measure_reduce(kj, inv, red, summary);
}

template <typename T>
int hyper_step_bound(int device, const int32_t *conn, int64_t ne, const int32_t *x_src, const T *x_free, const T *x_fixed,
                     const int32_t *u_src, const T *u_free, const T *u_fixed, const double *d, double eta, double *alpha_out,
                     void *stream) {
    HFEM_ARG_CHECK(alpha_out && x_free && d && (u_free || u_fixed), "null pointer");
    HFEM_ARG_CHECK(ne >= 0 && ne < ((int64_t)1 << 31), "ne must be in [0, 2^31)");
    HFEM_ARG_CHECK(ne == 0 || (conn && x_src && u_src), "null pointer");
    HFEM_ARG_CHECK(eta > 0.0 && eta < 1.0, "eta must be in (0, 1)");
    if (int rc = use_device(device)) return rc;
    typedef typename MeshRow<T>::type R;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(step_bound_init_kernel, dim3(1), dim3(1), 0, s, alpha_out);
    if (ne > 0)
        hipLaunchKernelGGL(tri3_hyper_step_bound_kernel<T>, dim3(mesh_blocks(ne)), dim3(kMeshBlock), 0, s, ne, conn, x_src,
                           (const R *)x_free, (const R *)x_fixed, u_src, (const R *)u_free, (const R *)u_fixed,
                           (const double2 *)d, eta, alpha_out);
    return launch_status("hfem_tri3_hyper_step_bound");
}

template <typename T>
int deformation_measure(int device, const int32_t *conn, int64_t ne, const int32_t *x_src, const T *x_free, const T *x_fixed,
                        const int32_t *u_src, const T *u_free, const T *u_fixed, double *j_out, double *summary_out,
                        void *stream) {
    HFEM_ARG_CHECK(summary_out && x_free && (u_free || u_fixed), "null pointer");
    HFEM_ARG_CHECK(ne >= 0 && ne < ((int64_t)1 << 31), "ne must be in [0, 2^31)");
    HFEM_ARG_CHECK(ne == 0 || (conn && x_src && u_src), "null pointer");
    if (int rc = use_device(device)) return rc;
    typedef typename MeshRow<T>::type R;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *sm = reinterpret_cast<unsigned long long *>(summary_out);
    hipLaunchKernelGGL(deformation_measure_init_kernel, dim3(1), dim3(1), 0, s, sm);
    if (ne > 0)
        hipLaunchKernelGGL(tri3_deformation_measure_kernel<T>, dim3(mesh_blocks(ne)), dim3(kMeshBlock), 0, s, ne, conn, x_src,
                           (const R *)x_free, (const R *)x_fixed, u_src, (const R *)u_free, (const R *)u_fixed, j_out, sm);
    hipLaunchKernelGGL(deformation_measure_finish_kernel, dim3(1), dim3(1), 0, s, sm);
    return launch_status("hfem_tri3_deformation_measure");
}

}  // namespace
}  // namespace hfem

#define HFEM_HYPER_MESH_ABI(SUFFIX, T)                                                                                        \
    extern "C" int hfem_tri3_hyper_step_bound##SUFFIX(int device, const int32_t *conn, int64_t ne, const int32_t *x_src,       \
                                                      const T *x_free, const T *x_fixed, const int32_t *u_src,                 \
                                                      const T *u_free, const T *u_fixed, const double *d, double eta,          \
                                                      double *alpha_out, void *stream) {                                       \
        return hfem::hyper_step_bound<T>(device, conn, ne, x_src, x_free, x_fixed, u_src, u_free, u_fixed, d, eta, alpha_out, \
                                         stream);                                                                              \
    }                                                                                                                          \
    extern "C" int hfem_tri3_deformation_measure##SUFFIX(int device, const int32_t *conn, int64_t ne, const int32_t *x_src,    \
                                                         const T *x_free, const T *x_fixed, const int32_t *u_src,              \
                                                         const T *u_free, const T *u_fixed, double *j_out,                     \
                                                         double *summary_out, void *stream) {                                  \
        return hfem::deformation_measure<T>(device, conn, ne, x_src, x_free, x_fixed, u_src, u_free, u_fixed, j_out,          \
                                            summary_out, stream);                                                              \
    }

HFEM_HYPER_MESH_ABI(, double)
HFEM_HYPER_MESH_ABI(_f32, float)
#undef HFEM_HYPER_MESH_ABI
