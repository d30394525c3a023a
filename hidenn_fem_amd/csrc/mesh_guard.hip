// Mesh validity for r-adaptivity on TRI3 and QUAD4, gfx950 (MI355X): the element measure, the inversion-safe step bound and
// the opt-in quality barrier at small strain, the det F-safe step bound and the deformation measure at finite strain
// (hidenn_fem_amd/radapt.py).  No reference counterpart: the reference's example 4 moves the nodes
// with L-BFGS and nothing keeps an element from turning inside out (its alternating-scheme sketch calls a mesh_quality_loss
// it never defines).
//
// The kernels are the instances of hfem_mesh_dev.h's frame over {Tri3, Quad4} x the five operations x {fp64, fp32 rows}; the
// per-element mathematics is hfem_mesh_elem_dev.h's.  Here: one launcher per reduction kind and the twenty entry points.
//   bound     init + element kernel (2 launches): deterministic, capturable (no host sync)
//   summary   init + element kernel + finish (3 launches): min q, min ratio, inverted count / min J, count of J <= 0 or NaN
//   sum       the element kernel alone, ACCUMULATING onto the caller's value and gradient with fp64 atomics
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "hfem_common.h"
#include "hfem_mesh_dev.h"

namespace hfem {
namespace {

// The arguments of an entry point, under the names the frame gives them (what an operation does not read stays null).
struct MeshCall {
    const char *name;
    int device;
    const int32_t *conn;
    int64_t ne;
    const int32_t *x_src;
    const void *x_free, *x_fixed, *x_ref;
    const int32_t *u_src;
    const void *u_free, *u_fixed;
    const double *d;
    double param;                                                // eta, or the barrier's weight
    double *out0, *out1, *acc;
    void *stream;
};

int arg_error(const MeshCall &c, const char *msg) {
    set_error(std::string(c.name) + ": " + msg);
    return -1;
}

// What every entry point checks of its rows, before any device is touched; `outputs` = it has somewhere to write.
template <typename Op> int check_rows(const MeshCall &c, bool outputs) {
    if (!(outputs && c.x_free && (!Op::kDir || c.d) && (!Op::kU || c.u_free || c.u_fixed))) return arg_error(c, "null pointer");
    if (!(c.ne >= 0 && c.ne < ((int64_t)1 << 31))) return arg_error(c, "ne must be in [0, 2^31)");
    if (!(c.ne == 0 || (c.conn && c.x_src && (!Op::kRef || c.x_ref) && (!Op::kU || c.u_src)))) return arg_error(c, "null pointer");
    return 0;
}

template <typename E, typename Op, typename T> void launch_elements(const MeshCall &c, double param) {
    typedef const typename MeshRow<T>::type *R;
    hipLaunchKernelGGL((mesh_element_kernel<E, Op, T>), dim3(mesh_blocks(c.ne)), dim3(kMeshBlock), 0, (hipStream_t)c.stream, c.ne,
                       c.conn, c.x_src, (R)c.x_free, (R)c.x_fixed, (R)c.x_ref, c.u_src, (R)c.u_free, (R)c.u_fixed,
                       (const double2 *)c.d, param, c.out0, c.out1, reinterpret_cast<unsigned long long *>(c.acc));
}

template <typename E, typename Op, typename T> int launch_bound(const MeshCall &c) {
    if (int rc = check_rows<Op>(c, c.acc != nullptr)) return rc;
    if (!(c.param > 0.0 && c.param < 1.0)) return arg_error(c, "eta must be in (0, 1)");
    if (int rc = use_device(c.device)) return rc;
    hipLaunchKernelGGL(step_bound_init_kernel, dim3(1), dim3(1), 0, (hipStream_t)c.stream, c.acc);
    if (c.ne > 0) launch_elements<E, Op, T>(c, c.param);
    return launch_status(c.name);
}

template <typename E, typename Op, typename T> int launch_summary(const MeshCall &c) {
    constexpr int K = Op::Reduce::kKeys;
    if (int rc = check_rows<Op>(c, c.acc != nullptr)) return rc;
    if (int rc = use_device(c.device)) return rc;
    unsigned long long *sm = reinterpret_cast<unsigned long long *>(c.acc);
    hipLaunchKernelGGL(summary_init_kernel<K>, dim3(1), dim3(1), 0, (hipStream_t)c.stream, sm);
    if (c.ne > 0) launch_elements<E, Op, T>(c, 0.0);
    hipLaunchKernelGGL(summary_finish_kernel<K>, dim3(1), dim3(1), 0, (hipStream_t)c.stream, sm);
    return launch_status(c.name);
}

template <typename E, typename Op, typename T> int launch_sum(const MeshCall &c) {
    if (int rc = check_rows<Op>(c, c.out0 || c.out1)) return rc;
    if (!(c.param >= 0.0 && std::isfinite(c.param))) return arg_error(c, "weight must be finite and >= 0");
    if (c.ne == 0) return 0;
    if (int rc = use_device(c.device)) return rc;
    launch_elements<E, Op, T>(c, c.param / (E::kBarrierTerms * (double)c.ne));
    return launch_status(c.name);
}

}  // namespace
}  // namespace hfem

// The five entry points of one element kind and row type.  MeshCall's fields in order: name, device, conn, ne, x_src, x_free,
// x_fixed, x_ref, u_src, u_free, u_fixed, d, param, out0, out1, acc, stream.
#define HFEM_MESH_GUARD_ABI(KIND, E, SUFFIX, T)                                                                               \
    extern "C" int hfem_##KIND##_mesh_measure##SUFFIX(int device, const int32_t *conn, int64_t ne, const int32_t *x_src,       \
                                                      const T *x_free, const T *x_fixed, const T *x_ref, double *q_out,         \
                                                      double *ratio_out, double *summary_out, void *stream) {                   \
        return hfem::launch_summary<hfem::E, hfem::MeasureOp, T>(                                                              \
            {"hfem_" #KIND "_mesh_measure", device, conn, ne, x_src, x_free, x_fixed, x_ref, nullptr, nullptr, nullptr, nullptr, \
             0.0, q_out, ratio_out, summary_out, stream});                                                                     \
    }                                                                                                                          \
    extern "C" int hfem_##KIND##_step_bound##SUFFIX(int device, const int32_t *conn, int64_t ne, const int32_t *x_src,         \
                                                    const T *x_free, const T *x_fixed, const double *d, double eta,            \
                                                    double *alpha_out, void *stream) {                                         \
        return hfem::launch_bound<hfem::E, hfem::StepBoundOp, T>(                                                              \
            {"hfem_" #KIND "_step_bound", device, conn, ne, x_src, x_free, x_fixed, nullptr, nullptr, nullptr, nullptr, d, eta, \
             nullptr, nullptr, alpha_out, stream});                                                                            \
    }                                                                                                                          \
    extern "C" int hfem_##KIND##_quality_barrier##SUFFIX(int device, const int32_t *conn, int64_t ne, const int32_t *x_src,    \
                                                         const T *x_free, const T *x_fixed, const T *x_ref, double weight,     \
                                                         double *value_acc, double *grad_acc, void *stream) {                  \
        return hfem::launch_sum<hfem::E, hfem::BarrierOp, T>(                                                                  \
            {"hfem_" #KIND "_quality_barrier", device, conn, ne, x_src, x_free, x_fixed, x_ref, nullptr, nullptr, nullptr,      \
             nullptr, weight, value_acc, grad_acc, nullptr, stream});                                                          \
    }                                                                                                                          \
    extern "C" int hfem_##KIND##_hyper_step_bound##SUFFIX(int device, const int32_t *conn, int64_t ne, const int32_t *x_src,   \
                                                          const T *x_free, const T *x_fixed, const int32_t *u_src,             \
                                                          const T *u_free, const T *u_fixed, const double *d, double eta,      \
                                                          double *alpha_out, void *stream) {                                   \
        return hfem::launch_bound<hfem::E, hfem::HyperStepBoundOp, T>(                                                         \
            {"hfem_" #KIND "_hyper_step_bound", device, conn, ne, x_src, x_free, x_fixed, nullptr, u_src, u_free, u_fixed, d,   \
             eta, nullptr, nullptr, alpha_out, stream});                                                                       \
    }                                                                                                                          \
    extern "C" int hfem_##KIND##_deformation_measure##SUFFIX(int device, const int32_t *conn, int64_t ne,                      \
                                                             const int32_t *x_src, const T *x_free, const T *x_fixed,          \
                                                             const int32_t *u_src, const T *u_free, const T *u_fixed,          \
                                                             double *j_out, double *summary_out, void *stream) {               \
        return hfem::launch_summary<hfem::E, hfem::DeformationOp, T>(                                                          \
            {"hfem_" #KIND "_deformation_measure", device, conn, ne, x_src, x_free, x_fixed, nullptr, u_src, u_free, u_fixed,   \
             nullptr, 0.0, j_out, nullptr, summary_out, stream});                                                              \
    }

HFEM_MESH_GUARD_ABI(tri3, Tri3, , double)
HFEM_MESH_GUARD_ABI(tri3, Tri3, _f32, float)
HFEM_MESH_GUARD_ABI(quad4, Quad4, , double)
HFEM_MESH_GUARD_ABI(quad4, Quad4, _f32, float)
#undef HFEM_MESH_GUARD_ABI
