// Implicit transient dynamics, gfx950 (MI355X): the vector kernels of a Newmark step in the a-form (hidenn_fem_amd/dynamics.py,
// DESIGN 26).  The linear solve of a step is the PCG driver's (cg.hip) on the shifted operator A = c_M M + c_K K
// (the MASS instances of tri3_cg.hip, quad4_cg.hip); what is left of a step is three elementwise passes over fp64 rows [n][2] in the storage
// order of u_free:
//   newmark_predict_kernel   u~ = u + dt v + dt^2 (1/2 - beta) a,   v~ = v + dt (1 - gamma) a,   w = u~ + beta_R v~
//   newmark_rhs_kernel       rhs = load b0 - K w - alpha_R M v~;   g_zero = rhs,   g0 = A a - rhs  (what hfem_cg_start takes:
//                            r = -g0 is the residual of the warm start a, |g_zero| the norm of the stopping test)
//   newmark_correct_kernel   u = u~ + beta dt^2 a+,   v = v~ + gamma dt a+
// One row (16 bytes) per access, grid-stride under a fixed grid cap, launch-only (capturable).  Every output entry is one or
// two FMAs of its own row: bit-reproducible, no reduction, no atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "hfem_device.h"

namespace hfem {
namespace {

constexpr int kDynBlock = 256, kDynMaxBlocks = 1024;

__global__ __launch_bounds__(kDynBlock) void newmark_predict_kernel(int64_t n, const double2 *__restrict__ u,
                                                                    const double2 *__restrict__ v,
                                                                    const double2 *__restrict__ a, double dt, double c_ua,
                                                                    double c_va, double beta_r, double2 *__restrict__ ut,
                                                                    double2 *__restrict__ vt, double2 *__restrict__ w) {
    for (int64_t i = (int64_t)blockIdx.x * kDynBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kDynBlock) {
        const double2 ui = u[i], vi = v[i], ai = a[i];
        const double2 p = make_double2(__builtin_fma(c_ua, ai.x, __builtin_fma(dt, vi.x, ui.x)),
                                       __builtin_fma(c_ua, ai.y, __builtin_fma(dt, vi.y, ui.y)));
        const double2 q = make_double2(__builtin_fma(c_va, ai.x, vi.x), __builtin_fma(c_va, ai.y, vi.y));
        ut[i] = p;
        vt[i] = q;
        w[i] = make_double2(__builtin_fma(beta_r, q.x, p.x), __builtin_fma(beta_r, q.y, p.y));
    }
}

// mv == NULL: no mass-proportional damping (alpha_R = 0)
__global__ __launch_bounds__(kDynBlock) void newmark_rhs_kernel(int64_t n, const double2 *__restrict__ b0,
                                                                const double2 *__restrict__ kw, const double2 *__restrict__ mv,
                                                                const double2 *__restrict__ aa, double load, double alpha_r,
                                                                double2 *__restrict__ g0, double2 *__restrict__ gzero) {
    for (int64_t i = (int64_t)blockIdx.x * kDynBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kDynBlock) {
        const double2 b = b0[i], k = kw[i], q = aa[i];
        double2 r = make_double2(__builtin_fma(load, b.x, -k.x), __builtin_fma(load, b.y, -k.y));
        if (mv) {
            const double2 m = mv[i];
            r.x = __builtin_fma(-alpha_r, m.x, r.x);
            r.y = __builtin_fma(-alpha_r, m.y, r.y);
        }
        gzero[i] = r;
        g0[i] = make_double2(q.x - r.x, q.y - r.y);
    }
}

// u may be ut and v may be vt (every row is read before it is written)
__global__ __launch_bounds__(kDynBlock) void newmark_correct_kernel(int64_t n, const double2 *ut, const double2 *vt,
                                                                    const double2 *__restrict__ a, double c_u, double c_v,
                                                                    double2 *u, double2 *v) {
    for (int64_t i = (int64_t)blockIdx.x * kDynBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kDynBlock) {
        const double2 p = ut[i], q = vt[i], ai = a[i];
        u[i] = make_double2(__builtin_fma(c_u, ai.x, p.x), __builtin_fma(c_u, ai.y, p.y));
        v[i] = make_double2(__builtin_fma(c_v, ai.x, q.x), __builtin_fma(c_v, ai.y, q.y));
    }
}

dim3 dyn_grid(int64_t n) { return dim3((unsigned)std::min<int64_t>(kDynMaxBlocks, (n + kDynBlock - 1) / kDynBlock)); }

// len doubles = len / 2 rows; 0 rows is a no-op (returns 1), an argument error returns -1
int dyn_check(const char *who, int device, int64_t len, bool pointers, bool scalars) {
    if (device < 0) { set_error(std::string(who) + ": negative device"); return -1; }
    if (len < 0 || (len & 1)) { set_error(std::string(who) + ": len must be even and >= 0 (rows of two doubles)"); return -1; }
    if (!pointers) { set_error(std::string(who) + ": null pointer"); return -1; }
    if (!scalars) { set_error(std::string(who) + ": non-finite scalar"); return -1; }
    return len == 0 ? 1 : 0;
}

}  // namespace
}  // namespace hfem

using namespace hfem;

extern "C" int hfem_newmark_predict(int device, const double *u, const double *v, const double *a, int64_t len, double dt,
                                    double beta, double gamma, double beta_r, double *u_pred, double *v_pred, double *w,
                                    void *stream) {
    const char *who = "hfem_newmark_predict";
    if (int rc = dyn_check(who, device, len, u && v && a && u_pred && v_pred && w,
                           std::isfinite(dt) && std::isfinite(beta) && std::isfinite(gamma) && std::isfinite(beta_r)))
        return rc < 0 ? rc : 0;
    if (u_pred == u || u_pred == v || u_pred == a || v_pred == u || v_pred == v || v_pred == a || w == u || w == v || w == a ||
        u_pred == v_pred || u_pred == w || v_pred == w) {
        set_error(std::string(who) + ": the three outputs must differ from each other and from the inputs");
        return -1;
    }
    if (int rc = use_device(device)) return rc;
    const int64_t n = len / 2;
    hipLaunchKernelGGL(newmark_predict_kernel, dyn_grid(n), dim3(kDynBlock), 0, (hipStream_t)stream, n, (const double2 *)u,
                       (const double2 *)v, (const double2 *)a, dt, dt * dt * (0.5 - beta), dt * (1.0 - gamma), beta_r,
                       (double2 *)u_pred, (double2 *)v_pred, (double2 *)w);
    return launch_status(who);
}

extern "C" int hfem_newmark_rhs(int device, const double *b0, const double *kw, const double *mv, const double *aa, int64_t len,
                                double load, double alpha_r, double *g0, double *g_zero, void *stream) {
    const char *who = "hfem_newmark_rhs";
    if (int rc = dyn_check(who, device, len, b0 && kw && aa && g0 && g_zero, std::isfinite(load) && std::isfinite(alpha_r)))
        return rc < 0 ? rc : 0;
    if (g0 == g_zero || g0 == b0 || g0 == kw || g0 == mv || g0 == aa || g_zero == b0 || g_zero == kw || g_zero == mv ||
        g_zero == aa) {
        set_error(std::string(who) + ": the two outputs must differ from each other and from the inputs");
        return -1;
    }
    if (int rc = use_device(device)) return rc;
    const int64_t n = len / 2;
    hipLaunchKernelGGL(newmark_rhs_kernel, dyn_grid(n), dim3(kDynBlock), 0, (hipStream_t)stream, n, (const double2 *)b0,
                       (const double2 *)kw, (const double2 *)mv, (const double2 *)aa, load, alpha_r, (double2 *)g0,
                       (double2 *)g_zero);
    return launch_status(who);
}

extern "C" int hfem_newmark_correct(int device, const double *u_pred, const double *v_pred, const double *a, int64_t len, double dt,
                                    double beta, double gamma, double *u, double *v, void *stream) {
    const char *who = "hfem_newmark_correct";
    if (int rc = dyn_check(who, device, len, u_pred && v_pred && a && u && v,
                           std::isfinite(dt) && std::isfinite(beta) && std::isfinite(gamma)))
        return rc < 0 ? rc : 0;
    if (u == v || u == a || v == a || u == v_pred || v == u_pred) {
        set_error(std::string(who) + ": u may alias u_pred and v may alias v_pred, nothing else");
        return -1;
    }
    if (int rc = use_device(device)) return rc;
    const int64_t n = len / 2;
    hipLaunchKernelGGL(newmark_correct_kernel, dyn_grid(n), dim3(kDynBlock), 0, (hipStream_t)stream, n, (const double2 *)u_pred,
                       (const double2 *)v_pred, (const double2 *)a, beta * dt * dt, gamma * dt, (double2 *)u, (double2 *)v);
    return launch_status(who);
}
