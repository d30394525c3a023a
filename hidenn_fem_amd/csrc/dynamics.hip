// Implicit transient dynamics, gfx950 (MI355X): the vector kernels of a Newmark step in the a-form (hidenn_fem_amd/dynamics.py,
// DESIGN 26).  The linear solve of a step is the PCG driver's (cg.hip) on the shifted operator A = c_M M + c_K K
// (the MASS instances of tri3_cg.hip, quad4_cg.hip); what is left of a step is three elementwise passes over fp64 rows [n][2] in the storage
// order of u_free:
//   newmark_predict_kernel   u~ = u + dt v + dt^2 (1/2 - beta) a,   v~ = v + dt (1 - gamma) a,   w = u~ + beta_R v~
//   newmark_rhs_kernel       rhs = load b0 - K w - alpha_R M v~;   g_zero = rhs,   g0 = A a - rhs  (what hfem_cg_start takes:
//                            r = -g0 is the residual of the warm start a, |g_zero| the norm of the stopping test)
//   newmark_correct_kernel   u = u~ + beta dt^2 a+,   v = v~ + gamma dt a+
// and, for the Newton loop of a finite-strain step (HyperNewmarkSolver, DESIGN 27: A = c_M M + c_K K_T(u), the MASS instances
// of tri3_hyper_cg.hip, quad4_hyper_cg.hip), two more:
//   newmark_trial_kernel     a_t = a + s d,   u_t = u~ + c_K a_t,   (M a)_t = M a + s M d   (M is linear: M d is formed once per
//                            Newton iteration, a line-search trial costs this pass and one energy launch)
//   newmark_residual_kernel  R = c_M (M a) + alpha_R (M v~) + f_int - load b_ext,   and -R
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

// every output may be its input of the same role (a_t = a, ma_t = ma): each row is read before it is written
__global__ __launch_bounds__(kDynBlock) void newmark_trial_kernel(int64_t n, const double2 *a, const double2 *__restrict__ d,
                                                                  const double2 *__restrict__ ut, const double2 *ma,
                                                                  const double2 *__restrict__ md, double s, double c_k,
                                                                  double2 *a_t, double2 *__restrict__ u_t, double2 *ma_t) {
    for (int64_t i = (int64_t)blockIdx.x * kDynBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kDynBlock) {
        const double2 ai = a[i], di = d[i], ui = ut[i], mi = ma[i], ni = md[i];
        const double2 at = make_double2(__builtin_fma(s, di.x, ai.x), __builtin_fma(s, di.y, ai.y));
        a_t[i] = at;
        u_t[i] = make_double2(__builtin_fma(c_k, at.x, ui.x), __builtin_fma(c_k, at.y, ui.y));
        ma_t[i] = make_double2(__builtin_fma(s, ni.x, mi.x), __builtin_fma(s, ni.y, mi.y));
    }
}

// mv == NULL: no mass-proportional damping (alpha_R = 0); neg_r == NULL: only R
__global__ __launch_bounds__(kDynBlock) void newmark_residual_kernel(int64_t n, const double2 *__restrict__ ma,
                                                                     const double2 *__restrict__ mv,
                                                                     const double2 *__restrict__ fint,
                                                                     const double2 *__restrict__ b, double c_m, double alpha_r,
                                                                     double load, double2 *__restrict__ r,
                                                                     double2 *__restrict__ neg_r) {
    for (int64_t i = (int64_t)blockIdx.x * kDynBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kDynBlock) {
        const double2 m = ma[i], f = fint[i], bi = b[i];
        double2 v = make_double2(__builtin_fma(c_m, m.x, __builtin_fma(-load, bi.x, f.x)),
                                 __builtin_fma(c_m, m.y, __builtin_fma(-load, bi.y, f.y)));
        if (mv) {
            const double2 w = mv[i];
            v.x = __builtin_fma(alpha_r, w.x, v.x);
            v.y = __builtin_fma(alpha_r, w.y, v.y);
        }
        r[i] = v;
        if (neg_r) neg_r[i] = make_double2(-v.x, -v.y);
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

extern "C" int hfem_newmark_trial(int device, const double *a, const double *d, const double *u_pred, const double *ma,
                                  const double *md, int64_t len, double s, double c_k, double *a_t, double *u_t, double *ma_t,
                                  void *stream) {
    const char *who = "hfem_newmark_trial";
    if (int rc = dyn_check(who, device, len, a && d && u_pred && ma && md && a_t && u_t && ma_t, std::isfinite(s) && std::isfinite(c_k)))
        return rc < 0 ? rc : 0;
    if (a_t == u_t || a_t == ma_t || u_t == ma_t || a_t == d || a_t == u_pred || a_t == ma || a_t == md || u_t == a || u_t == d ||
        u_t == u_pred || u_t == ma || u_t == md || ma_t == a || ma_t == d || ma_t == u_pred || ma_t == md) {
        set_error(std::string(who) + ": a_t may alias a and ma_t may alias ma, nothing else");
        return -1;
    }
    if (int rc = use_device(device)) return rc;
    const int64_t n = len / 2;
    hipLaunchKernelGGL(newmark_trial_kernel, dyn_grid(n), dim3(kDynBlock), 0, (hipStream_t)stream, n, (const double2 *)a,
                       (const double2 *)d, (const double2 *)u_pred, (const double2 *)ma, (const double2 *)md, s, c_k, (double2 *)a_t,
                       (double2 *)u_t, (double2 *)ma_t);
    return launch_status(who);
}

extern "C" int hfem_newmark_residual(int device, const double *ma, const double *mv, const double *f_int, const double *b_ext,
                                     int64_t len, double c_m, double alpha_r, double load, double *r, double *neg_r, void *stream) {
    const char *who = "hfem_newmark_residual";
    if (int rc = dyn_check(who, device, len, ma && f_int && b_ext && r,
                           std::isfinite(c_m) && std::isfinite(alpha_r) && std::isfinite(load)))
        return rc < 0 ? rc : 0;
    if (r == neg_r || r == ma || r == mv || r == f_int || r == b_ext || (neg_r && (neg_r == ma || neg_r == mv || neg_r == f_int ||
                                                                                  neg_r == b_ext))) {
        set_error(std::string(who) + ": the two outputs must differ from each other and from the inputs");
        return -1;
    }
    if (int rc = use_device(device)) return rc;
    const int64_t n = len / 2;
    hipLaunchKernelGGL(newmark_residual_kernel, dyn_grid(n), dim3(kDynBlock), 0, (hipStream_t)stream, n, (const double2 *)ma,
                       (const double2 *)mv, (const double2 *)f_int, (const double2 *)b_ext, c_m, alpha_r, load, (double2 *)r,
                       (double2 *)neg_r);
    return launch_status(who);
}
