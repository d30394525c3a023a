// Device-side helpers shared by the gfx950 kernels of libhidenn_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include "hfem_common.h"

namespace hfem {

#define HFEM_HIP_CHECK(expr)                                                          \
    do {                                                                              \
        hipError_t _e = (expr);                                                       \
        if (_e != hipSuccess) {                                                       \
            ::hfem::set_error(std::string(__func__) + ": " #expr " -> " +             \
                              hipGetErrorString(_e));                                 \
            return (int)_e;                                                           \
        }                                                                             \
    } while (0)

// Select the device for this call (no thread-affine state is kept: PyTorch runs
// backward on a different host thread than forward).
inline int use_device(int device) {
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) {
        set_error(std::string("hipSetDevice(") + std::to_string(device) + "): " + hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

inline int launch_status(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error(std::string(what) + ": launch failed: " + hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

// Material + quadrature constants of one energy evaluation (kernel argument).
struct Tri3Consts {
    double c11, c12, c22, c33;   // plane-stress C, /root/reference/src/loss.py:29-32
    double W;                    // sum of triangle weights
    double Bk[6];                // body-force table [3][2]
};

// 64-lane wavefront sum (gfx950: wave64).  Result valid in lane 0.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// 64-lane wavefront minimum.  Result valid in lane 0.
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_down(v, off, 64));
    return v;
}

// DPP control of v_mov_b32_dpp: row_shl:N -- within a row of 16 lanes, lane i reads lane i + N (lanes past the row read 0).
constexpr int kDppRowShl = 0x100;
template <int N> __device__ __forceinline__ double row_shl(double v) {
    return __hiloint2double(__builtin_amdgcn_update_dpp(0, __double2hiint(v), kDppRowShl + N, 0xF, 0xF, true),
                            __builtin_amdgcn_update_dpp(0, __double2loint(v), kDppRowShl + N, 0xF, 0xF, true));
}

// wave_sum without the LDS unit (__shfl_down is ds_bpermute_b32: six dependent LDS round trips, queued behind whatever the
// wave has in flight there).  Lane 0's association tree is wave_sum's -- v[i] + v[i+32], then +16, +8, +4, +2, +1 -- so its
// result has the same bits; the other lanes hold garbage.  v_permlane32_swap / v_permlane16_swap of a register with its own
// copy leave "mine" in one result and "lane + 32" / "lane + 16" in the other (lanes 0-31 / rows 0 and 2); below a row of 16
// lanes, DPP row_shl.
__device__ __forceinline__ double wave_sum_valu(double v) {
    unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
    {
        const auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
        const auto b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        v = __hiloint2double((int)b[0], (int)a[0]) + __hiloint2double((int)b[1], (int)a[1]);
        lo = (unsigned)__double2loint(v); hi = (unsigned)__double2hiint(v);
    }
    {
        const auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
        const auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        v = __hiloint2double((int)b[0], (int)a[0]) + __hiloint2double((int)b[1], (int)a[1]);
    }
    v += row_shl<8>(v);
    v += row_shl<4>(v);
    v += row_shl<2>(v);
    v += row_shl<1>(v);
    return v;
}

// Block sum; `scratch` holds >= blockDim.x/64 doubles in LDS.  Result in thread 0.
__device__ __forceinline__ double block_sum(double v, double *scratch) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    v = wave_sum(v);
    if (lane == 0) scratch[wid] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) {
        const int nw = (blockDim.x + 63) >> 6;
        for (int w = 0; w < nw; ++w) r += scratch[w];   // fixed order: deterministic
    }
    return r;
}

// 1/x to ~1 ulp: hardware v_rcp_f64 seed + two Newton steps (4 FMAs) instead of the ~15-instruction
// IEEE division sequence.  det of a non-degenerate element is far from the denormal range; for
// det = 0 the result is inf/NaN like the division (NaN/Inf propagate, as upstream).
__device__ __forceinline__ double fast_rcp(double x) {
    double r = __builtin_amdgcn_rcp(x);
    double e = __builtin_fma(-x, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-x, r, 1.0);
    r = __builtin_fma(r, e, r);
    return r;
}

// One TRI3 element: energy density terms and (optionally) the 12 gradient
// entries.  Closed forms of SURVEY section 8a; they restate
//   J = [[x0-x2, x1-x2],[y0-y2, y1-y2]], detJ, Jinv      src/models.py:336-343
//   dN_dx = Jinv * dN_dxi  (reference convention, F4)    src/models.py:347-351
//   grad_u = sum_a U_a (x) dN_dx[:,a] = G Jinv^T          src/models.py:355
//   eps, sigma = C eps, psi = 1/2 eps.sigma               src/loss.py:66-77
//   e = abs(detJ) (W psi - sum_k U_k.B_k)                 src/loss.py:80-88
// and the hand-derived backward w.r.t. U (gu[k][i]) and X (gx[k][i]).
// HASB = false compiles the body-force table out (B_k = 0: the reference's default, loss.py:43-45).
//
// Operation count (fp64, HASB = false): 73 + one v_rcp_f64.  Two identities keep it low:
//   * a,b,c,d are pre-scaled by 1/det once (ai..di); H and dL/dG then need no trailing multiply;
//   * sum_ij P_ij H_ij = A W (eps . sigma) = 2 A W psi, and A/det = sign(det), so
//     dL/d(det) = sign(det) (W psi - beta) - 2 W sign(det) psi = -sign(det) (W psi + beta).
//
// PHYS = true: the opt-in "physical" gradient convention, grad_u = G Jinv (dN_dx = Jinv^T dN_dxi; exact for linear
// fields, invariant to the local node order) instead of the reference's G Jinv^T.  With
// J = [[a, b], [c, d]]: Jinv = [[d, -b], [-c, a]] / det, so E_phys(a, b, c, d) = E_ref(a, c, b, d) -- the same code
// with b and c swapped on the way in and dL/db, dL/dc swapped on the way out (det is symmetric in the swap).
template <bool GRAD, bool HASB = true, bool PHYS = false>
__device__ __forceinline__ double tri3_element(const double2 X0, const double2 X1, const double2 X2,
                                               const double2 U0, const double2 U1, const double2 U2,
                                               const Tri3Consts &k, double2 (&gx)[3], double2 (&gu)[3]) {
    const double a = X0.x - X2.x, d = X1.y - X2.y;
    const double b = PHYS ? X0.y - X2.y : X1.x - X2.x, c = PHYS ? X1.x - X2.x : X0.y - X2.y;
    const double det = a * d - b * c;
    const double inv = fast_rcp(det);
    const double ai = a * inv, bi = b * inv, ci = c * inv, di = d * inv;      // rows of Jinv (up to sign/placement)
    const double g0x = U0.x - U2.x, g0y = U0.y - U2.y;
    const double g1x = U1.x - U2.x, g1y = U1.y - U2.y;
    const double h00 = g0x * di - g1x * bi, h01 = g1x * ai - g0x * ci;      // H = G Jinv^T (reference convention, F4)
    const double h10 = g0y * di - g1y * bi, h11 = g1y * ai - g0y * ci;
    const double gam = h01 + h10;
    const double sxx = k.c11 * h00 + k.c12 * h11;
    const double syy = k.c12 * h00 + k.c22 * h11;
    const double sxy = k.c33 * gam;
    const double hs = h00 * sxx + h11 * syy + gam * sxy;                      // h : sigma = 2 psi
    // |det| and sign(det) enter only through sW = W sign(det) (one v_bfi on the high word): A W = det sW,
    // A W psi = (det sW / 2) hs, -sign(det) W psi = (-sW / 2) hs.  No compare / select chain (round-2 VALU trimming).
    const double sW = __builtin_copysign(k.W, det);
    const double aw = det * sW;                                               // A W
    double e = (0.5 * aw) * hs;                                               // A W psi
    double beta = 0.0, A = 0.0, sgn = 0.0;
    if (HASB) {
        A = fabs(det);
        sgn = __builtin_copysign(1.0, det);
        beta = U0.x * k.Bk[0] + U0.y * k.Bk[1] + U1.x * k.Bk[2] + U1.y * k.Bk[3] + U2.x * k.Bk[4] + U2.y * k.Bk[5];
        e -= A * beta;
    }
    if (GRAD) {
        const double p00 = aw * sxx, p01 = aw * sxy, p11 = aw * syy;         // P = dL/dH (P10 = P01)
        const double dg0x = p00 * di - p01 * ci, dg0y = p01 * di - p11 * ci;
        const double dg1x = p01 * ai - p00 * bi, dg1y = p11 * ai - p01 * bi;
        if (HASB) {
            gu[0] = make_double2(dg0x - A * k.Bk[0], dg0y - A * k.Bk[1]);
            gu[1] = make_double2(dg1x - A * k.Bk[2], dg1y - A * k.Bk[3]);
            gu[2] = make_double2(-(dg0x + dg1x) - A * k.Bk[4], -(dg0y + dg1y) - A * k.Bk[5]);
        } else {
            gu[0] = make_double2(dg0x, dg0y);
            gu[1] = make_double2(dg1x, dg1y);
            gu[2] = make_double2(-dg0x - dg1x, -dg0y - dg1y);
        }
        const double q = sW;                                                  // W sign(det) = A W / det
        double ddet = (-0.5 * sW) * hs;                                       // -sign(det) W psi
        if (HASB) ddet -= sgn * beta;                                         // -sign(det) (W psi + beta)
        const double da = q * (sxy * g1x + syy * g1y) + ddet * d;
        const double db = -q * (sxx * g1x + sxy * g1y) - ddet * c;
        const double dc = -q * (sxy * g0x + syy * g0y) - ddet * b;
        const double dd = q * (sxx * g0x + sxy * g0y) + ddet * a;
        gx[0] = PHYS ? make_double2(da, db) : make_double2(da, dc);       // (dL/dx0, dL/dy0): y0 enters through c (b if PHYS)
        gx[1] = PHYS ? make_double2(dc, dd) : make_double2(db, dd);
        gx[2] = PHYS ? make_double2(-da - dc, -db - dd) : make_double2(-da - db, -dc - dd);
    }
    return e;
}

// One Neumann edge (i,j): work ds*m and gradient of (-work).   src/loss.py:91-110,
// src/models.py:359-376.  t = {Ti.x, Ti.y, Tj.x, Tj.y}.
template <bool GRAD>
__device__ __forceinline__ double edge2_element(const double2 Xi, const double2 Xj, const double2 Ui,
                                                const double2 Uj, const double4 t, double2 (&gx)[2],
                                                double2 (&gu)[2]) {
    const double rx = Xj.x - Xi.x, ry = Xj.y - Xi.y;
    const double ds = sqrt(rx * rx + ry * ry);
    const double m = Ui.x * t.x + Ui.y * t.y + Uj.x * t.z + Uj.y * t.w;
    if (GRAD) {
        gu[0] = make_double2(-ds * t.x, -ds * t.y);
        gu[1] = make_double2(-ds * t.z, -ds * t.w);
        const double f = m / ds;
        gx[0] = make_double2(f * rx, f * ry);
        gx[1] = make_double2(-f * rx, -f * ry);
    }
    return ds * m;
}

}  // namespace hfem
