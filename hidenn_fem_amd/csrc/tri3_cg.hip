// Frozen-mesh displacement solve on TRI3, gfx950 (MI355X): matrix-free preconditioned conjugate gradients over the paired
// owner-computes tile plan (hidenn_fem_amd/solve.py).  The PCG driver at the end of this file also runs QUAD4 plans: the
// vector kernels, the status record and the halt logic know nothing of the element, and the two element kernels of a QUAD4
// solve (apply, block diagonal) are quad4_cg.hip's, reached through hfem_cg_dev.h.
//
// At fixed coordinates the total potential is exactly quadratic in u: E(u) = 1/2 u^T K u - f^T u.  So K p is the u-half of
// the energy gradient at u = p with no forces (tri3_element<GRAD, HASB = false>: the same closed forms, both gradient
// conventions), and the residual r = -dE/du comes from the graded energy kernel itself (hfem_tri3_energy_plan, called by
// the host once per solve).  Three kernels here:
//   tri3_cg_apply_kernel  q = K p on the free u rows: the pair kernel's gather, slot loop and LDS accumulation with the
//                         coordinate cotangent, the forces and the edges dropped.  Fused p-update: every node it gathers forms
//                         p = z + beta p_old on the fly; the tile that owns a row stores p to the OTHER buffer of a ping-pong
//                         pair (tiles still gathering read p_old as halo).  One partial of p^T q per tile (2 x the strain
//                         energy of p over its home elements); the last workgroup (ticket) sums them in tile order and
//                         writes alpha = rho / p^T q.
//   tri3_cg_diag_kernel   2x2 diagonal blocks of K (block Jacobi), once per refresh: per corner a of every element the
//                         block d2E/du_a^2 = the element gradient at u = unit vector at a, accumulated into the owner node.
//   tri3_cg_vec_kernel    u += alpha p, r -= alpha q, z = D^-1 r, partials of r^T z and r^T r; the last workgroup sums them
//                         in block order, forms beta, and applies the stopping test (START: r = -g0, z = D^-1 r, |f|).
// Two launches per iteration; every scalar is reduced on the device in a fixed order (bit-reproducible given q; q itself
// carries the LDS atomics' run-to-run last bits).  Once the status record says halted (converged, max_iter, breakdown) every
// later launch returns at once: iterations replayed behind the last one do nothing.
// precond = AMG (hfem_cg_start_amg / hfem_cg_iterate_amg): the vector kernel's JACOBI = false instance (the update without z),
// the V-cycle of tri3_amg.hip (z = M r) and tri3_cg_rz_kernel (rho = r^T z, beta) replace it: four launch groups per iteration.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>

#include "hfem_amg.h"
#include "hfem_cg_dev.h"
#include "hfem_device.h"
#include "hfem_plan_dev.h"

namespace hfem {
namespace {

constexpr int kVecBlock = 256, kVecMaxBlocks = 1024;

// ---------------------------------------------------------------- q = K p
// st != NULL: an iteration (p = z + beta p_old gathered, p stored to the other ping-pong buffer, alpha written);
// st == NULL: the standalone apply (p = z as given, pq_out[0] = p^T q).
template <int BLOCK, int NPT, int EPT, bool PHYS>
__global__ __launch_bounds__(BLOCK) void tri3_cg_apply_kernel(
    PlanDev pd, int n_tiles, const double2 *__restrict__ x_free, const double2 *__restrict__ x_fixed,
    const double2 *__restrict__ z, double2 *pbuf0, double2 *pbuf1, double2 *__restrict__ q, Tri3Consts k,
    double *__restrict__ partials, unsigned *ticket, double *st, double *host, double *pq_out, int cap_nodes, int cap_owned,
    int col_stride) {
    extern __shared__ double2 lds[];
    double2 *nd_xy = lds, *nd_p = lds + cap_nodes;
    double *acc0 = reinterpret_cast<double *>(lds + 2 * cap_nodes), *acc1 = acc0 + cap_owned;
    double *red = acc1 + cap_owned;                         // BLOCK / 64 doubles + one flag word
    const int tid = threadIdx.x;
    if (st && st[kHalted] != 0.0) return;                   // uniform over the grid: nothing is written after a halt
    double beta = 0.0;
    const double2 *p_old = nullptr;
    double2 *p_new = nullptr;
    if (st) {
        const int par = ((long long)st[kIter]) & 1;
        beta = st[kBeta];
        p_old = par ? pbuf1 : pbuf0;
        p_new = par ? pbuf0 : pbuf1;
    }
    const int slot = xcd_tile((int)blockIdx.x, (int)gridDim.x);
    int2 s[NPT];
    const int2 *src = pd.node_src + (size_t)slot * pd.node_stride;
#pragma unroll
    for (int j = 0; j < NPT; ++j) s[j] = src[min(tid + j * BLOCK, pd.node_stride - 1)];
    const TileDesc d = pd.tiles[slot];
    uint32_t w0[EPT], w1[EPT];
    const size_t rec0 = (size_t)slot * pd.elem_stride;
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const size_t i = rec0 + min(tid + j * col_stride, pd.elem_stride - 1);
        w0[j] = pd.elem_pack[i];
        w1[j] = pd.elem_pack_hi[i];
    }
    // gather: coordinates through the x row map, p through the u row map (fixed u rows are 0)
    double2 vx[NPT], vp[NPT];
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        vx[j] = s[j].x >= 0 ? x_free[s[j].x] : x_fixed[~s[j].x];
        vp[j] = make_double2(0.0, 0.0);
        if (s[j].y >= 0) {
            vp[j] = z[s[j].y];
            if (p_old) {
                const double2 o = p_old[s[j].y];
                vp[j].x = __builtin_fma(beta, o.x, vp[j].x);
                vp[j].y = __builtin_fma(beta, o.y, vp[j].y);
            }
        }
    }
    const int n_owned = d.n_owned;
#pragma unroll
    for (int j = 0; j < EPT; ++j)
        if (!(tid < col_stride && tid + j * col_stride < d.n_elem)) { w0[j] = kSkipBit; w1[j] = 0u; }
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int l = tid + j * BLOCK;
        if (l < d.n_node) { nd_xy[l] = vx[j]; nd_p[l] = vp[j]; }
        if (l < n_owned) { acc0[l] = 0.0; acc1[l] = 0.0; }
    }
    __syncthreads();
    auto add_row = [&](int l, const double2 g) {
        unsafeAtomicAdd(&acc0[l], g.x);
        unsafeAtomicAdd(&acc1[l], g.y);
    };
    double e_loc = 0.0;
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const uint32_t a = w0[j], b = w1[j];
        if (!(a & kSkipBit)) {
            const int ln = (int)(a & kLocalMask), lb = (int)((a >> kLocalBits) & kLocalMask),
                      lc = (int)((a >> (2 * kLocalBits)) & kLocalMask);
            const double2 Xn = nd_xy[ln], Pn = nd_p[ln], Xc = nd_xy[lc], Pc = nd_p[lc];
            double2 sn, sc;
            {
                double2 gx[3], gu[3];
                const double e = tri3_element<true, false, PHYS>(Xn, nd_xy[lb], Xc, Pn, nd_p[lb], Pc, k, gx, gu);
                if (a & kHomeBit) e_loc += e;
                if (lb < n_owned) add_row(lb, gu[1]);
                sn = gu[0]; sc = gu[2];
            }
            if (b & kHasBBit) {                             // B = (n, c, d)
                const int ld = (int)(b & kLocalMask);
                double2 gx[3], gu[3];
                const double e = tri3_element<true, false, PHYS>(Xn, Xc, nd_xy[ld], Pn, Pc, nd_p[ld], k, gx, gu);
                if (b & kHomeBBit) e_loc += e;
                if (ld < n_owned) add_row(ld, gu[2]);
                sn.x += gu[0].x; sn.y += gu[0].y; sc.x += gu[1].x; sc.y += gu[1].y;
            }
            if (ln < n_owned) add_row(ln, sn);
            if (lc < n_owned) add_row(lc, sc);
        }
    }
    {
        const double w = wave_sum(e_loc);
        if ((tid & 63) == 0) red[tid >> 6] = w;
    }
    __syncthreads();
    // owned free rows: q, and (iterations) the new p into the other buffer
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int l = tid + j * BLOCK;
        if (l < n_owned && s[j].y >= 0) {
            q[s[j].y] = make_double2(acc0[l], acc1[l]);
            if (p_new) p_new[s[j].y] = nd_p[l];
        }
    }
    if (tid == 0) {
        double tile_e = 0.0;
#pragma unroll
        for (int w = 0; w < BLOCK / 64; ++w) tile_e += red[w];
        put_partial(partials + slot, 2.0 * tile_e);         // p^T K_tile p over the home elements
    }
    if (!last_block(ticket, (unsigned)n_tiles, reinterpret_cast<int *>(red + BLOCK / 64))) return;
    const double pq = ordered_sum<BLOCK>(partials, n_tiles, red);
    if (tid == 0) {
        if (!st) {
            pq_out[0] = pq;
            return;
        }
        const double alpha = st[kRho] / pq;
        st[kPq] = pq;
        st[kAlpha] = alpha;
        if (!(pq > 0.0) || !isfinite(alpha)) {              // K not positive definite on p, or a non-finite scalar
            st[kHalted] = 1.0;
            st[kReason] = kBreakdown;
            publish(st, host);
        }
    }
}

// ---------------------------------------------------------------- block-Jacobi setup
template <int BLOCK, int NPT, int EPT, bool PHYS>
__global__ __launch_bounds__(BLOCK) void tri3_cg_diag_kernel(PlanDev pd, const double2 *__restrict__ x_free,
                                                             const double2 *__restrict__ x_fixed, Tri3Consts k,
                                                             double *__restrict__ diag, double *__restrict__ dinv, int precond,
                                                             int cap_nodes, int cap_owned, int col_stride) {
    extern __shared__ double2 lds[];
    double2 *nd_xy = lds;
    double *acc0 = reinterpret_cast<double *>(lds + cap_nodes), *acc1 = acc0 + cap_owned, *acc2 = acc1 + cap_owned;
    const int tid = threadIdx.x;
    const int slot = (int)blockIdx.x;
    int2 s[NPT];
    const int2 *src = pd.node_src + (size_t)slot * pd.node_stride;
#pragma unroll
    for (int j = 0; j < NPT; ++j) s[j] = src[min(tid + j * BLOCK, pd.node_stride - 1)];
    const TileDesc d = pd.tiles[slot];
    const int n_owned = d.n_owned;
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int l = tid + j * BLOCK;
        if (l < d.n_node) nd_xy[l] = s[j].x >= 0 ? x_free[s[j].x] : x_fixed[~s[j].x];
        if (l < n_owned) { acc0[l] = 0.0; acc1[l] = 0.0; acc2[l] = 0.0; }
    }
    __syncthreads();
    const double2 o = make_double2(0.0, 0.0), ex = make_double2(1.0, 0.0), ey = make_double2(0.0, 1.0);
    // the three corner blocks of one element: column c of K_aa = the gradient at u_a = e_c, u_b = 0 (b != a)
    auto element = [&](int l0, int l1, int l2) {
        const int ls[3] = {l0, l1, l2};
        const double2 X0 = nd_xy[l0], X1 = nd_xy[l1], X2 = nd_xy[l2];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (ls[a] >= n_owned) continue;
            double2 gx[3], gu[3], hu[3];
            tri3_element<true, false, PHYS>(X0, X1, X2, a == 0 ? ex : o, a == 1 ? ex : o, a == 2 ? ex : o, k, gx, gu);
            tri3_element<true, false, PHYS>(X0, X1, X2, a == 0 ? ey : o, a == 1 ? ey : o, a == 2 ? ey : o, k, gx, hu);
            unsafeAtomicAdd(&acc0[ls[a]], gu[a].x);
            unsafeAtomicAdd(&acc1[ls[a]], 0.5 * (gu[a].y + hu[a].x));
            unsafeAtomicAdd(&acc2[ls[a]], hu[a].y);
        }
    };
    for (int j = 0; j < EPT; ++j) {
        if (!(tid < col_stride && tid + j * col_stride < d.n_elem)) continue;
        const size_t i = (size_t)slot * pd.elem_stride + tid + j * col_stride;
        const uint32_t a = pd.elem_pack[i], b = pd.elem_pack_hi[i];
        if (a & kSkipBit) continue;
        const int ln = (int)(a & kLocalMask), lb = (int)((a >> kLocalBits) & kLocalMask),
                  lc = (int)((a >> (2 * kLocalBits)) & kLocalMask);
        element(ln, lb, lc);
        if (b & kHasBBit) element(ln, lc, (int)(b & kLocalMask));
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int l = tid + j * BLOCK;
        if (l < n_owned && s[j].y >= 0) {
            const size_t r = (size_t)s[j].y * 3;
            const double a = acc0[l], b = acc1[l], c = acc2[l];
            if (diag) { diag[r] = a; diag[r + 1] = b; diag[r + 2] = c; }
            const double det = a * c - b * b;
            if (precond && det > 0.0 && isfinite(det)) {
                const double inv = 1.0 / det;
                dinv[r] = c * inv; dinv[r + 1] = -b * inv; dinv[r + 2] = a * inv;
            } else {                                        // "none", or a block that is not positive definite
                dinv[r] = 1.0; dinv[r + 1] = 0.0; dinv[r + 2] = 1.0;
            }
        }
    }
}

// ---------------------------------------------------------------- vector update + scalars
// Thread 0 of the last workgroup, rho step: beta = rho / rho_old (0 on the first direction), rho; true on a non-finite one.
__device__ __forceinline__ bool rho_step(double *st, double rho) {
    const double beta = st[kIter] == 0.0 ? 0.0 : rho / st[kRho];
    st[kBeta] = beta;
    st[kRho] = rho;
    return !isfinite(rho) || !isfinite(beta);
}

// Residual step: the START reset of the record (|f|, tolerance, max_iter, rtol-wins) or one more iteration, the rho step when
// this launch also formed rho (JACOBI), |r|, and the halt decision: breakdown before a met tolerance before max_iter.
template <bool START, bool JACOBI>
__device__ __forceinline__ void residual_step(double *st, double *host, double rho, double r2, double f2, double rtol,
                                              double atol, double max_iter) {
    const double rnorm = sqrt(r2);
    int reason = kRunning;
    if (START) {
        for (int i = 0; i < kStatusN; ++i) st[i] = 0.0;
        st[kFnorm] = sqrt(f2);
        st[kTol] = fmax(rtol * st[kFnorm], atol);
        st[kMaxIter] = max_iter;
        st[kRtolWins] = rtol * st[kFnorm] >= atol ? 1.0 : 0.0;
    } else {
        st[kIter] += 1.0;
    }
    const bool bad = JACOBI && rho_step(st, rho);
    st[kRnorm] = rnorm;
    if (bad || !isfinite(rnorm)) reason = kBreakdown;
    else if (rnorm <= st[kTol]) reason = st[kRtolWins] != 0.0 ? kRtol : kAtol;
    else if (st[kIter] >= st[kMaxIter]) reason = kMaxIterHit;
    if (reason != kRunning) {
        st[kHalted] = 1.0;
        st[kReason] = reason;
    }
    publish(st, host);
}

// JACOBI: the whole update with z = D^-1 r and rho fused.  Otherwise (precond = AMG) the update without z: z = M r comes from
// the V-cycle after this launch, rho = r^T z and beta from tri3_cg_rz_kernel after that.
template <bool START, bool JACOBI>
__global__ __launch_bounds__(kVecBlock) void tri3_cg_vec_kernel(
    int64_t n, double2 *__restrict__ u, double2 *__restrict__ r, double2 *__restrict__ z, const double2 *pbuf0,
    const double2 *pbuf1, const double2 *__restrict__ q, const double *__restrict__ dinv, const double2 *__restrict__ g0,
    const double2 *__restrict__ gzero, double *__restrict__ part, unsigned *ticket, double *st, double *host, double rtol,
    double atol, double max_iter) {
    __shared__ double red[kVecBlock / 64 + 1];
    const int tid = threadIdx.x;
    const int nb = (int)gridDim.x;
    if (!START && st[kHalted] != 0.0) return;
    double alpha = 0.0;
    const double2 *p = nullptr;
    if (!START) {
        alpha = st[kAlpha];
        p = (((long long)st[kIter]) & 1) ? pbuf0 : pbuf1;    // the buffer this iteration's apply stored p to
    }
    double rz = 0.0, rr = 0.0, ff = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kVecBlock + tid; i < n; i += (int64_t)nb * kVecBlock) {
        double2 ri;
        if (START) {
            const double2 g = g0[i], h = gzero[i];
            ri = make_double2(-g.x, -g.y);
            ff += h.x * h.x + h.y * h.y;
        } else {
            const double2 pi = p[i], qi = q[i];
            double2 ui = u[i];
            ri = r[i];
            ui.x = __builtin_fma(alpha, pi.x, ui.x); ui.y = __builtin_fma(alpha, pi.y, ui.y);
            ri.x = __builtin_fma(-alpha, qi.x, ri.x); ri.y = __builtin_fma(-alpha, qi.y, ri.y);
            u[i] = ui;
        }
        r[i] = ri;
        if constexpr (JACOBI) {
            const double d0 = dinv[3 * i], d1 = dinv[3 * i + 1], d2 = dinv[3 * i + 2];
            const double2 zi = make_double2(d0 * ri.x + d1 * ri.y, d1 * ri.x + d2 * ri.y);
            z[i] = zi;
            rz += ri.x * zi.x + ri.y * zi.y;
        }
        rr += ri.x * ri.x + ri.y * ri.y;
    }
    const double s_rz = JACOBI ? block_sum(rz, red) : 0.0;
    if (JACOBI) __syncthreads();
    const double s_rr = block_sum(rr, red);
    __syncthreads();
    const double s_ff = START ? block_sum(ff, red) : 0.0;
    if (tid == 0) {
        if constexpr (JACOBI) put_partial(part + blockIdx.x, s_rz);
        put_partial(part + nb + blockIdx.x, s_rr);
        put_partial(part + 2 * nb + blockIdx.x, s_ff);
    }
    if (!last_block(ticket, (unsigned)nb, reinterpret_cast<int *>(red + kVecBlock / 64))) return;
    const double rho = JACOBI ? ordered_sum<kVecBlock>(part, nb, red) : 0.0;
    if (JACOBI) __syncthreads();
    const double r2 = ordered_sum<kVecBlock>(part + nb, nb, red);
    __syncthreads();
    const double f2 = START ? ordered_sum<kVecBlock>(part + 2 * nb, nb, red) : 0.0;
    if (tid == 0) residual_step<START, JACOBI>(st, host, rho, r2, f2, rtol, atol, max_iter);
}

// rho = r^T z in block order, then the rho step
__global__ __launch_bounds__(kVecBlock) void tri3_cg_rz_kernel(int64_t n, const double2 *__restrict__ r,
                                                               const double2 *__restrict__ z, double *__restrict__ part,
                                                               unsigned *ticket, double *st, double *host) {
    __shared__ double red[kVecBlock / 64 + 1];
    const int tid = threadIdx.x;
    const int nb = (int)gridDim.x;
    if (st[kHalted] != 0.0) return;
    double rz = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kVecBlock + tid; i < n; i += (int64_t)nb * kVecBlock) {
        const double2 ri = r[i], zi = z[i];
        rz += ri.x * zi.x + ri.y * zi.y;
    }
    const double s_rz = block_sum(rz, red);
    if (tid == 0) put_partial(part + blockIdx.x, s_rz);
    if (!last_block(ticket, (unsigned)nb, reinterpret_cast<int *>(red + kVecBlock / 64))) return;
    const double rho = ordered_sum<kVecBlock>(part, nb, red);
    if (tid != 0) return;
    if (rho_step(st, rho)) {
        st[kHalted] = 1.0;
        st[kReason] = kBreakdown;
    }
    publish(st, host);
}

}  // namespace
}  // namespace hfem

// ---------------------------------------------------------------- host side
struct hfem_cg {
    hfem_plan *plan = nullptr;
    int device = -1;
    int64_t n_u = 0;
    int n_tiles = 0, block = 256, vec_blocks = 1;
    bool phys = false, quad = false;   // quad: a QUAD4 plan (one element per slot; kernels of quad4_cg.hip)
    size_t lds_apply = 0, lds_diag = 0;
    // device memory, one allocation: p[2], r, z, q (double2 rows), dinv (3 doubles per row), tile partials, vector partials,
    // status record, tickets
    char *mem = nullptr;
    double2 *p[2] = {nullptr, nullptr}, *r = nullptr, *z = nullptr, *q = nullptr;
    double *dinv = nullptr, *tile_part = nullptr, *vec_part = nullptr, *st = nullptr;
    unsigned *tickets = nullptr;       // [0] apply, [1] vector kernels, [2] standalone apply
    double *host = nullptr;            // pinned mirror of the status record
    // bound by hfem_cg_setup
    const double2 *x_free = nullptr, *x_fixed = nullptr;
    hfem::Tri3Consts k{};
    bool ready = false;
};

namespace {
using hfem::PlanDev;

template <int BLOCK, int NPT, int EPT>
void launch_apply(const hfem_cg *c, const double2 *z, double2 *q, unsigned *ticket, double *st, double *host, double *pq_out,
                  hipStream_t s) {
    const hfem::HostPlan &h = c->plan->host;
    const PlanDev pd = hfem::plan_dev(c->plan);
#define HFEM_CG_APPLY(PH)                                                                                                    \
    hipLaunchKernelGGL((hfem::tri3_cg_apply_kernel<BLOCK, NPT, EPT, PH>), dim3(c->n_tiles), dim3(BLOCK), c->lds_apply, s, pd, \
                       c->n_tiles, c->x_free, c->x_fixed, z, c->p[0], c->p[1], q, c->k, c->tile_part, ticket, st, host, pq_out, \
                       h.max_nodes, h.max_owned, h.col_stride)
    if (c->phys) HFEM_CG_APPLY(true);
    else HFEM_CG_APPLY(false);
#undef HFEM_CG_APPLY
}

template <int BLOCK, int NPT, int EPT>
void launch_diag(const hfem_cg *c, double *diag, int precond, hipStream_t s) {
    const hfem::HostPlan &h = c->plan->host;
    const PlanDev pd = hfem::plan_dev(c->plan);
#define HFEM_CG_DIAG(PH)                                                                                                     \
    hipLaunchKernelGGL((hfem::tri3_cg_diag_kernel<BLOCK, NPT, EPT, PH>), dim3(c->n_tiles), dim3(BLOCK), c->lds_diag, s, pd,   \
                       c->x_free, c->x_fixed, c->k, diag, c->dinv, precond, h.max_nodes, h.max_owned, h.col_stride)
    if (c->phys) HFEM_CG_DIAG(true);
    else HFEM_CG_DIAG(false);
#undef HFEM_CG_DIAG
}

hfem::Quad4CgArgs quad4_args(const hfem_cg *c, size_t lds, hipStream_t s) {
    hfem::Quad4CgArgs A;
    A.plan = c->plan; A.n_tiles = c->n_tiles; A.phys = c->phys; A.x_free = c->x_free; A.x_fixed = c->x_fixed; A.k = c->k;
    A.lds = lds; A.s = s;
    return A;
}

// the tile shapes of a paired plan: 512 threads (2 nodes and 2 slot rows per thread), or 256 threads with 3 | 4 nodes and
// 3 | 4 | 6 slot rows per thread (the pair kernel's matrix: a masked row or node costs a full pass of the slot loop)
void cg_apply(const hfem_cg *c, const double2 *z, double2 *q, unsigned *ticket, double *st, double *host, double *pq_out,
              hipStream_t s) {
    const hfem::HostPlan &h = c->plan->host;
    if (c->quad) {
        hfem::launch_quad4_cg_apply(quad4_args(c, c->lds_apply, s), z, c->p[0], c->p[1], q, c->tile_part, ticket, st, host, pq_out);
        return;
    }
#define HFEM_CG_A(NPT, EPT) launch_apply<256, NPT, EPT>(c, z, q, ticket, st, host, pq_out, s)
    if (c->block == 512) launch_apply<512, 2, 2>(c, z, q, ticket, st, host, pq_out, s);
    else if (h.max_nodes <= 3 * 256) {
        if (h.max_rows <= 3) HFEM_CG_A(3, 3);
        else if (h.max_rows == 4) HFEM_CG_A(3, 4);
        else HFEM_CG_A(3, 6);
    } else {
        if (h.max_rows <= 3) HFEM_CG_A(4, 3);
        else if (h.max_rows == 4) HFEM_CG_A(4, 4);
        else HFEM_CG_A(4, 6);
    }
#undef HFEM_CG_A
}

void cg_rz(const hfem_cg *c, hipStream_t s) {
    hipLaunchKernelGGL(hfem::tri3_cg_rz_kernel, dim3(c->vec_blocks), dim3(hfem::kVecBlock), 0, s, c->n_u, c->r, c->z,
                       c->vec_part, c->tickets + 1, c->st, c->host);
}

// amg == nullptr: block Jacobi, z and rho fused into the vector launch; otherwise z = M r (the V-cycle) and rho follow it
template <bool START>
void cg_vec(const hfem_cg *c, const hfem_amg *amg, double2 *u, const double2 *g0, const double2 *gzero, double rtol, double atol,
            double max_iter, hipStream_t s) {
#define HFEM_CG_VEC(J)                                                                                                       \
    hipLaunchKernelGGL((hfem::tri3_cg_vec_kernel<START, J>), dim3(c->vec_blocks), dim3(hfem::kVecBlock), 0, s, c->n_u, u, c->r, \
                       c->z, c->p[0], c->p[1], c->q, c->dinv, g0, gzero, c->vec_part, c->tickets + 1, c->st, c->host, rtol,  \
                       atol, max_iter)
    if (!amg) HFEM_CG_VEC(true);
    else {
        HFEM_CG_VEC(false);
        hfem::amg_cycle(amg, (const double *)c->r, (double *)c->z, c->st, s);
        cg_rz(c, s);
    }
#undef HFEM_CG_VEC
}

// The PCG driver behind both pairs of entry points, which check the arguments.
int cg_start(hfem_cg *c, const hfem_amg *amg, const double *g0, const double *g_zero, double rtol, double atol, int64_t max_iter,
             hipStream_t s, const char *what) {
    if (int rc = hfem::use_device(c->device)) return rc;
    HFEM_HIP_CHECK(hipMemsetAsync(c->p[0], 0, 2 * (size_t)std::max<int64_t>(c->n_u, 1) * 16, s));   // p_old of iteration 0
    cg_vec<true>(c, amg, nullptr, (const double2 *)g0, (const double2 *)g_zero, rtol, atol, (double)max_iter, s);
    return hfem::launch_status(what);
}

int cg_iterate(hfem_cg *c, const hfem_amg *amg, double *u_free, int32_t n_iter, hipStream_t s, const char *what) {
    if (int rc = hfem::use_device(c->device)) return rc;
    for (int it = 0; it < n_iter; ++it) {                    // launch-only: capturable in one graph
        cg_apply(c, c->z, c->q, c->tickets, c->st, c->host, nullptr, s);
        cg_vec<false>(c, amg, (double2 *)u_free, nullptr, nullptr, 0.0, 0.0, 0.0, s);
    }
    return hfem::launch_status(what);
}

int check_amg(const hfem_cg *c, const hfem_amg *a) {
    HFEM_ARG_CHECK(c->ready, "hfem_cg_setup has not run");
    HFEM_ARG_CHECK(hfem::amg_ready(a), "hfem_amg_setup / hfem_amg_set_coarse have not run");
    HFEM_ARG_CHECK(hfem::amg_rows(a) == c->n_u, "the AMG hierarchy and the CG solve have different free rows");
    HFEM_ARG_CHECK(hfem::amg_device(a) == c->device, "the AMG hierarchy lives on another device");
    return 0;
}
}  // namespace

extern "C" int hfem_cg_create(hfem_plan *plan, int64_t n_u, int32_t flags, hfem_cg **out) {
    HFEM_ARG_CHECK(plan && out, "null pointer");
    *out = nullptr;
    HFEM_ARG_CHECK(plan->device >= 0, "host-only plan (created with device < 0) cannot launch");
    const hfem::HostPlan &h = plan->host;
    const bool quad = h.npe == 4;                            // QUAD4: the model's own plan, one element per slot, no pairing
    HFEM_ARG_CHECK(quad || (h.paired && plan->d_elem_pack_hi && h.n_chained == 0),
                   "the CG solve needs a paired-slot plan (plan_elem_order 5)");
    HFEM_ARG_CHECK(!quad || plan->d_elem_pack_hi, "QUAD4 plan without its fourth-corner records");
    HFEM_ARG_CHECK((flags & ~HFEM_FLAG_PHYSICAL_GRAD) == 0, "flags: only HFEM_FLAG_PHYSICAL_GRAD");
    const bool b512 = !quad && h.pair_block == 512;
    HFEM_ARG_CHECK(quad    ? (h.max_nodes <= 4 * 256 && h.max_elems <= 4 * 256)
                   : b512 ? (h.max_nodes <= 2 * 512 && h.max_rows <= 2)
                          : (h.max_nodes <= 4 * 256 && h.max_rows <= 6),
                   "tile shape outside the CG kernels' instances");
    HFEM_ARG_CHECK(!quad || h.max_owned <= h.max_nodes, "QUAD4 plan owns more rows than a tile holds");
    int64_t rows = 0;                                        // free u rows the plan's row maps address
    for (size_t i = 1; i < h.node_src.size(); i += 2) rows = std::max<int64_t>(rows, (int64_t)h.node_src[i] + 1);
    HFEM_ARG_CHECK(n_u >= rows, "n_u is smaller than the plan's free u rows");
    HFEM_ARG_CHECK(n_u < ((int64_t)1 << 31), "n_u too large");
    std::unique_ptr<hfem_cg> c(new hfem_cg);
    c->plan = plan; c->device = plan->device; c->n_u = n_u; c->phys = (flags & HFEM_FLAG_PHYSICAL_GRAD) != 0;
    c->quad = quad;
    c->n_tiles = (int)h.tiles.size(); c->block = b512 ? 512 : 256;
    c->vec_blocks = (int)std::max<int64_t>(1, std::min<int64_t>(hfem::kVecMaxBlocks, (n_u + hfem::kVecBlock - 1) / hfem::kVecBlock));
    c->lds_apply = (size_t)h.max_nodes * 32 + (size_t)h.max_owned * 16 + (c->block / 64 + 2) * 8;
    c->lds_diag = (size_t)h.max_nodes * 16 + (size_t)h.max_owned * 24;
    if (int rc = hfem::use_device(c->device)) return rc;
    const size_t rows16 = (size_t)std::max<int64_t>(n_u, 1) * 16;
    const size_t off_r = 2 * rows16, off_z = 3 * rows16, off_q = 4 * rows16, off_d = 5 * rows16;
    const size_t off_tp = off_d + (size_t)std::max<int64_t>(n_u, 1) * 24;
    const size_t off_vp = off_tp + (size_t)std::max(c->n_tiles, 1) * 8;
    const size_t off_st = off_vp + 3 * (size_t)hfem::kVecMaxBlocks * 8;
    const size_t off_tk = off_st + hfem::kStatusN * 8;
    const size_t bytes = off_tk + 64;
    HFEM_HIP_CHECK(hipMalloc((void **)&c->mem, bytes));
    if (hipHostMalloc((void **)&c->host, hfem::kStatusN * sizeof(double)) != hipSuccess) {
        (void)hipFree(c->mem);
        hfem::set_error("hfem_cg_create: hipHostMalloc failed");
        return 1;
    }
    for (int i = 0; i < hfem::kStatusN; ++i) c->host[i] = 0.0;
    c->p[0] = (double2 *)c->mem; c->p[1] = (double2 *)(c->mem + rows16);
    c->r = (double2 *)(c->mem + off_r); c->z = (double2 *)(c->mem + off_z); c->q = (double2 *)(c->mem + off_q);
    c->dinv = (double *)(c->mem + off_d); c->tile_part = (double *)(c->mem + off_tp); c->vec_part = (double *)(c->mem + off_vp);
    c->st = (double *)(c->mem + off_st); c->tickets = (unsigned *)(c->mem + off_tk);
    const hipError_t e = hipMemset(c->mem, 0, bytes);                 // tickets zero, p buffers zero (0 * p_old is 0)
    if (e != hipSuccess) {
        (void)hipFree(c->mem); (void)hipHostFree(c->host);
        hfem::set_error(std::string("hfem_cg_create: hipMemset -> ") + hipGetErrorString(e));
        return (int)e;
    }
    *out = c.release();
    return 0;
}

extern "C" int hfem_cg_destroy(hfem_cg *c) {
    if (!c) return 0;
    if (c->device >= 0) (void)hipSetDevice(c->device);
    if (c->mem) (void)hipFree(c->mem);
    if (c->host) (void)hipHostFree(c->host);
    delete c;
    return 0;
}

extern "C" int hfem_cg_setup(hfem_cg *c, const double *x_free, const double *x_fixed, const double mat[4], double W,
                             int32_t precond, double *diag_out, void *stream) {
    HFEM_ARG_CHECK(c && x_free && mat, "null pointer");
    HFEM_ARG_CHECK(precond == 0 || precond == 1, "precond: 0 none, 1 block Jacobi");
    bool fixed_rows = false;
    const hfem::HostPlan &h = c->plan->host;
    for (size_t i = 0; i < h.node_src.size(); i += 2) fixed_rows = fixed_rows || h.node_src[i] < 0;
    HFEM_ARG_CHECK(x_fixed || !fixed_rows, "the plan reads fixed coordinate rows: x_fixed must be given");
    if (int rc = hfem::use_device(c->device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    c->x_free = (const double2 *)x_free; c->x_fixed = (const double2 *)x_fixed;
    c->k = hfem::make_consts(mat, c->quad ? 1.0 : W, nullptr);   // QUAD4: the 2x2 rule's weights are 1 (hfem_quad4_energy_plan_ex)
    if (c->quad) hfem::launch_quad4_cg_diag(quad4_args(c, c->lds_diag, s), diag_out, c->dinv, precond);
    else if (c->block == 512) launch_diag<512, 2, 2>(c, diag_out, precond, s);
    else launch_diag<256, 4, 6>(c, diag_out, precond, s);
    if (int rc = hfem::launch_status("hfem_cg_setup")) return rc;
    c->ready = true;
    return 0;
}

extern "C" int hfem_cg_start(hfem_cg *c, const double *g0, const double *g_zero, double rtol, double atol, int64_t max_iter,
                             void *stream) {
    HFEM_ARG_CHECK(c && g0 && g_zero, "null pointer");
    HFEM_ARG_CHECK(c->ready, "hfem_cg_setup has not run");
    HFEM_ARG_CHECK(rtol >= 0.0 && atol >= 0.0 && max_iter >= 0, "rtol, atol and max_iter must be >= 0");
    return cg_start(c, nullptr, g0, g_zero, rtol, atol, max_iter, (hipStream_t)stream, __func__);
}

extern "C" int hfem_cg_iterate(hfem_cg *c, double *u_free, int32_t n_iter, void *stream) {
    HFEM_ARG_CHECK(c && (u_free || c->n_u == 0), "null pointer");
    HFEM_ARG_CHECK(c->ready, "hfem_cg_setup has not run");
    HFEM_ARG_CHECK(n_iter >= 0, "n_iter must be >= 0");
    return cg_iterate(c, nullptr, u_free, n_iter, (hipStream_t)stream, __func__);
}

extern "C" int hfem_cg_status(hfem_cg *c, double *status_host, void *stream) {
    HFEM_ARG_CHECK(c && status_host, "null pointer");
    if (int rc = hfem::use_device(c->device)) return rc;
    HFEM_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    for (int i = 0; i < hfem::kStatusN; ++i) status_host[i] = c->host[i];
    return 0;
}

extern "C" int hfem_cg_apply(hfem_cg *c, const double *p, double *q, double *pq_out, void *stream) {
    HFEM_ARG_CHECK(c && p && q && pq_out, "null pointer");
    HFEM_ARG_CHECK(c->ready, "hfem_cg_setup has not run");
    if (int rc = hfem::use_device(c->device)) return rc;
    cg_apply(c, (const double2 *)p, (double2 *)q, c->tickets + 2, nullptr, nullptr, pq_out, (hipStream_t)stream);
    return hfem::launch_status("hfem_cg_apply");
}

// ---------------------------------------------------------------- AMG-preconditioned PCG
extern "C" int hfem_cg_start_amg(hfem_cg *c, hfem_amg *amg, const double *g0, const double *g_zero, double rtol, double atol,
                                 int64_t max_iter, void *stream) {
    HFEM_ARG_CHECK(c && amg && g0 && g_zero, "null pointer");
    if (int rc = check_amg(c, amg)) return rc;
    HFEM_ARG_CHECK(rtol >= 0.0 && atol >= 0.0 && max_iter >= 0, "rtol, atol and max_iter must be >= 0");
    return cg_start(c, amg, g0, g_zero, rtol, atol, max_iter, (hipStream_t)stream, __func__);
}

extern "C" int hfem_cg_iterate_amg(hfem_cg *c, hfem_amg *amg, double *u_free, int32_t n_iter, void *stream) {
    HFEM_ARG_CHECK(c && amg && (u_free || c->n_u == 0), "null pointer");
    if (int rc = check_amg(c, amg)) return rc;
    HFEM_ARG_CHECK(n_iter >= 0, "n_iter must be >= 0");
    return cg_iterate(c, amg, u_free, n_iter, (hipStream_t)stream, __func__);
}
