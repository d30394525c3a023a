// PCG driver of the frozen-mesh displacement solve, gfx950 (MI355X) (hidenn_fem_amd/solve.py): everything above the element
// level -- the vector kernels, the status record, the halt logic and the hfem_cg_* entry points.  Nothing here knows the
// element: q = K p and the block-Jacobi blocks come from the element kernels of tri3_cg.hip (paired TRI3 plan), quad4_cg.hip
// (the model's own QUAD4 plan), tri3_hyper_cg.hip or quad4_hyper_cg.hip (the Neo-Hookean tangent at a linearisation point,
// on the one-element-per-slot TRI3 plan or the model's own QUAD4 plan: the inner solve of hidenn_fem_amd/newton.py), chosen in
// cg_apply and cg_diag.  The shifted operator c_K K + c_M M of a Newmark step (after hfem_cg_setup_shifted:
// hidenn_fem_amd/dynamics.py) and the element-scaled operator K(w) = sum_e w_e K_e (after hfem_cg_setup_scaled) are no element
// kinds of their own: they are the Mass and the Scaled instance of the kernels of tri3_cg.hip and quad4_cg.hip, picked by
// their launchers from the bound shifted flag and w_slot; likewise c_K K_T + c_M M of a finite-strain step (after
// hfem_cg_setup_hyper_shifted) is the MASS instance of the tangent kernels.  The residual r = -dE/du comes from the graded energy kernel, called by the host
// once per solve.
//   cg_vec_kernel   u += alpha p, r -= alpha q, z = D^-1 r, partials of r^T z and r^T r; the last workgroup sums them in block
//                   order, forms beta, and applies the stopping test (START: r = -g0, z = D^-1 r, |f|).
//   cg_rz_kernel    rho = r^T z in block order, then beta (precond = AMG only).
// Two launches per iteration (apply, vector); every scalar is reduced on the device in a fixed order (bit-reproducible given
// q; q itself carries the LDS atomics' run-to-run last bits).  Once the status record says halted (converged, max_iter,
// breakdown) every later launch returns at once: iterations replayed behind the last one do nothing.
// precond = AMG (hfem_cg_start_amg / hfem_cg_iterate_amg): the vector kernel's JACOBI = false instance (the update without z),
// the V-cycle of tri3_amg.hip (z = M r) and cg_rz_kernel (rho = r^T z, beta) replace it: four launch groups per iteration.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>

#include "hfem_amg.h"
#include "hfem_cg_dev.h"
#include "hfem_device.h"
#include "hfem_j2_dev.h"
#include "hfem_plan_dev.h"

namespace hfem {
namespace {

constexpr int kVecBlock = 256, kVecMaxBlocks = 1024;

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
// the V-cycle after this launch, rho = r^T z and beta from cg_rz_kernel after that.
template <bool START, bool JACOBI>
__global__ __launch_bounds__(kVecBlock) void cg_vec_kernel(
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
__global__ __launch_bounds__(kVecBlock) void cg_rz_kernel(int64_t n, const double2 *__restrict__ r,
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
    bool hyper = false;                // the Neo-Hookean tangent (unpaired TRI3 plan; kernels of tri3_hyper_cg.hip); with quad:
                                       // on the QUAD4 plan (kernels of quad4_hyper_cg.hip)
    size_t lds_apply = 0, lds_diag = 0;
    // device memory, one allocation: p[2], r, z, q (double2 rows), dinv (3 doubles per row), tile partials, vector partials,
    // status record, tickets
    char *mem = nullptr;
    double2 *p[2] = {nullptr, nullptr}, *r = nullptr, *z = nullptr, *q = nullptr;
    double *dinv = nullptr, *tile_part = nullptr, *vec_part = nullptr, *st = nullptr;
    double *work = nullptr;            // hyper: the diag launch's tile partials [3][n_tiles]
    double *cq = nullptr;              // hyper && quad: c = mu - lambda L of the last linearisation, [n_tiles][4][elem_stride]
    unsigned *tickets = nullptr;       // [0] apply, [1] vector kernels, [2] standalone apply
    double *host = nullptr;            // pinned mirror of the status record
    // bound by hfem_cg_setup
    const double2 *x_free = nullptr, *x_fixed = nullptr;
    hfem::Tri3Consts k{};
    // bound by hfem_cg_setup_shifted: A = c_K K + c_M M (k carries c_K; the Mass instances of tri3_cg.hip / quad4_cg.hip), or
    // by hfem_cg_setup_hyper_shifted: A = c_K K_T + c_M M (hk's lambda and mu carry c_K; the MASS instances of
    // tri3_hyper_cg.hip / quad4_hyper_cg.hip)
    bool shifted = false;
    hfem::DynMass dm{};
    // bound by hfem_cg_setup_scaled (non-null: the Scaled instances of tri3_cg.hip / quad4_cg.hip): K(w) = sum_e w_e K_e, one
    // weight record per slot of the plan.  Never together with shifted: each setup entry point clears what it does not bind
    const double *w_slot = nullptr;
    // bound by hfem_cg_setup_hyper
    const double2 *u_lin = nullptr, *u_fixed = nullptr;
    hfem::HyperConsts hk{};
    // bound by hfem_cg_setup_j2 (a handle of hfem_cg_create_hyper on a TRI3 plan): the J2 elastoplastic tangent from stored
    // records (the kernels of tri3_j2.hip, their own LDS sizes: never more than the Neo-Hookean tangent's)
    const hfem_j2 *j2 = nullptr;
    double *j2_tan = nullptr;
    size_t lds_apply_j2 = 0, lds_diag_j2 = 0;
    bool ready = false;
};

namespace {
hfem::CgElemArgs elem_args(const hfem_cg *c, size_t lds, hipStream_t s) {
    hfem::CgElemArgs A;
    A.plan = c->plan; A.n_tiles = c->n_tiles; A.block = c->block; A.phys = c->phys; A.x_free = c->x_free; A.x_fixed = c->x_fixed;
    A.k = c->k; A.lds = lds; A.s = s;
    A.u_lin_free = c->u_lin; A.u_fixed = c->u_fixed; A.hk = c->hk; A.cq = c->cq;
    A.shifted = c->shifted; A.dm = c->dm;
    A.w_slot = c->w_slot;
    A.j2 = c->j2; A.j2_tan = c->j2_tan;
    return A;
}

// the two places that choose the element
void cg_apply(const hfem_cg *c, const double2 *z, double2 *q, unsigned *ticket, double *st, double *host, double *pq_out,
              hipStream_t s) {
    const hfem::CgElemArgs A = elem_args(c, c->j2 ? c->lds_apply_j2 : c->lds_apply, s);
    if (c->j2) hfem::launch_tri3_j2_apply(A, z, c->p[0], c->p[1], q, c->tile_part, ticket, st, host, pq_out);
    else if (c->hyper && c->quad) hfem::launch_quad4_hyper_cg_apply(A, z, c->p[0], c->p[1], q, c->tile_part, ticket, st, host, pq_out);
    else if (c->hyper) hfem::launch_tri3_hyper_cg_apply(A, z, c->p[0], c->p[1], q, c->tile_part, ticket, st, host, pq_out);
    else if (c->quad) hfem::launch_quad4_cg_apply(A, z, c->p[0], c->p[1], q, c->tile_part, ticket, st, host, pq_out);
    else hfem::launch_tri3_cg_apply(A, z, c->p[0], c->p[1], q, c->tile_part, ticket, st, host, pq_out);
}

void cg_diag(const hfem_cg *c, double *diag, int precond, double *info, hipStream_t s) {
    const hfem::CgElemArgs A = elem_args(c, c->j2 ? c->lds_diag_j2 : c->lds_diag, s);
    if (c->j2) hfem::launch_tri3_j2_diag(A, diag, c->dinv, precond, c->work, info);
    else if (c->hyper && c->quad) hfem::launch_quad4_hyper_cg_diag(A, diag, c->dinv, precond, c->work, info);
    else if (c->hyper) hfem::launch_tri3_hyper_cg_diag(A, diag, c->dinv, precond, c->work, info);
    else if (c->quad) hfem::launch_quad4_cg_diag(A, diag, c->dinv, precond);
    else hfem::launch_tri3_cg_diag(A, diag, c->dinv, precond);
}

void cg_rz(const hfem_cg *c, hipStream_t s) {
    hipLaunchKernelGGL(hfem::cg_rz_kernel, dim3(c->vec_blocks), dim3(hfem::kVecBlock), 0, s, c->n_u, c->r, c->z,
                       c->vec_part, c->tickets + 1, c->st, c->host);
}

// amg == nullptr: block Jacobi, z and rho fused into the vector launch; otherwise z = M r (the V-cycle) and rho follow it
template <bool START>
void cg_vec(const hfem_cg *c, const hfem_amg *amg, double2 *u, const double2 *g0, const double2 *gzero, double rtol, double atol,
            double max_iter, hipStream_t s) {
#define HFEM_CG_VEC(J)                                                                                                       \
    hipLaunchKernelGGL((hfem::cg_vec_kernel<START, J>), dim3(c->vec_blocks), dim3(hfem::kVecBlock), 0, s, c->n_u, u, c->r,      \
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

static int cg_alloc(std::unique_ptr<hfem_cg> &c, hfem_cg **out);

// free u rows the plan's row maps address
static int64_t plan_u_rows(const hfem::HostPlan &h) {
    int64_t rows = 0;
    for (size_t i = 1; i < h.node_src.size(); i += 2) rows = std::max<int64_t>(rows, (int64_t)h.node_src[i] + 1);
    return rows;
}

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
    HFEM_ARG_CHECK(n_u >= plan_u_rows(h), "n_u is smaller than the plan's free u rows");
    HFEM_ARG_CHECK(n_u < ((int64_t)1 << 31), "n_u too large");
    std::unique_ptr<hfem_cg> c(new hfem_cg);
    c->plan = plan; c->device = plan->device; c->n_u = n_u; c->phys = (flags & HFEM_FLAG_PHYSICAL_GRAD) != 0;
    c->quad = quad;
    c->n_tiles = (int)h.tiles.size(); c->block = b512 ? 512 : 256;
    c->vec_blocks = (int)std::max<int64_t>(1, std::min<int64_t>(hfem::kVecMaxBlocks, (n_u + hfem::kVecBlock - 1) / hfem::kVecBlock));
    c->lds_apply = (size_t)h.max_nodes * 32 + (size_t)h.max_owned * 16 + (c->block / 64 + 2) * 8;
    c->lds_diag = (size_t)h.max_nodes * 16 + (size_t)h.max_owned * 24;
    return cg_alloc(c, out);
}

// The solver's device memory and its pinned status mirror; hands the solver over on success.
static int cg_alloc(std::unique_ptr<hfem_cg> &c, hfem_cg **out) {
    const int64_t n_u = c->n_u;
    if (int rc = hfem::use_device(c->device)) return rc;
    const size_t rows16 = (size_t)std::max<int64_t>(n_u, 1) * 16;
    const size_t off_r = 2 * rows16, off_z = 3 * rows16, off_q = 4 * rows16, off_d = 5 * rows16;
    const size_t off_tp = off_d + (size_t)std::max<int64_t>(n_u, 1) * 24;
    const size_t off_vp = off_tp + 4 * (size_t)std::max(c->n_tiles, 1) * 8;   // tile partials, then hyper's [3][n_tiles]
    const size_t off_st = off_vp + 3 * (size_t)hfem::kVecMaxBlocks * 8;
    const size_t off_tk = off_st + hfem::kStatusN * 8;
    const size_t off_cq = off_tk + 64;                                // QUAD4 tangent: four doubles per slot of the plan
    const size_t n_cq = c->hyper && c->quad ? 4 * (size_t)std::max(c->n_tiles, 1) * (size_t)c->plan->host.elem_stride : 0;
    const size_t bytes = off_cq + n_cq * 8;
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
    c->work = c->tile_part + std::max(c->n_tiles, 1);
    c->cq = n_cq ? (double *)(c->mem + off_cq) : nullptr;
    const hipError_t e = hipMemset(c->mem, 0, bytes);                 // tickets zero, p buffers zero (0 * p_old is 0)
    if (e != hipSuccess) {
        (void)hipFree(c->mem); (void)hipHostFree(c->host);
        hfem::set_error(std::string("hfem_cg_create: hipMemset -> ") + hipGetErrorString(e));
        return (int)e;
    }
    *out = c.release();
    return 0;
}

// The Neo-Hookean tangent: the plan hfem_tri3_hyper_energy_plan takes (TRI3, one element per slot), tri3_hyper_cg.hip's LDS;
// or, by h.npe as in hfem_cg_create, the plan hfem_quad4_hyper_energy_plan takes (the model's own QUAD4 plan),
// quad4_hyper_cg.hip's LDS
extern "C" int hfem_cg_create_hyper(hfem_plan *plan, int64_t n_u, hfem_cg **out) {
    HFEM_ARG_CHECK(plan && out, "null pointer");
    *out = nullptr;
    HFEM_ARG_CHECK(plan->device >= 0, "host-only plan (created with device < 0) cannot launch");
    const hfem::HostPlan &h = plan->host;
    const bool quad = h.npe == 4;
    HFEM_ARG_CHECK(quad || h.npe == 3, "the Neo-Hookean tangent exists for TRI3 and QUAD4 plans");
    HFEM_ARG_CHECK(!quad || plan->d_elem_pack_hi, "QUAD4 plan without its fourth-corner records");
    HFEM_ARG_CHECK(!h.paired, "paired plan: the Neo-Hookean tangent kernels read one element per slot (plan_elem_order 3)");
    HFEM_ARG_CHECK(h.max_nodes <= hfem::kMaxLocal && h.max_owned <= h.max_nodes, "tile shape outside the tangent kernels' instance");
    const int block = quad ? hfem::kQuad4HyperCgBlock : 512;
    const size_t lds_apply = (size_t)h.max_nodes * 48 + (size_t)h.max_owned * 16 + (block / 64 + 2) * 8;
    const size_t lds_diag = (size_t)h.max_nodes * 32 + (size_t)h.max_owned * 24 + 2 * (block / 64) * 8;
    HFEM_ARG_CHECK(lds_apply <= 64 * 1024 && lds_diag <= 64 * 1024, "tile needs more than 64 KiB of LDS");
    HFEM_ARG_CHECK(n_u >= plan_u_rows(h), "n_u is smaller than the plan's free u rows");
    HFEM_ARG_CHECK(n_u < ((int64_t)1 << 31), "n_u too large");
    std::unique_ptr<hfem_cg> c(new hfem_cg);
    c->plan = plan; c->device = plan->device; c->n_u = n_u; c->phys = true; c->hyper = true; c->quad = quad;
    c->n_tiles = (int)h.tiles.size(); c->block = block;
    c->vec_blocks = (int)std::max<int64_t>(1, std::min<int64_t>(hfem::kVecMaxBlocks, (n_u + hfem::kVecBlock - 1) / hfem::kVecBlock));
    c->lds_apply = lds_apply; c->lds_diag = lds_diag;
    return cg_alloc(c, out);
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
    HFEM_ARG_CHECK(!c->hyper, "this solver was created by hfem_cg_create_hyper: hfem_cg_setup_hyper binds it");
    bool fixed_rows = false;
    const hfem::HostPlan &h = c->plan->host;
    for (size_t i = 0; i < h.node_src.size(); i += 2) fixed_rows = fixed_rows || h.node_src[i] < 0;
    HFEM_ARG_CHECK(x_fixed || !fixed_rows, "the plan reads fixed coordinate rows: x_fixed must be given");
    if (int rc = hfem::use_device(c->device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    c->x_free = (const double2 *)x_free; c->x_fixed = (const double2 *)x_fixed;
    c->k = hfem::make_consts(mat, c->quad ? 1.0 : W, nullptr);   // QUAD4: the 2x2 rule's weights are 1 (hfem_quad4_energy_plan_ex)
    c->shifted = false; c->dm = hfem::DynMass{};
    c->w_slot = nullptr;
    cg_diag(c, diag_out, precond, nullptr, s);
    if (int rc = hfem::launch_status("hfem_cg_setup")) return rc;
    c->ready = true;
    return 0;
}

// hfem_cg_setup for K(w) = sum_e w_e K_e: the same bindings plus the slot-ordered weights, bound as a POINTER (new weights in
// the same buffer and another call re-linearise; a captured iterate graph stays valid, as after hfem_cg_setup_hyper)
extern "C" int hfem_cg_setup_scaled(hfem_cg *c, const double *x_free, const double *x_fixed, const double mat[4], double W,
                                    const double *w_slot, int32_t precond, double *diag_out, void *stream) {
    HFEM_ARG_CHECK(c && x_free && mat, "null pointer");
    HFEM_ARG_CHECK(w_slot, "w_slot must be given (one weight record per slot of the plan)");
    HFEM_ARG_CHECK(precond == 0 || precond == 1, "precond: 0 none, 1 block Jacobi");
    HFEM_ARG_CHECK(!c->hyper, "this solver was created by hfem_cg_create_hyper: the scaled operator exists for hfem_cg_create");
    bool fixed_rows = false;
    const hfem::HostPlan &h = c->plan->host;
    for (size_t i = 0; i < h.node_src.size(); i += 2) fixed_rows = fixed_rows || h.node_src[i] < 0;
    HFEM_ARG_CHECK(x_fixed || !fixed_rows, "the plan reads fixed coordinate rows: x_fixed must be given");
    if (int rc = hfem::use_device(c->device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    c->x_free = (const double2 *)x_free; c->x_fixed = (const double2 *)x_fixed;
    c->k = hfem::make_consts(mat, c->quad ? 1.0 : W, nullptr);
    c->shifted = false; c->dm = hfem::DynMass{};
    c->w_slot = w_slot;
    cg_diag(c, diag_out, precond, nullptr, s);
    if (int rc = hfem::launch_status("hfem_cg_setup_scaled")) return rc;
    c->ready = true;
    return 0;
}

// hfem_cg_setup for A = c_K K + c_M M: the same bindings, the material constants scaled by c_K and the mass coefficients
extern "C" int hfem_cg_setup_shifted(hfem_cg *c, const double *x_free, const double *x_fixed, const double mat[4], double W,
                                     double c_k, double c_m, int32_t lumped, int32_t precond, double *diag_out, void *stream) {
    HFEM_ARG_CHECK(std::isfinite(c_k) && std::isfinite(c_m) && c_k >= 0.0 && c_m >= 0.0 && (c_k > 0.0 || c_m > 0.0),
                   "c_k and c_m must be finite, >= 0 and not both zero");
    HFEM_ARG_CHECK(c && x_free && mat, "null pointer");
    HFEM_ARG_CHECK(precond == 0 || precond == 1, "precond: 0 none, 1 block Jacobi");
    HFEM_ARG_CHECK(!c->hyper, "this solver was created by hfem_cg_create_hyper: the shifted operator exists for hfem_cg_create");
    bool fixed_rows = false;
    const hfem::HostPlan &h = c->plan->host;
    for (size_t i = 0; i < h.node_src.size(); i += 2) fixed_rows = fixed_rows || h.node_src[i] < 0;
    HFEM_ARG_CHECK(x_fixed || !fixed_rows, "the plan reads fixed coordinate rows: x_fixed must be given");
    if (int rc = hfem::use_device(c->device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    c->x_free = (const double2 *)x_free; c->x_fixed = (const double2 *)x_fixed;
    c->k = hfem::scaled_consts(hfem::make_consts(mat, c->quad ? 1.0 : W, nullptr), c_k);
    c->shifted = true; c->dm = hfem::dyn_mass(c->quad, c_m, lumped != 0);
    c->w_slot = nullptr;
    cg_diag(c, diag_out, precond, nullptr, s);
    if (int rc = hfem::launch_status("hfem_cg_setup_shifted")) return rc;
    c->ready = true;
    return 0;
}

// The bindings and checks of the two hyper setups.  shifted: A = c_K K_T + c_M M -- lambda and mu times c_K (K_T is linear in
// them, tri3_hyper_cg.hip) and the mass coefficients; otherwise plain K_T.  Nothing of the handle changes before every check
// has passed.
static int cg_setup_hyper(hfem_cg *c, const double *x_free, const double *x_fixed, const double *u_lin_free, const double *u_fixed,
                          const double lame[2], double W, bool shifted, double c_k, double c_m, int32_t lumped, int32_t precond,
                          double *diag_out, double *info_out, void *stream, const char *who) {
    // the messages carry the public entry point's name, not this function's
#define HFEM_WHO_CHECK(cond, msg)                                                                                             \
    do {                                                                                                                      \
        if (!(cond)) {                                                                                                        \
            hfem::set_error(std::string(who) + ": " + (msg));                                                                 \
            return -1;                                                                                                        \
        }                                                                                                                     \
    } while (0)
    HFEM_WHO_CHECK(c && x_free && lame && (u_lin_free || c->n_u == 0), "null pointer");
    HFEM_WHO_CHECK(c->hyper, shifted ? "this solver was created by hfem_cg_create: hfem_cg_setup_shifted binds its shifted operator"
                                     : "this solver was created by hfem_cg_create: hfem_cg_setup binds it");
    HFEM_WHO_CHECK(precond == 0 || precond == 1, "precond: 0 none, 1 block Jacobi");
    bool fixed_x = false, fixed_u = false;
    const hfem::HostPlan &h = c->plan->host;
    for (size_t i = 0; i + 1 < h.node_src.size(); i += 2) {
        fixed_x = fixed_x || h.node_src[i] < 0;
        fixed_u = fixed_u || h.node_src[i + 1] < 0;
    }
    HFEM_WHO_CHECK(x_fixed || !fixed_x, "the plan reads fixed coordinate rows: x_fixed must be given");
    HFEM_WHO_CHECK(u_fixed || !fixed_u, "the plan reads Dirichlet rows: u_fixed must be given");
    HFEM_WHO_CHECK(u_lin_free || !h.tiles.size(), "u_lin_free must be given");
    if (int rc = hfem::use_device(c->device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    c->x_free = (const double2 *)x_free; c->x_fixed = (const double2 *)x_fixed;
    c->u_lin = (const double2 *)u_lin_free; c->u_fixed = (const double2 *)u_fixed;
    c->hk = hfem::HyperConsts{};
    c->hk.lambda = c_k * lame[0]; c->hk.mu = c_k * lame[1];
    c->hk.W = c->quad ? 1.0 : W;                                      // QUAD4: the 2x2 rule's weights are 1, W is not read
    c->shifted = shifted; c->dm = shifted ? hfem::dyn_mass(c->quad, c_m, lumped != 0) : hfem::DynMass{};
    c->j2 = nullptr; c->j2_tan = nullptr;
    cg_diag(c, diag_out, precond, info_out, s);
    if (int rc = hfem::launch_status(who)) return rc;
    c->ready = true;
    return 0;
#undef HFEM_WHO_CHECK
}

extern "C" int hfem_cg_setup_hyper(hfem_cg *c, const double *x_free, const double *x_fixed, const double *u_lin_free,
                                   const double *u_fixed, const double lame[2], double W, int32_t precond, double *diag_out,
                                   double *info_out, void *stream) {
    return cg_setup_hyper(c, x_free, x_fixed, u_lin_free, u_fixed, lame, W, false, 1.0, 0.0, 0, precond, diag_out, info_out, stream,
                          "hfem_cg_setup_hyper");
}

// hfem_cg_setup_hyper for A(u) = c_K K_T(u) + c_M M (c_K = 0 allowed: the pure mass operator of the initial acceleration and
// of an explicit step).  A later hfem_cg_setup_hyper returns the handle to plain K_T.
extern "C" int hfem_cg_setup_hyper_shifted(hfem_cg *c, const double *x_free, const double *x_fixed, const double *u_lin_free,
                                           const double *u_fixed, const double lame[2], double W, double c_k, double c_m,
                                           int32_t lumped, int32_t precond, double *diag_out, double *info_out, void *stream) {
    HFEM_ARG_CHECK(std::isfinite(c_k) && std::isfinite(c_m) && c_k >= 0.0 && c_m >= 0.0 && (c_k > 0.0 || c_m > 0.0),
                   "c_k and c_m must be finite, >= 0 and not both zero");
    return cg_setup_hyper(c, x_free, x_fixed, u_lin_free, u_fixed, lame, W, true, c_k, c_m, lumped, precond, diag_out, info_out,
                          stream, "hfem_cg_setup_hyper_shifted");
}

// The J2 elastoplastic tangent (tri3_j2.hip) on a handle of hfem_cg_create_hyper: the same plan kind, and no more LDS than
// the Neo-Hookean tangent (one gathered row array less).  The linearisation launch runs the return map at u_lin_free against
// j2's committed state and writes the tangent records into `tan`, bound as a POINTER: new records in the same buffer come
// from another call, and a captured hfem_cg_iterate stays valid (hfem_cg_setup_hyper's rule).  Nothing of the handle changes
// before every check has passed.
extern "C" int hfem_cg_setup_j2(hfem_cg *c, hfem_j2 *j2, const double *x_free, const double *x_fixed, const double *u_lin_free,
                                const double *u_fixed, double *tan, int32_t precond, double *diag_out, double *info_out,
                                void *stream) {
    HFEM_ARG_CHECK(c && j2 && x_free && tan && (u_lin_free || c->n_u == 0), "null pointer");
    HFEM_ARG_CHECK(c->hyper && !c->quad, "the J2 tangent binds a solver of hfem_cg_create_hyper on a TRI3 plan");
    HFEM_ARG_CHECK(j2->plan == c->plan, "the J2 state handle and the solver were created on different plans");
    HFEM_ARG_CHECK(precond == 0 || precond == 1, "precond: 0 none, 1 block Jacobi");
    bool fixed_x = false, fixed_u = false;
    const hfem::HostPlan &h = c->plan->host;
    for (size_t i = 0; i + 1 < h.node_src.size(); i += 2) {
        fixed_x = fixed_x || h.node_src[i] < 0;
        fixed_u = fixed_u || h.node_src[i + 1] < 0;
    }
    HFEM_ARG_CHECK(x_fixed || !fixed_x, "the plan reads fixed coordinate rows: x_fixed must be given");
    HFEM_ARG_CHECK(u_fixed || !fixed_u, "the plan reads Dirichlet rows: u_fixed must be given");
    HFEM_ARG_CHECK(u_lin_free || !h.tiles.size(), "u_lin_free must be given");
    if (int rc = hfem::use_device(c->device)) return rc;
    c->x_free = (const double2 *)x_free; c->x_fixed = (const double2 *)x_fixed;
    c->u_lin = (const double2 *)u_lin_free; c->u_fixed = (const double2 *)u_fixed;
    c->shifted = false; c->dm = hfem::DynMass{};
    c->j2 = j2; c->j2_tan = tan;
    c->lds_apply_j2 = (size_t)h.max_nodes * 32 + (size_t)h.max_owned * 16 + (c->block / 64 + 2) * 8;
    c->lds_diag_j2 = (size_t)h.max_nodes * 32 + (size_t)h.max_owned * 24 + (c->block / 64) * 8;
    cg_diag(c, diag_out, precond, info_out, (hipStream_t)stream);
    if (int rc = hfem::launch_status("hfem_cg_setup_j2")) return rc;
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
