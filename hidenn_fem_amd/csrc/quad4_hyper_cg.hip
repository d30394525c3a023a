// Newton-Krylov solve on the Neo-Hookean tangent of a QUAD4 model, gfx950 (MI355X): the element kernels of the PCG driver's
// fourth element kind (cg.hip; hidenn_fem_amd/newton.py).  Both run on the model's own QUAD4 plan (one cell per
// slot, elem_pack + elem_pack_hi), the plan of the Neo-Hookean energy launch, so the residual (quad4_hyper.hip) and the
// operator share a plan and its row maps; the element is hfem_quad4_hyper_dev.h's fused tangent, the phases that do not
// depend on the element are hfem_cg_dev.h's.
//   quad4_hyper_cg_apply_kernel   q = K_T(u_lin) p on the free u rows.  quad4_hyper_kernel's phases: row maps and slot
//                                 records requested up front, rows gathered to LDS (xy | uv | p per local node, p through
//                                 gather_p), the slot loop with LDS atomics into two owned-row accumulators, a plain loop
//                                 behind the prefetched records.  No edges (dead loads do not enter the tangent), no
//                                 coordinate cotangent.  Home cells contribute 1/2 p_e . q_e, so that apply_finish's factor 2
//                                 gives p^T q.
//   quad4_hyper_cg_diag_kernel    the 2x2 blocks d2Pi/du_a^2 of the owned rows (the closed form of
//                                 quad4_hyper_tangent_blocks; store_jacobi_block: a block that is not positive definite
//                                 becomes the identity) and three partials per tile over its home cells {unused, min over
//                                 the Gauss points of 1 + j_q, inverted cell count}; launch_hyper_info (tri3_hyper_cg.hip)
//                                 reduces them.
// The tangent needs L_q = log1p(j_q) only through c_q = mu - lambda L_q, and one linearisation is applied hundreds of times:
// the diag kernel, which runs once per linearisation (hfem_cg_setup_hyper), stores c_q of every slot and point (four doubles
// per slot in the driver's memory, laid out so that lanes read consecutive doubles), and the apply reads them instead of
// calling log1p four times per cell (Q1M: 52.5 -> 45.6 us per apply).  -DHFEM_QUAD4_TANGENT_RECOMPUTE builds the
// apply that recomputes them (build.py --tag: the A/B build scripts/newton_timing.py --lib-tag measures).
//
// MASS = true is the operator A(u) = c_K K_T(u) + c_M M of an implicit finite-strain Newmark step (hidenn_fem_amd/dynamics.py,
// HyperNewmarkSolver), picked by the launchers once hfem_cg_setup_hyper_shifted has bound the solver (the pattern
// of quad4_cg.hip).  c_K is on the host: lambda and mu arrive times c_K.  Exact, because every term of dP carries exactly one
// factor out of {mu, c_q = mu - lambda L_q, lambda}, each linear in (lambda, mu), and nothing else of the point's state
// depends on the material: the stored c_q of a shifted linearisation is c_K times the plain one, written and read by the
// same binding.  The mass part is quad4_mass_rows (hfem_cg_dev.h) on the corner rows of xy and p the slot already holds (its
// |det J_q| are the determinants the tangent forms from the same bilinear coefficients): no second gather, the same LDS.  It
// does not see the cell's inversion select: an inverted cell contributes zeros to K_T and its full mass to M.
// MASS = false takes the DynMass argument and does not read it.
#include <hip/hip_runtime.h>

#include "hfem_cg_dev.h"
#include "hfem_quad4_hyper_dev.h"

namespace hfem {
namespace {

constexpr int kBlock = kQuad4HyperCgBlock, kNpt = 4, kEpt = 3;

// ---------------------------------------------------------------- q = K_T p
// st != NULL: an iteration (p = z + beta p_old gathered, p stored to the other ping-pong buffer, alpha written);
// st == NULL: the standalone apply (p = z as given, pq_out[0] = p^T q).
// LDS: xy[cap_nodes] double2 | uv[cap_nodes] double2 | p[cap_nodes] double2 | acc[2][cap_owned] | red[BLOCK / 64 + 2]
// STORED: c_q = mu - lambda L_q of every slot and point is read from cq (written by the diag launch of this linearisation,
// tile t at cq + 4 t elem_stride, point q at + q elem_stride: lanes read consecutive doubles) instead of calling log1p.
template <int BLOCK, int NPT, int EPT, bool STORED, bool MASS>
__global__ __launch_bounds__(BLOCK) void quad4_hyper_cg_apply_kernel(
    PlanDev pd, int n_tiles, const double2 *__restrict__ x_free, const double2 *__restrict__ x_fixed,
    const double2 *__restrict__ u_free, const double2 *__restrict__ u_fixed, const double2 *__restrict__ z, double2 *pbuf0,
    double2 *pbuf1, double2 *__restrict__ q, Quad4HyperConsts k, DynMass dm, double *__restrict__ partials, unsigned *ticket,
    double *st, double *host, double *pq_out, const double *__restrict__ cq, int cap_nodes, int cap_owned) {
    static_assert(NPT * BLOCK >= kMaxLocal, "the row maps of a whole tile (<= 1024 local nodes) are held in registers");
    if (st && st[kHalted] != 0.0) return;                   // uniform over the grid: nothing is written after a halt
    extern __shared__ double2 lds[];
    double2 *nd_xy = lds, *nd_uv = lds + cap_nodes, *nd_p = lds + 2 * cap_nodes;
    double *acc0 = reinterpret_cast<double *>(lds + 3 * cap_nodes), *acc1 = acc0 + cap_owned;
    double *red = acc1 + cap_owned;                         // BLOCK / 64 doubles + one flag word
    const int tid = threadIdx.x;
    const CgIter it = cg_iter(st, pbuf0, pbuf1);
    const int slot = xcd_tile((int)blockIdx.x, (int)gridDim.x);
    // ---- row maps and slot records from the tile index alone (uniform strides; lanes past a stride repeat its last record)
    int2 s[NPT];
    uint32_t pk[EPT], pk3[EPT];
    const int2 *src = pd.node_src + (size_t)slot * pd.node_stride;
    const uint32_t *ep = pd.elem_pack + (size_t)slot * pd.elem_stride;
    const uint32_t *ep3 = pd.elem_pack_hi + (size_t)slot * pd.elem_stride;
    const double *cq_t = STORED ? cq + (size_t)slot * 4 * pd.elem_stride : nullptr;
#pragma unroll
    for (int j = 0; j < NPT; ++j) s[j] = src[min(tid + j * BLOCK, pd.node_stride - 1)];
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const int i = min(tid + j * BLOCK, pd.elem_stride - 1);
        pk[j] = ep[i];
        pk3[j] = ep3[i];
    }
    const TileDesc d = pd.tiles[slot];
    const int n_owned = d.n_owned;
#pragma unroll
    for (int j = 0; j < EPT; ++j)
        if (tid + j * BLOCK >= d.n_elem) pk[j] = kSkipBit;
    // ---- gather: coordinates through the x row map, the linearisation point and p through the u row map (fixed p rows are 0)
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int l = tid + j * BLOCK;
        const double2 vx = *(s[j].x >= 0 ? x_free + s[j].x : x_fixed + ~s[j].x);
        const double2 vu = *(s[j].y >= 0 ? u_free + s[j].y : u_fixed + ~s[j].y);
        const double2 vp = gather_p(it, z, s[j].y);
        if (l < d.n_node) { nd_xy[l] = vx; nd_uv[l] = vu; nd_p[l] = vp; }
        if (l < n_owned) { acc0[l] = 0.0; acc1[l] = 0.0; }
    }
    __syncthreads();

    // ---- cells (home + halo): registers + LDS only
    double e_loc = 0.0;
    auto add_row = [&](int l, const double2 v) {
        if (l < n_owned) { unsafeAtomicAdd(&acc0[l], v.x); unsafeAtomicAdd(&acc1[l], v.y); }
    };
    auto element = [&](uint32_t p, uint32_t p3, int i) {    // i: the slot's index in the tile (< d.n_elem where not skipped)
        if (p & kSkipBit) return;
        double c[4] = {0.0, 0.0, 0.0, 0.0};
        if (STORED) {
#pragma unroll
            for (int g = 0; g < 4; ++g) c[g] = cq_t[g * pd.elem_stride + i];
        }
        const int l0 = (int)(p & kLocalMask), l1 = (int)((p >> kLocalBits) & kLocalMask),
                  l2 = (int)((p >> (2 * kLocalBits)) & kLocalMask), l3 = (int)(p3 & kLocalMask);
        const double2 Xn[4] = {nd_xy[l0], nd_xy[l1], nd_xy[l2], nd_xy[l3]};
        const double2 Un[4] = {nd_uv[l0], nd_uv[l1], nd_uv[l2], nd_uv[l3]};
        const double2 Pn[4] = {nd_p[l0], nd_p[l1], nd_p[l2], nd_p[l3]};
        double2 qe[4];
        double jm1;
        bool inv;
        const double pq = STORED ? quad4_hyper_tangent_apply(Xn, Un, Pn, k, qe, jm1, inv, nullptr, c)
                                 : quad4_hyper_tangent_apply(Xn, Un, Pn, k, qe, jm1, inv);
        if constexpr (MASS) {
            const double em = quad4_mass_rows(Xn, Pn, dm, qe);
            if (p & kHomeBit) e_loc += 0.5 * pq + em;       // 1/2 p_e . q_e of the sum
        } else {
            if (p & kHomeBit) e_loc += 0.5 * pq;
        }
        add_row(l0, qe[0]);
        add_row(l1, qe[1]);
        add_row(l2, qe[2]);
        add_row(l3, qe[3]);
    };
#pragma unroll
    for (int j = 0; j < EPT; ++j) element(pk[j], pk3[j], tid + j * BLOCK);
    for (int i = tid + EPT * BLOCK; i < d.n_elem; i += BLOCK) element(ep[i], ep3[i], i);
    wave_energy(e_loc, red);
    __syncthreads();
    store_q_p<BLOCK>(s, n_owned, acc0, acc1, nd_p, q, it.p_new);
    apply_finish<BLOCK>(red, partials, slot, ticket, n_tiles, st, host, pq_out);
}

// ---------------------------------------------------------------- block-Jacobi setup + inversion report
// LDS: xy[cap_nodes] double2 | uv[cap_nodes] double2 | acc[3][cap_owned] | red[2][BLOCK / 64]
// MASS: the blocks of A, the mass on xx and yy: M_e[a][a] = sum_q |det J_q| N_a(q) (m_off N_a(q) + m_dd), of every cell,
// inverted or not.
template <int BLOCK, int NPT, bool MASS>
__global__ __launch_bounds__(BLOCK) void quad4_hyper_cg_diag_kernel(
    PlanDev pd, int n_tiles, const double2 *__restrict__ x_free, const double2 *__restrict__ x_fixed,
    const double2 *__restrict__ u_free, const double2 *__restrict__ u_fixed, Quad4HyperConsts k, DynMass dm,
    double *__restrict__ diag, double *__restrict__ dinv, int precond, double *__restrict__ work, double *__restrict__ cq,
    int cap_nodes, int cap_owned) {
    static_assert(NPT * BLOCK >= kMaxLocal, "the row maps of a whole tile (<= 1024 local nodes) are held in registers");
    extern __shared__ double2 lds[];
    double2 *nd_xy = lds, *nd_uv = lds + cap_nodes;
    double *acc0 = reinterpret_cast<double *>(lds + 2 * cap_nodes), *acc1 = acc0 + cap_owned, *acc2 = acc1 + cap_owned;
    double *red = acc2 + cap_owned;
    const int tid = threadIdx.x;
    const int slot = (int)blockIdx.x;
    int2 s[NPT];
    const int2 *src = pd.node_src + (size_t)slot * pd.node_stride;
    const uint32_t *ep = pd.elem_pack + (size_t)slot * pd.elem_stride;
    const uint32_t *ep3 = pd.elem_pack_hi + (size_t)slot * pd.elem_stride;
#pragma unroll
    for (int j = 0; j < NPT; ++j) s[j] = src[min(tid + j * BLOCK, pd.node_stride - 1)];
    const TileDesc d = pd.tiles[slot];
    const int n_owned = d.n_owned;
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int l = tid + j * BLOCK;
        const double2 vx = *(s[j].x >= 0 ? x_free + s[j].x : x_fixed + ~s[j].x);
        const double2 vu = *(s[j].y >= 0 ? u_free + s[j].y : u_fixed + ~s[j].y);
        if (l < d.n_node) { nd_xy[l] = vx; nd_uv[l] = vu; }
        if (l < n_owned) { acc0[l] = 0.0; acc1[l] = 0.0; acc2[l] = 0.0; }
    }
    __syncthreads();
    double j_min = (double)INFINITY, n_inv = 0.0;
    for (int i = tid; i < d.n_elem; i += BLOCK) {
        const uint32_t p = ep[i];
        if (p & kSkipBit) continue;
        const int l[4] = {(int)(p & kLocalMask), (int)((p >> kLocalBits) & kLocalMask), (int)((p >> (2 * kLocalBits)) & kLocalMask),
                          (int)(ep3[i] & kLocalMask)};
        const double2 Xn[4] = {nd_xy[l[0]], nd_xy[l[1]], nd_xy[l[2]], nd_xy[l[3]]};
        const double2 Un[4] = {nd_uv[l[0]], nd_uv[l[1]], nd_uv[l[2]], nd_uv[l[3]]};
        double blk[4][3], jm1, c[4];
        bool inv;
        quad4_hyper_tangent_blocks(Xn, Un, k, blk, jm1, inv, c);
        double ad[4];                                       // |det J_q| (MASS only)
        if constexpr (MASS) quad4_abs_dets(Xn, ad);
        if (cq) {                                           // every slot, home or halo: the apply reads it by slot
#pragma unroll
            for (int g = 0; g < 4; ++g) cq[((size_t)slot * 4 + g) * pd.elem_stride + i] = c[g];
        }
        if (p & kHomeBit) {
            j_min = fmin(j_min, 1.0 + jm1);
            n_inv += inv ? 1.0 : 0.0;
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            if (l[a] >= n_owned) continue;
            double mm = 0.0;                                // M_e[a][a] (MASS only)
            if constexpr (MASS) {
#pragma unroll
                for (int q = 0; q < 4; ++q) mm += ad[q] * quad4_n(a, q) * (dm.m_off * quad4_n(a, q) + dm.m_dd);
            }
            unsafeAtomicAdd(&acc0[l[a]], with_mass<MASS>(blk[a][0], mm));
            unsafeAtomicAdd(&acc1[l[a]], blk[a][1]);
            unsafeAtomicAdd(&acc2[l[a]], with_mass<MASS>(blk[a][2], mm));
        }
    }
    {
        const double wj = wave_min(j_min), wc = wave_sum(n_inv);
        if ((tid & 63) == 0) {
            red[tid >> 6] = wj;
            red[BLOCK / 64 + (tid >> 6)] = wc;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int l = tid + j * BLOCK;
        if (l < n_owned && s[j].y >= 0) store_jacobi_block(diag, dinv, s[j].y, precond, acc0[l], acc1[l], acc2[l]);
    }
    if (tid == 0) {
        double tj = (double)INFINITY, tc = 0.0;
#pragma unroll
        for (int w = 0; w < BLOCK / 64; ++w) {
            tj = fmin(tj, red[w]);
            tc += red[BLOCK / 64 + w];
        }
        work[slot] = 0.0;
        work[n_tiles + slot] = tj;
        work[2 * n_tiles + slot] = tc;
    }
}

}  // namespace

// ---------------------------------------------------------------- launchers
// the driver binds the material as hfem_cg_setup_hyper's HyperConsts: lambda and mu (no body force enters the tangent)
static Quad4HyperConsts quad4_consts(const CgElemArgs &A) {
    Quad4HyperConsts k{};
    k.lambda = A.hk.lambda; k.mu = A.hk.mu;
    return k;
}

void launch_quad4_hyper_cg_apply(const CgElemArgs &A, const double2 *z, double2 *pbuf0, double2 *pbuf1, double2 *q,
                                 double *partials, unsigned *ticket, double *st, double *host, double *pq_out) {
    const HostPlan &h = A.plan->host;
    if (A.n_tiles <= 0) return;
#ifdef HFEM_QUAD4_TANGENT_RECOMPUTE                         // A/B build of scripts/newton_timing.py --quad: log1p in every apply
    constexpr bool stored = false;
#else
    constexpr bool stored = true;
#endif
#define HFEM_Q4HCG_APPLY(MASS)                                                                                                \
    hipLaunchKernelGGL((quad4_hyper_cg_apply_kernel<kBlock, kNpt, kEpt, stored, MASS>), dim3(A.n_tiles), dim3(kBlock), A.lds, \
                       A.s, plan_dev(A.plan), A.n_tiles, A.x_free, A.x_fixed, A.u_lin_free, A.u_fixed, z, pbuf0, pbuf1, q,    \
                       quad4_consts(A), A.dm, partials, ticket, st, host, pq_out, A.cq, h.max_nodes, h.max_owned)
    if (A.shifted) HFEM_Q4HCG_APPLY(true);
    else HFEM_Q4HCG_APPLY(false);
#undef HFEM_Q4HCG_APPLY
}

void launch_quad4_hyper_cg_diag(const CgElemArgs &A, double *diag, double *dinv, int precond, double *work, double *info) {
    const HostPlan &h = A.plan->host;
#define HFEM_Q4HCG_DIAG(MASS)                                                                                                 \
    hipLaunchKernelGGL((quad4_hyper_cg_diag_kernel<kBlock, kNpt, MASS>), dim3(A.n_tiles), dim3(kBlock), A.lds, A.s,           \
                       plan_dev(A.plan), A.n_tiles, A.x_free, A.x_fixed, A.u_lin_free, A.u_fixed, quad4_consts(A), A.dm, diag, dinv, \
                       precond, work, A.cq, h.max_nodes, h.max_owned)
    if (A.n_tiles > 0) {
        if (A.shifted) HFEM_Q4HCG_DIAG(true);
        else HFEM_Q4HCG_DIAG(false);
    }
#undef HFEM_Q4HCG_DIAG
    if (info) launch_hyper_info(work, A.n_tiles, info, A.s);
}

}  // namespace hfem
