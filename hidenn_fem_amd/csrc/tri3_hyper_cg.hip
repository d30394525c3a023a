// Newton-Krylov solve on the Neo-Hookean tangent of a TRI3 model, gfx950 (MI355X): the element kernels of the PCG driver's
// third element kind (cg.hip; hidenn_fem_amd/newton.py).  Both run on the one-element-per-slot plan of the
// Neo-Hookean energy launch (plan_elem_order 3), so the residual (tri3_hyper.hip) and the operator share a plan and its row
// maps; the element is hfem_hyper_dev.h's state + apply, the phases that do not depend on the element are hfem_cg_dev.h's.
//   tri3_hyper_cg_apply_kernel   q = K_T(u_lin) p on the free u rows.  tri3_hyper_kernel's phases: row maps and slot records
//                                requested up front, rows gathered to LDS (xy | uv | p per local node, p through gather_p),
//                                the slot loop with LDS atomics into two owned-row accumulators, a plain loop behind the
//                                prefetched records.  No edges (dead loads do not enter the tangent), no coordinate cotangent.
//                                Home elements contribute 1/2 p_e . q_e, so that apply_finish's factor 2 gives p^T q.
//   tri3_hyper_cg_diag_kernel    the 2x2 blocks d2Pi/du_a^2 of the owned rows (six unit directions on one element state,
//                                store_jacobi_block: a block that is not positive definite becomes the identity -- the tangent
//                                can be indefinite) and three partials per tile over its home elements {unused, min J,
//                                inverted count}; hyper_info_kernel reduces them, so the host learns whether the
//                                linearisation point has an inverted element without a second element launch.
//
// MASS = true is the operator A(u) = c_K K_T(u) + c_M M of an implicit finite-strain Newmark step (hidenn_fem_amd/dynamics.py,
// HyperNewmarkSolver), which the launchers pick once hfem_cg_setup_hyper_shifted has bound the solver: the same
// kernels with the mass code compiled in (the pattern of tri3_cg.hip).  c_K is on the host: HyperConsts::lambda and mu arrive
// times c_K.  That is exact, not an approximation: every term of dP = mu dH + (mu - lambda L) T dH^T T + lambda (T : dH) T
// carries exactly one factor out of {mu, c = mu - lambda L, lambda}, each linear in (lambda, mu), while T, L, J^-1 and A depend
// on the state alone -- so K_T(c_K lambda, c_K mu) = c_K K_T(lambda, mu) and no instruction is added.  The mass part is
// tri3_mass_rows (hfem_cg_dev.h) on the corner rows of xy and p the slot has already read from LDS: no second gather, the
// same LDS.  It reads neither HyperTangent::sA (0 for an inverted element, and it carries the loss's W) nor W: an inverted
// element contributes zeros to K_T and its full |det J_ref| (m_off + m_dd delta_ab) to M.  min J and the inverted count do
// not change.  MASS = false takes the DynMass argument and does not read it.
#include <hip/hip_runtime.h>

#include "hfem_cg_dev.h"
#include "hfem_hyper_dev.h"

namespace hfem {
namespace {

constexpr int kBlock = 512, kNpt = 2, kEpt = 4, kInfoBlock = 256;

// ---------------------------------------------------------------- q = K_T p
// st != NULL: an iteration (p = z + beta p_old gathered, p stored to the other ping-pong buffer, alpha written);
// st == NULL: the standalone apply (p = z as given, pq_out[0] = p^T q).
// LDS: xy[cap_nodes] double2 | uv[cap_nodes] double2 | p[cap_nodes] double2 | acc[2][cap_owned] | red[BLOCK / 64 + 2]
template <int BLOCK, int NPT, int EPT, bool MASS>
__global__ __launch_bounds__(BLOCK) void tri3_hyper_cg_apply_kernel(
    PlanDev pd, int n_tiles, const double2 *__restrict__ x_free, const double2 *__restrict__ x_fixed,
    const double2 *__restrict__ u_free, const double2 *__restrict__ u_fixed, const double2 *__restrict__ z, double2 *pbuf0,
    double2 *pbuf1, double2 *__restrict__ q, HyperConsts k, DynMass dm, double *__restrict__ partials, unsigned *ticket,
    double *st, double *host, double *pq_out, int cap_nodes, int cap_owned) {
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
    uint32_t pk[EPT];
    const int2 *src = pd.node_src + (size_t)slot * pd.node_stride;
    const uint32_t *ep = pd.elem_pack + (size_t)slot * pd.elem_stride;
#pragma unroll
    for (int j = 0; j < NPT; ++j) s[j] = src[min(tid + j * BLOCK, pd.node_stride - 1)];
#pragma unroll
    for (int j = 0; j < EPT; ++j) pk[j] = ep[min(tid + j * BLOCK, pd.elem_stride - 1)];
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

    // ---- elements (home + halo): registers + LDS only
    double e_loc = 0.0;
    auto element = [&](uint32_t p) {
        if (p & kSkipBit) return;
        const int l0 = (int)(p & kLocalMask), l1 = (int)((p >> kLocalBits) & kLocalMask),
                  l2 = (int)((p >> (2 * kLocalBits)) & kLocalMask);
        const HyperTangent t = hyper_tangent_state(nd_xy[l0], nd_xy[l1], nd_xy[l2], nd_uv[l0], nd_uv[l1], nd_uv[l2], k);
        double2 qe[3];
        const double pq = hyper_tangent_apply(t, k, nd_p[l0], nd_p[l1], nd_p[l2], qe);
        if constexpr (MASS) {                               // the same LDS rows again: no store lies between, they are not re-read
            const double em = tri3_mass_rows(nd_xy[l0], nd_xy[l1], nd_xy[l2], nd_p[l0], nd_p[l1], nd_p[l2], dm, qe);
            if (p & kHomeBit) e_loc += 0.5 * pq + em;       // 1/2 p_e . q_e of the sum
        } else {
            if (p & kHomeBit) e_loc += 0.5 * pq;
        }
        if (l0 < n_owned) { unsafeAtomicAdd(&acc0[l0], qe[0].x); unsafeAtomicAdd(&acc1[l0], qe[0].y); }
        if (l1 < n_owned) { unsafeAtomicAdd(&acc0[l1], qe[1].x); unsafeAtomicAdd(&acc1[l1], qe[1].y); }
        if (l2 < n_owned) { unsafeAtomicAdd(&acc0[l2], qe[2].x); unsafeAtomicAdd(&acc1[l2], qe[2].y); }
    };
#pragma unroll
    for (int j = 0; j < EPT; ++j) element(pk[j]);
    for (int i = tid + EPT * BLOCK; i < d.n_elem; i += BLOCK) element(ep[i]);
    wave_energy(e_loc, red);
    __syncthreads();
    store_q_p<BLOCK>(s, n_owned, acc0, acc1, nd_p, q, it.p_new);
    apply_finish<BLOCK>(red, partials, slot, ticket, n_tiles, st, host, pq_out);
}

// ---------------------------------------------------------------- block-Jacobi setup + inversion report
// LDS: xy[cap_nodes] double2 | uv[cap_nodes] double2 | acc[3][cap_owned] | red[2][BLOCK / 64]
// MASS: the blocks of A, the mass on xx and yy: M_e[a][a] = |det J_ref| (m_off + m_dd), of every element, inverted or not.
template <int BLOCK, int NPT, bool MASS>
__global__ __launch_bounds__(BLOCK) void tri3_hyper_cg_diag_kernel(
    PlanDev pd, int n_tiles, const double2 *__restrict__ x_free, const double2 *__restrict__ x_fixed,
    const double2 *__restrict__ u_free, const double2 *__restrict__ u_fixed, HyperConsts k, DynMass dm,
    double *__restrict__ diag, double *__restrict__ dinv, int precond, double *__restrict__ work, int cap_nodes, int cap_owned) {
    extern __shared__ double2 lds[];
    double2 *nd_xy = lds, *nd_uv = lds + cap_nodes;
    double *acc0 = reinterpret_cast<double *>(lds + 2 * cap_nodes), *acc1 = acc0 + cap_owned, *acc2 = acc1 + cap_owned;
    double *red = acc2 + cap_owned;
    const int tid = threadIdx.x;
    const int slot = (int)blockIdx.x;
    int2 s[NPT];
    const int2 *src = pd.node_src + (size_t)slot * pd.node_stride;
    const uint32_t *ep = pd.elem_pack + (size_t)slot * pd.elem_stride;
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
        const int l[3] = {(int)(p & kLocalMask), (int)((p >> kLocalBits) & kLocalMask), (int)((p >> (2 * kLocalBits)) & kLocalMask)};
        const HyperTangent t = hyper_tangent_state(nd_xy[l[0]], nd_xy[l[1]], nd_xy[l[2]], nd_uv[l[0]], nd_uv[l[1]], nd_uv[l[2]], k);
        double mm = 0.0;                                    // M_e[a][a], the same for the three corners (MASS only)
        if constexpr (MASS) {
            const double2 X0 = nd_xy[l[0]], X1 = nd_xy[l[1]], X2 = nd_xy[l[2]];
            mm = fabs((X0.x - X2.x) * (X1.y - X2.y) - (X1.x - X2.x) * (X0.y - X2.y)) * (dm.m_off + dm.m_dd);
        }
        if (p & kHomeBit) {
            j_min = fmin(j_min, 1.0 + t.j);
            n_inv += t.j > -1.0 ? 0.0 : 1.0;
        }
        // the corner blocks: column c of K_aa = row a of the apply at p_a = e_c, p_b = 0 (b != a)
        const double2 o = make_double2(0.0, 0.0), ex = make_double2(1.0, 0.0), ey = make_double2(0.0, 1.0);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (l[a] >= n_owned) continue;
            double2 gu[3], hu[3];
            hyper_tangent_apply(t, k, a == 0 ? ex : o, a == 1 ? ex : o, a == 2 ? ex : o, gu);
            hyper_tangent_apply(t, k, a == 0 ? ey : o, a == 1 ? ey : o, a == 2 ? ey : o, hu);
            unsafeAtomicAdd(&acc0[l[a]], with_mass<MASS>(gu[a].x, mm));
            unsafeAtomicAdd(&acc1[l[a]], 0.5 * (gu[a].y + hu[a].x));
            unsafeAtomicAdd(&acc2[l[a]], with_mass<MASS>(hu[a].y, mm));
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

// info = {min J, inverted count} from the tile partials work[3][n] (hyper_finish_kernel's pattern; one block, behind the
// diag launch's kernel boundary)
__global__ __launch_bounds__(kInfoBlock) void hyper_info_kernel(const double *__restrict__ work, int n, double *__restrict__ info_out) {
    __shared__ double red_j[kInfoBlock / 64], red_c[kInfoBlock / 64];
    double e, mj, cnt;
    hyper_finish_thread(work, n, (int)threadIdx.x, kInfoBlock, e, mj, cnt);
    mj = wave_min(mj);
    if ((threadIdx.x & 63) == 0) red_j[threadIdx.x >> 6] = mj;
    const double tc = block_sum(cnt, red_c);                // its barrier also orders red_j
    if (threadIdx.x == 0) {
        double tj = red_j[0];
        for (int w = 1; w < kInfoBlock / 64; ++w) tj = fmin(tj, red_j[w]);
        info_out[0] = tj;
        info_out[1] = tc;
    }
}

}  // namespace

// ---------------------------------------------------------------- launchers
void launch_tri3_hyper_cg_apply(const CgElemArgs &A, const double2 *z, double2 *pbuf0, double2 *pbuf1, double2 *q,
                                double *partials, unsigned *ticket, double *st, double *host, double *pq_out) {
    const HostPlan &h = A.plan->host;
    if (A.n_tiles <= 0) return;
#define HFEM_HCG_APPLY(MASS)                                                                                                  \
    hipLaunchKernelGGL((tri3_hyper_cg_apply_kernel<kBlock, kNpt, kEpt, MASS>), dim3(A.n_tiles), dim3(kBlock), A.lds, A.s,     \
                       plan_dev(A.plan), A.n_tiles, A.x_free, A.x_fixed, A.u_lin_free, A.u_fixed, z, pbuf0, pbuf1, q, A.hk, A.dm, \
                       partials, ticket, st, host, pq_out, h.max_nodes, h.max_owned)
    if (A.shifted) HFEM_HCG_APPLY(true);
    else HFEM_HCG_APPLY(false);
#undef HFEM_HCG_APPLY
}

void launch_tri3_hyper_cg_diag(const CgElemArgs &A, double *diag, double *dinv, int precond, double *work, double *info) {
    const HostPlan &h = A.plan->host;
#define HFEM_HCG_DIAG(MASS)                                                                                                   \
    hipLaunchKernelGGL((tri3_hyper_cg_diag_kernel<kBlock, kNpt, MASS>), dim3(A.n_tiles), dim3(kBlock), A.lds, A.s,            \
                       plan_dev(A.plan), A.n_tiles, A.x_free, A.x_fixed, A.u_lin_free, A.u_fixed, A.hk, A.dm, diag, dinv,     \
                       precond, work, h.max_nodes, h.max_owned)
    if (A.n_tiles > 0) {
        if (A.shifted) HFEM_HCG_DIAG(true);
        else HFEM_HCG_DIAG(false);
    }
#undef HFEM_HCG_DIAG
    if (info) launch_hyper_info(work, A.n_tiles, info, A.s);
}

void launch_hyper_info(const double *work, int n, double *info, hipStream_t s) {
    hipLaunchKernelGGL(hyper_info_kernel, dim3(1), dim3(kInfoBlock), 0, s, work, n, info);
}

}  // namespace hfem
