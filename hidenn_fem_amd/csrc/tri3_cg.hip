// Frozen-mesh displacement solve on TRI3, gfx950 (MI355X): the element kernels of the matrix-free PCG solve over the paired
// owner-computes tile plan (hidenn_fem_amd/solve.py, FrozenMeshSolver).  The PCG driver (cg.hip) launches them through
// launch_tri3_cg_apply / launch_tri3_cg_diag; the phases they share with the QUAD4 kernels (quad4_cg.hip) -- iteration state,
// p rows, write-out, the p^T q epilogue, the Jacobi block store -- are hfem_cg_dev.h's.
//
// At fixed coordinates the total potential is exactly quadratic in u: E(u) = 1/2 u^T K u - f^T u.  So K p is the u-half of
// the energy gradient at u = p with no forces (tri3_element<GRAD, HASB = false>: the same closed forms, both gradient
// conventions).
//   tri3_cg_apply_kernel  q = K p on the free u rows: the pair kernel's gather, slot loop and LDS accumulation with the
//                         coordinate cotangent, the forces and the edges dropped.  Fused p-update: every node it gathers forms
//                         p = z + beta p_old on the fly; the tile that owns a row stores p to the OTHER buffer of a ping-pong
//                         pair (tiles still gathering read p_old as halo).  One partial of p^T q per tile (2 x the strain
//                         energy of p over its home elements); the last workgroup (ticket) sums them in tile order and
//                         writes alpha = rho / p^T q.  Nothing runs once the status record says halted.
//   tri3_cg_diag_kernel   2x2 diagonal blocks of K (block Jacobi), once per refresh: per corner a of every element the
//                         block d2E/du_a^2 = the element gradient at u = unit vector at a, accumulated into the owner node.
//
// Every kernel here is one frame in three instances of the operator tag ElemOp (hfem_cg_dev.h), which the launchers pick:
// Plain is K as above.
//
// ElemOp::Mass is the shifted operator A = c_K K + c_M M of a Newmark step (hidenn_fem_amd/dynamics.py), which the
// launchers pick once hfem_cg_setup_shifted has bound the solver: the same kernels with the mass code compiled in.  The
// stiffness part is tri3_element on material constants the host scaled by c_K (K is linear in them, so gu and e arrive
// scaled); the mass part is formed in the slot loop from what the element already holds -- the corner coordinates and the
// corner values of p -- with no extra memory traffic:
//   M_e[a][b] = |det J| (m_off + m_dd delta_ab),  consistent: m_off = m_dd = c_M / 24,  lumped: m_off = 0, m_dd = c_M / 6
// (c_M includes the density; run-time coefficients, not instances).  Always |det J|: no gradient convention enters the mass.
//   (M_e p)_a = |det J| (m_off (p_0 + p_1 + p_2) + m_dd p_a),   1/2 p^T M_e p = 1/2 |det J| (m_off |sum p|^2 + m_dd sum |p_a|^2)
// The tile energy is c_K e + 1/2 c_M p^T M_e p, so apply_finish's p^T q = 2 x sum stays right.  The diag kernel adds
// M_e[a][a] = |det J| (m_off + m_dd) to xx and yy of every block.  The other instances take the DynMass argument and do not
// read it.
//
// ElemOp::Scaled is the element-scaled stiffness K(w) = sum_e w_e K_e (hidenn_fem_amd/solve.py set_element_scale),
// picked once hfem_cg_setup_scaled has bound w_slot: n_tiles x elem_stride records double2 {w_A, w_B} addressed exactly as
// elem_pack, loaded in the round of elem_pack / elem_pack_hi (one coalesced read per slot row, lane t at record t) and held in
// registers: no extra LDS, no index stream, no scattered gather (reading w[elem_gid[slot]] would add both to every CG
// iteration).  In the slot loop each element's gradient rows and energy are multiplied by its weight before the in-register
// pair sum and the LDS atomics; the diag kernel multiplies the element's three block entries.  w_B is used inside the hasB
// branch only; the record of a skipped or padded slot is never used (it may hold anything, NaN included).  The other
// instances take the w_slot argument and do not read it.
#include <hip/hip_runtime.h>

#include "hfem_cg_dev.h"

namespace hfem {
namespace {

// ---------------------------------------------------------------- q = K p (Mass: q = A p; Scaled: q = K(w) p)
// st != NULL: an iteration (p = z + beta p_old gathered, p stored to the other ping-pong buffer, alpha written);
// st == NULL: the standalone apply (p = z as given, pq_out[0] = p^T q).  Mass: k is the material constants times c_K.
template <int BLOCK, int NPT, int EPT, bool PHYS, ElemOp OP>
__global__ __launch_bounds__(BLOCK) void tri3_cg_apply_kernel(
    PlanDev pd, int n_tiles, const double2 *__restrict__ x_free, const double2 *__restrict__ x_fixed,
    const double2 *__restrict__ z, double2 *pbuf0, double2 *pbuf1, double2 *__restrict__ q, Tri3Consts k, DynMass dm,
    const double2 *__restrict__ w_slot, double *__restrict__ partials, unsigned *ticket, double *st, double *host, double *pq_out,
    int cap_nodes, int cap_owned, int col_stride) {
    if (st && st[kHalted] != 0.0) return;                   // uniform over the grid: nothing is written after a halt
    extern __shared__ double2 lds[];
    double2 *nd_xy = lds, *nd_p = lds + cap_nodes;
    double *acc0 = reinterpret_cast<double *>(lds + 2 * cap_nodes), *acc1 = acc0 + cap_owned;
    double *red = acc1 + cap_owned;                         // BLOCK / 64 doubles + one flag word
    const int tid = threadIdx.x;
    const CgIter it = cg_iter(st, pbuf0, pbuf1);
    const int slot = xcd_tile((int)blockIdx.x, (int)gridDim.x);
    int2 s[NPT];
    const int2 *src = pd.node_src + (size_t)slot * pd.node_stride;
#pragma unroll
    for (int j = 0; j < NPT; ++j) s[j] = src[min(tid + j * BLOCK, pd.node_stride - 1)];
    const TileDesc d = pd.tiles[slot];
    uint32_t w0[EPT], w1[EPT];
    double wa[EPT], wb[EPT];                                // Scaled: the slot's weights (plain doubles: no local double2 array)
    const size_t rec0 = (size_t)slot * pd.elem_stride;
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const size_t i = rec0 + min(tid + j * col_stride, pd.elem_stride - 1);
        w0[j] = pd.elem_pack[i];
        w1[j] = pd.elem_pack_hi[i];
        if constexpr (OP == ElemOp::Scaled) {
            const double2 w = w_slot[i];
            wa[j] = w.x; wb[j] = w.y;
        }
    }
    // gather: coordinates through the x row map, p through the u row map (fixed u rows are 0)
    double2 vx[NPT], vp[NPT];
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        vx[j] = s[j].x >= 0 ? x_free[s[j].x] : x_fixed[~s[j].x];
        vp[j] = gather_p(it, z, s[j].y);
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
                const double2 Xb = nd_xy[lb], Pb = nd_p[lb];
                double2 gx[3], gu[3];
                double e = tri3_element<true, false, PHYS>(Xn, Xb, Xc, Pn, Pb, Pc, k, gx, gu);
                if constexpr (OP == ElemOp::Mass) e += tri3_mass_rows(Xn, Xb, Xc, Pn, Pb, Pc, dm, gu);
                if constexpr (OP == ElemOp::Scaled) {
                    const double w = wa[j];
                    if (a & kHomeBit) e_loc += w * e;
                    if (lb < n_owned) add_row(lb, make_double2(w * gu[1].x, w * gu[1].y));
                    sn = make_double2(w * gu[0].x, w * gu[0].y); sc = make_double2(w * gu[2].x, w * gu[2].y);
                } else {
                    if (a & kHomeBit) e_loc += e;
                    if (lb < n_owned) add_row(lb, gu[1]);
                    sn = gu[0]; sc = gu[2];
                }
            }
            if (b & kHasBBit) {                             // B = (n, c, d): the only reader of w_B
                const int ld = (int)(b & kLocalMask);
                const double2 Xd = nd_xy[ld], Pd = nd_p[ld];
                double2 gx[3], gu[3];
                double e = tri3_element<true, false, PHYS>(Xn, Xc, Xd, Pn, Pc, Pd, k, gx, gu);
                if constexpr (OP == ElemOp::Mass) e += tri3_mass_rows(Xn, Xc, Xd, Pn, Pc, Pd, dm, gu);
                if constexpr (OP == ElemOp::Scaled) {
                    const double w = wb[j];
                    if (b & kHomeBBit) e_loc += w * e;
                    if (ld < n_owned) add_row(ld, make_double2(w * gu[2].x, w * gu[2].y));
                    sn.x = __builtin_fma(w, gu[0].x, sn.x); sn.y = __builtin_fma(w, gu[0].y, sn.y);
                    sc.x = __builtin_fma(w, gu[1].x, sc.x); sc.y = __builtin_fma(w, gu[1].y, sc.y);
                } else {
                    if (b & kHomeBBit) e_loc += e;
                    if (ld < n_owned) add_row(ld, gu[2]);
                    sn.x += gu[0].x; sn.y += gu[0].y; sc.x += gu[1].x; sc.y += gu[1].y;
                }
            }
            if (ln < n_owned) add_row(ln, sn);
            if (lc < n_owned) add_row(lc, sc);
        }
    }
    wave_energy(e_loc, red);
    __syncthreads();
    store_q_p<BLOCK>(s, n_owned, acc0, acc1, nd_p, q, it.p_new);
    apply_finish<BLOCK>(red, partials, slot, ticket, n_tiles, st, host, pq_out);
}

// ---------------------------------------------------------------- block-Jacobi setup
// Mass: the 2x2 diagonal blocks of A, the mass on xx and yy: M_e[a][a] = |det J| (m_off + m_dd).  Scaled: the element's three
// block entries times its weight.
template <int BLOCK, int NPT, int EPT, bool PHYS, ElemOp OP>
__global__ __launch_bounds__(BLOCK) void tri3_cg_diag_kernel(PlanDev pd, const double2 *__restrict__ x_free,
                                                             const double2 *__restrict__ x_fixed, Tri3Consts k, DynMass dm,
                                                             double *__restrict__ diag, double *__restrict__ dinv,
                                                             const double2 *__restrict__ w_slot, int precond, int cap_nodes,
                                                             int cap_owned, int col_stride) {
    constexpr bool MASS = OP == ElemOp::Mass;
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
    const double m_aa = dm.m_off + dm.m_dd;                 // read by MASS only
    // the three corner blocks of one element: column c of K_aa = the gradient at u_a = e_c, u_b = 0 (b != a)
    auto element = [&](int l0, int l1, int l2, double w) {
        const int ls[3] = {l0, l1, l2};
        const double2 X[3] = {nd_xy[l0], nd_xy[l1], nd_xy[l2]};
        double mm = 0.0;                                    // M_e[a][a], the same for the three corners (MASS only)
        if constexpr (MASS) mm = fabs((X[0].x - X[2].x) * (X[1].y - X[2].y) - (X[1].x - X[2].x) * (X[0].y - X[2].y)) * m_aa;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (ls[a] >= n_owned) continue;
            double2 gu[3], hu[3];
            unit_columns<PHYS>(X, a, k, gu, hu);
            unsafeAtomicAdd(&acc0[ls[a]], with_weight<OP>(with_mass<MASS>(gu[a].x, mm), w));
            unsafeAtomicAdd(&acc1[ls[a]], with_weight<OP>(0.5 * (gu[a].y + hu[a].x), w));
            unsafeAtomicAdd(&acc2[ls[a]], with_weight<OP>(with_mass<MASS>(hu[a].y, mm), w));
        }
    };
    for (int j = 0; j < EPT; ++j) {
        if (!(tid < col_stride && tid + j * col_stride < d.n_elem)) continue;
        const size_t i = (size_t)slot * pd.elem_stride + tid + j * col_stride;
        const uint32_t a = pd.elem_pack[i], b = pd.elem_pack_hi[i];
        if (a & kSkipBit) continue;
        double2 w = make_double2(0.0, 0.0);                 // {w_A, w_B} (Scaled only)
        if constexpr (OP == ElemOp::Scaled) w = w_slot[i];
        const int ln = (int)(a & kLocalMask), lb = (int)((a >> kLocalBits) & kLocalMask),
                  lc = (int)((a >> (2 * kLocalBits)) & kLocalMask);
        element(ln, lb, lc, w.x);
        if (b & kHasBBit) element(ln, lc, (int)(b & kLocalMask), w.y);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int l = tid + j * BLOCK;
        if (l < n_owned && s[j].y >= 0) store_jacobi_block(diag, dinv, s[j].y, precond, acc0[l], acc1[l], acc2[l]);
    }
}

}  // namespace

// ---------------------------------------------------------------- launchers
// The tile shapes of a paired plan: 512 threads (2 nodes and 2 slot rows per thread), or 256 threads with 3 | 4 nodes and
// 3 | 4 | 6 slot rows per thread (the pair kernel's matrix: a masked row or node costs a full pass of the slot loop).  Each
// shape in both gradient conventions (A.phys) and the three operators (HFEM_CG_OP: A.shifted, A.w_slot, neither).
void launch_tri3_cg_apply(const CgElemArgs &A, const double2 *z, double2 *pbuf0, double2 *pbuf1, double2 *q, double *partials,
                          unsigned *ticket, double *st, double *host, double *pq_out) {
    const HostPlan &h = A.plan->host;
    const PlanDev pd = plan_dev(A.plan);
#define HFEM_CG_APPLY(BLOCK, NPT, EPT, PH, OP)                                                                                \
    hipLaunchKernelGGL((tri3_cg_apply_kernel<BLOCK, NPT, EPT, PH, ElemOp::OP>), dim3(A.n_tiles), dim3(BLOCK), A.lds, A.s, pd, \
                       A.n_tiles, A.x_free, A.x_fixed, z, pbuf0, pbuf1, q, A.k, A.dm, (const double2 *)A.w_slot, partials,    \
                       ticket, st, host, pq_out, h.max_nodes, h.max_owned, h.col_stride)
#define HFEM_CG_A(BLOCK, NPT, EPT)                                                                                            \
    do {                                                                                                                      \
        if (A.phys) HFEM_CG_OP(HFEM_CG_APPLY, BLOCK, NPT, EPT, true);                                                         \
        else HFEM_CG_OP(HFEM_CG_APPLY, BLOCK, NPT, EPT, false);                                                               \
    } while (0)
    if (A.block == 512) HFEM_CG_A(512, 2, 2);
    else if (h.max_nodes <= 3 * 256) {
        if (h.max_rows <= 3) HFEM_CG_A(256, 3, 3);
        else if (h.max_rows == 4) HFEM_CG_A(256, 3, 4);
        else HFEM_CG_A(256, 3, 6);
    } else {
        if (h.max_rows <= 3) HFEM_CG_A(256, 4, 3);
        else if (h.max_rows == 4) HFEM_CG_A(256, 4, 4);
        else HFEM_CG_A(256, 4, 6);
    }
#undef HFEM_CG_A
#undef HFEM_CG_APPLY
}

void launch_tri3_cg_diag(const CgElemArgs &A, double *diag, double *dinv, int precond) {
    const HostPlan &h = A.plan->host;
    const PlanDev pd = plan_dev(A.plan);
#define HFEM_CG_DIAG(BLOCK, NPT, EPT, PH, OP)                                                                                 \
    hipLaunchKernelGGL((tri3_cg_diag_kernel<BLOCK, NPT, EPT, PH, ElemOp::OP>), dim3(A.n_tiles), dim3(BLOCK), A.lds, A.s, pd,  \
                       A.x_free, A.x_fixed, A.k, A.dm, diag, dinv, (const double2 *)A.w_slot, precond, h.max_nodes,           \
                       h.max_owned, h.col_stride)
#define HFEM_CG_D(BLOCK, NPT, EPT)                                                                                            \
    do {                                                                                                                      \
        if (A.phys) HFEM_CG_OP(HFEM_CG_DIAG, BLOCK, NPT, EPT, true);                                                          \
        else HFEM_CG_OP(HFEM_CG_DIAG, BLOCK, NPT, EPT, false);                                                                \
    } while (0)
    if (A.block == 512) HFEM_CG_D(512, 2, 2);
    else HFEM_CG_D(256, 4, 6);
#undef HFEM_CG_D
#undef HFEM_CG_DIAG
}

}  // namespace hfem
