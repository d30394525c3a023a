// Frozen-mesh displacement solve on QUAD4, gfx950 (MI355X): the element kernels of the matrix-free PCG solve for bilinear
// quadrilaterals (hidenn_fem_amd/solve.py, Quad4FrozenMeshSolver).  The PCG driver (cg.hip) launches them through
// launch_quad4_cg_apply / launch_quad4_cg_diag; the phases they share with the TRI3 kernels (tri3_cg.hip) -- iteration state,
// p rows, write-out, the p^T q epilogue, the Jacobi block store -- are hfem_cg_dev.h's, and the AMG fine level of a QUAD4
// model is assembled by tri3_amg.hip's one kernel.  All fp64, both gradient conventions.
//   quad4_cg_apply_kernel   q = K p on the free u rows: the u-half of quad4_energy_fast_kernel (quad4.hip) at u = p on the
//                           model's own QUAD4 tile plan -- its clamped index loads, its gather, its slot loop (2x2 Gauss from
//                           LDS rows, ds_add_f64 on the owned corners) -- with the coordinate cotangent, the forces and the
//                           edges dropped (quad4_element_u, hfem_quad4_dev.h).  The contract is tri3_cg_apply_kernel's: the
//                           gather forms p = z + beta p_old, the owner tile stores p into the other ping-pong buffer, one
//                           p^T K p partial per tile over its home elements, the last workgroup (ticket) sums them in tile
//                           order and writes alpha; nothing runs once the status record says halted.
//   quad4_cg_diag_kernel    2x2 diagonal blocks of K (block Jacobi), once per refresh: per owned corner a of every element the
//                           block d2E/du_a^2 = the element's u-gradient at u_a = e_x / e_y, accumulated into the owner node.
// The 2x2 rule's weights are 1, so the triangle weight sum W of the shared entry points is not read here.
//
// Every kernel here is one frame in three instances of the operator tag ElemOp (hfem_cg_dev.h), which the launchers pick:
// Plain is K as above.
//
// ElemOp::Mass is the shifted operator A = c_K K + c_M M of a Newmark step (hidenn_fem_amd/dynamics.py), which the
// launchers pick once hfem_cg_setup_shifted has bound the solver: the same kernels with the mass code compiled in.  The
// stiffness part is quad4_element_u on material constants the host scaled by c_K; the mass part is formed in the slot loop
// from the corner rows the element already holds:
//   M_e[a][b] = sum_q |det J_q| N_a(q) (m_off N_b(q) + m_dd delta_ab),  2x2 Gauss points
//   (M_e p)_a = sum_q |det J_q| N_a(q) (m_off p_h(q) + m_dd p_a),  p_h(q) = sum_b N_b(q) p_b
// consistent: m_off = c_M, m_dd = 0; lumped (the row sum on the diagonal): m_off = 0, m_dd = c_M (DynMass, hfem_cg_dev.h; c_M
// includes the density; run-time coefficients, not instances).  Always |det J_q|: no gradient convention enters the mass.
// The tile energy is c_K e + 1/2 c_M p^T M_e p, so apply_finish's p^T q = 2 x sum stays right.  The diag kernel adds
// M_e[a][a] to xx and yy of every block.  The other instances take the DynMass argument and do not read it.
//
// ElemOp::Scaled is the element-scaled stiffness K(w) = sum_e w_e K_e, picked once hfem_cg_setup_scaled has bound
// w_slot: one double per slot of the plan, addressed and loaded as elem_pack (tri3_cg.hip has the reasons), multiplied into the
// element's gradient rows and energy in the slot loop and into its block entries in the diag kernel.  The other instances
// take the w_slot argument and do not read it.
#include <hip/hip_runtime.h>

#include "hfem_cg_dev.h"

namespace hfem {
namespace {

// ---------------------------------------------------------------- q = K p (Mass: q = A p; Scaled: q = K(w) p)
// st != NULL: an iteration (p = z + beta p_old gathered, p stored to the other ping-pong buffer, alpha written);
// st == NULL: the standalone apply (p = z as given, pq_out[0] = p^T q).  Mass: k is the material constants times c_K.
// LDS: xy[cap_nodes] double2 | p[cap_nodes] double2 | acc[2][cap_owned] | red[BLOCK / 64 + 2]
template <int BLOCK, int NPT, int EPT, bool PHYS, ElemOp OP>
__global__ __launch_bounds__(BLOCK) void quad4_cg_apply_kernel(
    PlanDev pd, int n_tiles, const double2 *__restrict__ x_free, const double2 *__restrict__ x_fixed,
    const double2 *__restrict__ z, double2 *pbuf0, double2 *pbuf1, double2 *__restrict__ q, Tri3Consts k, DynMass dm,
    const double *__restrict__ w_slot, double *__restrict__ partials, unsigned *ticket, double *st, double *host, double *pq_out,
    int cap_nodes, int cap_owned) {
    if (st && st[kHalted] != 0.0) return;                   // uniform over the grid: nothing is written after a halt
    extern __shared__ double2 lds[];
    double2 *nd_xy = lds, *nd_p = lds + cap_nodes;
    double *acc0 = reinterpret_cast<double *>(lds + 2 * cap_nodes), *acc1 = acc0 + cap_owned;
    double *red = acc1 + cap_owned;                         // BLOCK / 64 doubles + one flag word
    const int tid = threadIdx.x;
    const CgIter it = cg_iter(st, pbuf0, pbuf1);
    const int slot = xcd_tile((int)blockIdx.x, (int)gridDim.x);
    mem_phase_begin();                                      // prologue at raised wave priority (hfem_plan_dev.h)
    // row maps and element records from the tile index alone (uniform strides), unguarded: lanes past a tile's records
    // repeat the stride's last one (a valid row / a skip record)
    int2 s[NPT];
    uint32_t pk[EPT], pk3[EPT];
    double we[EPT];                                         // Scaled: the slot's weight
    const int2 *src = pd.node_src + (size_t)slot * pd.node_stride;
    const size_t rec0 = (size_t)slot * pd.elem_stride;
#pragma unroll
    for (int j = 0; j < NPT; ++j) s[j] = src[min(tid + j * BLOCK, pd.node_stride - 1)];
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const size_t i = rec0 + min(tid + j * BLOCK, pd.elem_stride - 1);
        pk[j] = pd.elem_pack[i];
        pk3[j] = pd.elem_pack_hi[i];
        if constexpr (OP == ElemOp::Scaled) we[j] = w_slot[i];
    }
    const TileDesc d = pd.tiles[slot];
    const int n_owned = d.n_owned;
    // gather: coordinates through the x row map, p through the u row map (fixed u rows are 0)
    double vxx[NPT], vxy[NPT], vpx[NPT], vpy[NPT];          // plain doubles (double2 arrays end up in scratch)
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const double2 tx = *(s[j].x >= 0 ? x_free + s[j].x : x_fixed + ~s[j].x);
        vxx[j] = tx.x; vxy[j] = tx.y;
        const double2 tp = gather_p(it, z, s[j].y);
        vpx[j] = tp.x; vpy[j] = tp.y;
    }
#pragma unroll
    for (int j = 0; j < EPT; ++j)
        if (tid + j * BLOCK >= d.n_elem) { pk[j] = kSkipBit; pk3[j] = 0u; }
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int l = tid + j * BLOCK;
        if (l < d.n_node) { nd_xy[l] = make_double2(vxx[j], vxy[j]); nd_p[l] = make_double2(vpx[j], vpy[j]); }
        if (l < n_owned) { acc0[l] = 0.0; acc1[l] = 0.0; }
    }
    __syncthreads();
    mem_phase_end();
    double e_loc = 0.0;
#pragma unroll
    for (int jj = 0; jj < EPT; ++jj) {
        const uint32_t p = pk[jj];
        if (!(p & kSkipBit)) {
            const int l[4] = {(int)(p & kLocalMask), (int)((p >> kLocalBits) & kLocalMask),
                              (int)((p >> (2 * kLocalBits)) & kLocalMask), (int)(pk3[jj] & kLocalMask)};
            double w = 0.0;                                 // the element's weight (Scaled only)
            if constexpr (OP == ElemOp::Scaled) w = we[jj];
            double2 Xn[4], Pn[4], gu[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                Xn[j] = nd_xy[l[j]];
                Pn[j] = nd_p[l[j]];
            }
            double e = quad4_element_u<PHYS>(Xn, Pn, k, gu);
            if constexpr (OP == ElemOp::Mass) e += quad4_mass_rows(Xn, Pn, dm, gu);
            if constexpr (OP == ElemOp::Scaled) {
                if (p & kHomeBit) e_loc += w * e;
            } else {
                if (p & kHomeBit) e_loc += e;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (l[j] < n_owned) {
                    unsafeAtomicAdd(&acc0[l[j]], with_weight<OP>(gu[j].x, w));
                    unsafeAtomicAdd(&acc1[l[j]], with_weight<OP>(gu[j].y, w));
                }
        }
    }
    wave_energy(e_loc, red);
    __syncthreads();
    store_q_p<BLOCK>(s, n_owned, acc0, acc1, nd_p, q, it.p_new);
    apply_finish<BLOCK>(red, partials, slot, ticket, n_tiles, st, host, pq_out);
}

// ---------------------------------------------------------------- block-Jacobi setup
// Mass: the 2x2 diagonal blocks of A, the mass on xx and yy: M_e[a][a] = sum_q |det J_q| N_a(q) (m_off N_a(q) + m_dd).
// Scaled: the element's block entries times its weight.
// LDS: xy[cap_nodes] double2 | acc[3][cap_owned]
template <int BLOCK, int NPT, int EPT, bool PHYS, ElemOp OP>
__global__ __launch_bounds__(BLOCK) void quad4_cg_diag_kernel(PlanDev pd, const double2 *__restrict__ x_free,
                                                              const double2 *__restrict__ x_fixed, Tri3Consts k, DynMass dm,
                                                              double *__restrict__ diag, double *__restrict__ dinv,
                                                              const double *__restrict__ w_slot, int precond, int cap_nodes,
                                                              int cap_owned) {
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
        if (l < d.n_node) nd_xy[l] = *(s[j].x >= 0 ? x_free + s[j].x : x_fixed + ~s[j].x);
        if (l < n_owned) { acc0[l] = 0.0; acc1[l] = 0.0; acc2[l] = 0.0; }
    }
    __syncthreads();
    for (int j = 0; j < EPT; ++j) {
        if (tid + j * BLOCK >= d.n_elem) continue;
        const size_t i = (size_t)slot * pd.elem_stride + tid + j * BLOCK;
        const uint32_t p = pd.elem_pack[i];
        if (p & kSkipBit) continue;
        double w = 0.0;                                     // the element's weight (Scaled only)
        if constexpr (OP == ElemOp::Scaled) w = w_slot[i];
        const int l[4] = {(int)(p & kLocalMask), (int)((p >> kLocalBits) & kLocalMask),
                          (int)((p >> (2 * kLocalBits)) & kLocalMask), (int)(pd.elem_pack_hi[i] & kLocalMask)};
        const double2 Xn[4] = {nd_xy[l[0]], nd_xy[l[1]], nd_xy[l[2]], nd_xy[l[3]]};
        double ad[4];                                       // |det J_q| (MASS only)
        if constexpr (MASS) quad4_abs_dets(Xn, ad);
        // the corner blocks of one element: column c of K_aa = the gradient at u_a = e_c, u_b = 0 (b != a)
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            if (l[a] >= n_owned) continue;
            double mm = 0.0;                                // M_e[a][a] (MASS only)
            if constexpr (MASS) {
#pragma unroll
                for (int q = 0; q < 4; ++q) mm += ad[q] * quad4_n(a, q) * (dm.m_off * quad4_n(a, q) + dm.m_dd);
            }
            double2 gu[4], hu[4];
            unit_columns<PHYS>(Xn, a, k, gu, hu);
            unsafeAtomicAdd(&acc0[l[a]], with_weight<OP>(with_mass<MASS>(gu[a].x, mm), w));
            unsafeAtomicAdd(&acc1[l[a]], with_weight<OP>(0.5 * (gu[a].y + hu[a].x), w));
            unsafeAtomicAdd(&acc2[l[a]], with_weight<OP>(with_mass<MASS>(hu[a].y, mm), w));
        }
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
// Tile shapes: what hfem_quad4_energy_plan_ex accepts (max_nodes <= 4 * 256, max_elems <= 4 * 256; hfem_cg_create refuses the
// rest), in the energy kernel's two register tilings: 3 nodes and 3 slots per thread (the default tile shape) or 4 and 4.
// Each in both gradient conventions (A.phys) and the three operators (HFEM_CG_OP: A.shifted, A.w_slot, neither).
void launch_quad4_cg_apply(const CgElemArgs &A, const double2 *z, double2 *pbuf0, double2 *pbuf1, double2 *q, double *partials,
                           unsigned *ticket, double *st, double *host, double *pq_out) {
    const HostPlan &h = A.plan->host;
    const PlanDev pd = plan_dev(A.plan);
#define HFEM_Q4CG_APPLY(NPT, EPT, PH, OP)                                                                                    \
    hipLaunchKernelGGL((quad4_cg_apply_kernel<256, NPT, EPT, PH, ElemOp::OP>), dim3(A.n_tiles), dim3(256), A.lds, A.s, pd,   \
                       A.n_tiles, A.x_free, A.x_fixed, z, pbuf0, pbuf1, q, A.k, A.dm, A.w_slot, partials, ticket, st, host,  \
                       pq_out, h.max_nodes, h.max_owned)
#define HFEM_Q4CG_A(NPT, EPT)                                                                                                \
    do {                                                                                                                     \
        if (A.phys) HFEM_CG_OP(HFEM_Q4CG_APPLY, NPT, EPT, true);                                                             \
        else HFEM_CG_OP(HFEM_Q4CG_APPLY, NPT, EPT, false);                                                                   \
    } while (0)
    if (h.max_nodes <= 3 * 256 && h.max_elems <= 3 * 256) HFEM_Q4CG_A(3, 3);
    else HFEM_Q4CG_A(4, 4);
#undef HFEM_Q4CG_A
#undef HFEM_Q4CG_APPLY
}

void launch_quad4_cg_diag(const CgElemArgs &A, double *diag, double *dinv, int precond) {
    const HostPlan &h = A.plan->host;
    const PlanDev pd = plan_dev(A.plan);
#define HFEM_Q4CG_DIAG(PH, OP)                                                                                               \
    hipLaunchKernelGGL((quad4_cg_diag_kernel<256, 4, 4, PH, ElemOp::OP>), dim3(A.n_tiles), dim3(256), A.lds, A.s, pd,        \
                       A.x_free, A.x_fixed, A.k, A.dm, diag, dinv, A.w_slot, precond, h.max_nodes, h.max_owned)
    if (A.phys) HFEM_CG_OP(HFEM_Q4CG_DIAG, true);
    else HFEM_CG_OP(HFEM_Q4CG_DIAG, false);
#undef HFEM_Q4CG_DIAG
}

}  // namespace hfem
