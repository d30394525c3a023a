// Frozen-mesh displacement solve on QUAD4, gfx950 (MI355X): the element kernels of the matrix-free PCG solve and of the AMG
// fine level for bilinear quadrilaterals (hidenn_fem_amd/solve.py, Quad4FrozenMeshSolver).  The PCG driver, the vector and
// r^T z kernels, the status record and the whole AMG hierarchy below the fine-level assembly are those of the TRI3 solve
// (tri3_cg.hip, tri3_amg.hip): nothing above the element level knows the element.  All fp64, both gradient conventions.
//   quad4_cg_apply_kernel   q = K p on the free u rows: the u-half of quad4_energy_fast_kernel (quad4.hip) at u = p on the
//                           model's own QUAD4 tile plan -- its clamped index loads, its gather, its slot loop (2x2 Gauss from
//                           LDS rows, ds_add_f64 on the owned corners) -- with the coordinate cotangent, the forces and the
//                           edges dropped (quad4_element_u, hfem_quad4_dev.h).  The contract is tri3_cg_apply_kernel's: the
//                           gather forms p = z + beta p_old, the owner tile stores p into the other ping-pong buffer, one
//                           p^T K p partial per tile over its home elements, the last workgroup (ticket) sums them in tile
//                           order and writes alpha; nothing runs once the status record says halted.
//   quad4_cg_diag_kernel    2x2 diagonal blocks of K (block Jacobi), once per refresh: per owned corner a of every element the
//                           block d2E/du_a^2 = the element's u-gradient at u_a = e_x / e_y, accumulated into the owner node.
//   quad4_amg_assemble_kernel  K_ff in 2x2 blocks for the AMG fine level: one thread per free row walks the row's element fan in
//                           ascending element order and adds columns (a, x), (a, y) of K_e through four fan slots per record.
//                           No atomics: bit-deterministic.
// The 2x2 rule's weights are 1, so the triangle weight sum W of the shared entry points is not read here.
#include <hip/hip_runtime.h>

#include "hfem_cg_dev.h"
#include "hfem_quad4_dev.h"

namespace hfem {
namespace {

constexpr int kAsmBlock = 256;

// ---------------------------------------------------------------- q = K p
// st != NULL: an iteration (p = z + beta p_old gathered, p stored to the other ping-pong buffer, alpha written);
// st == NULL: the standalone apply (p = z as given, pq_out[0] = p^T q).
// LDS: xy[cap_nodes] double2 | p[cap_nodes] double2 | acc[2][cap_owned] | red[BLOCK / 64 + 2]
template <int BLOCK, int NPT, int EPT, bool PHYS>
__global__ __launch_bounds__(BLOCK) void quad4_cg_apply_kernel(
    PlanDev pd, int n_tiles, const double2 *__restrict__ x_free, const double2 *__restrict__ x_fixed,
    const double2 *__restrict__ z, double2 *pbuf0, double2 *pbuf1, double2 *__restrict__ q, Tri3Consts k,
    double *__restrict__ partials, unsigned *ticket, double *st, double *host, double *pq_out, int cap_nodes, int cap_owned) {
    if (st && st[kHalted] != 0.0) return;                   // uniform over the grid: nothing is written after a halt
    extern __shared__ double2 lds[];
    double2 *nd_xy = lds, *nd_p = lds + cap_nodes;
    double *acc0 = reinterpret_cast<double *>(lds + 2 * cap_nodes), *acc1 = acc0 + cap_owned;
    double *red = acc1 + cap_owned;                         // BLOCK / 64 doubles + one flag word
    const int tid = threadIdx.x;
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
    mem_phase_begin();                                      // prologue at raised wave priority (hfem_plan_dev.h)
    // row maps and element records from the tile index alone (uniform strides), unguarded: lanes past a tile's records
    // repeat the stride's last one (a valid row / a skip record)
    int2 s[NPT];
    uint32_t pk[EPT], pk3[EPT];
    const int2 *src = pd.node_src + (size_t)slot * pd.node_stride;
    const size_t rec0 = (size_t)slot * pd.elem_stride;
#pragma unroll
    for (int j = 0; j < NPT; ++j) s[j] = src[min(tid + j * BLOCK, pd.node_stride - 1)];
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const size_t i = rec0 + min(tid + j * BLOCK, pd.elem_stride - 1);
        pk[j] = pd.elem_pack[i];
        pk3[j] = pd.elem_pack_hi[i];
    }
    const TileDesc d = pd.tiles[slot];
    const int n_owned = d.n_owned;
    // gather: coordinates through the x row map, p through the u row map (fixed u rows are 0)
    double vxx[NPT], vxy[NPT], vpx[NPT], vpy[NPT];          // plain doubles (double2 arrays end up in scratch)
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const double2 tx = *(s[j].x >= 0 ? x_free + s[j].x : x_fixed + ~s[j].x);
        vxx[j] = tx.x; vxy[j] = tx.y;
        vpx[j] = 0.0; vpy[j] = 0.0;
        if (s[j].y >= 0) {
            const double2 zz = z[s[j].y];
            vpx[j] = zz.x; vpy[j] = zz.y;
            if (p_old) {
                const double2 o = p_old[s[j].y];
                vpx[j] = __builtin_fma(beta, o.x, vpx[j]);
                vpy[j] = __builtin_fma(beta, o.y, vpy[j]);
            }
        }
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
            double2 Xn[4], Pn[4], gu[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                Xn[j] = nd_xy[l[j]];
                Pn[j] = nd_p[l[j]];
            }
            const double e = quad4_element_u<PHYS>(Xn, Pn, k, gu);
            if (p & kHomeBit) e_loc += e;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (l[j] < n_owned) {
                    unsafeAtomicAdd(&acc0[l[j]], gu[j].x);
                    unsafeAtomicAdd(&acc1[l[j]], gu[j].y);
                }
        }
    }
    {
        const double w = wave_sum(e_loc);
        if ((tid & 63) == 0) red[tid >> 6] = w;
    }
    __syncthreads();
    // owned free rows: q (one 16-byte store per row), and (iterations) the new p into the other buffer
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
// LDS: xy[cap_nodes] double2 | acc[3][cap_owned]
template <int BLOCK, int NPT, int EPT, bool PHYS>
__global__ __launch_bounds__(BLOCK) void quad4_cg_diag_kernel(PlanDev pd, const double2 *__restrict__ x_free,
                                                              const double2 *__restrict__ x_fixed, Tri3Consts k,
                                                              double *__restrict__ diag, double *__restrict__ dinv, int precond,
                                                              int cap_nodes, int cap_owned) {
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
    const double2 o = make_double2(0.0, 0.0), ex = make_double2(1.0, 0.0), ey = make_double2(0.0, 1.0);
    for (int j = 0; j < EPT; ++j) {
        if (tid + j * BLOCK >= d.n_elem) continue;
        const size_t i = (size_t)slot * pd.elem_stride + tid + j * BLOCK;
        const uint32_t p = pd.elem_pack[i];
        if (p & kSkipBit) continue;
        const int l[4] = {(int)(p & kLocalMask), (int)((p >> kLocalBits) & kLocalMask),
                          (int)((p >> (2 * kLocalBits)) & kLocalMask), (int)(pd.elem_pack_hi[i] & kLocalMask)};
        const double2 Xn[4] = {nd_xy[l[0]], nd_xy[l[1]], nd_xy[l[2]], nd_xy[l[3]]};
        // the corner blocks of one element: column c of K_aa = the gradient at u_a = e_c, u_b = 0 (b != a)
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            if (l[a] >= n_owned) continue;
            const double2 Ux[4] = {a == 0 ? ex : o, a == 1 ? ex : o, a == 2 ? ex : o, a == 3 ? ex : o};
            const double2 Uy[4] = {a == 0 ? ey : o, a == 1 ? ey : o, a == 2 ? ey : o, a == 3 ? ey : o};
            double2 gu[4], hu[4];
            quad4_element_u<PHYS>(Xn, Ux, k, gu);
            quad4_element_u<PHYS>(Xn, Uy, k, hu);
            unsafeAtomicAdd(&acc0[l[a]], gu[a].x);
            unsafeAtomicAdd(&acc1[l[a]], 0.5 * (gu[a].y + hu[a].x));
            unsafeAtomicAdd(&acc2[l[a]], hu[a].y);
        }
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

// ---------------------------------------------------------------- AMG fine level (2x2 blocks)
__device__ __forceinline__ double2 x_row(const double2 *x_free, const double2 *x_fixed, int32_t code) {
    return code >= 0 ? x_free[code] : x_fixed[-1 - code];
}

template <bool PHYS>
__global__ __launch_bounds__(kAsmBlock) void quad4_amg_assemble_kernel(int32_t n, const int32_t *__restrict__ fan_ptr,
                                                                       const int32_t *__restrict__ fan_elem,
                                                                       const int32_t *__restrict__ fan_corner,
                                                                       const int32_t *__restrict__ fan_slot,
                                                                       const int32_t *__restrict__ conn_x,
                                                                       const double2 *__restrict__ x_free,
                                                                       const double2 *__restrict__ x_fixed,
                                                                       const int32_t *__restrict__ a_ptr,
                                                                       double *__restrict__ a_val, Tri3Consts k) {
    const int32_t r = (int32_t)(blockIdx.x * kAsmBlock + threadIdx.x);
    if (r >= n) return;
    for (int32_t s = a_ptr[r]; s < a_ptr[r + 1]; ++s)
        *reinterpret_cast<double4 *>(a_val + 4 * (size_t)s) = make_double4(0.0, 0.0, 0.0, 0.0);
    const double2 o = make_double2(0.0, 0.0), ex = make_double2(1.0, 0.0), ey = make_double2(0.0, 1.0);
    for (int32_t f = fan_ptr[r]; f < fan_ptr[r + 1]; ++f) {
        const int32_t e = fan_elem[f], a = fan_corner[f];
        const int32_t *cx = conn_x + 4 * (size_t)e;
        const double2 Xn[4] = {x_row(x_free, x_fixed, cx[0]), x_row(x_free, x_fixed, cx[1]), x_row(x_free, x_fixed, cx[2]),
                               x_row(x_free, x_fixed, cx[3])};
        // column (a, x) and (a, y) of K_e = rows (a, x) and (a, y) by symmetry
        const double2 Ux[4] = {a == 0 ? ex : o, a == 1 ? ex : o, a == 2 ? ex : o, a == 3 ? ex : o};
        const double2 Uy[4] = {a == 0 ? ey : o, a == 1 ? ey : o, a == 2 ? ey : o, a == 3 ? ey : o};
        double2 gu[4], hu[4];
        quad4_element_u<PHYS>(Xn, Ux, k, gu);
        quad4_element_u<PHYS>(Xn, Uy, k, hu);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int32_t s = fan_slot[4 * (size_t)f + b];
            if (s < 0) continue;
            double4 *p = reinterpret_cast<double4 *>(a_val + 4 * (size_t)s);
            double4 v = *p;
            v.x += gu[b].x; v.y += gu[b].y; v.z += hu[b].x; v.w += hu[b].y;
            *p = v;
        }
    }
}

}  // namespace

// ---------------------------------------------------------------- launchers
// Tile shapes: what hfem_quad4_energy_plan_ex accepts (max_nodes <= 4 * 256, max_elems <= 4 * 256; hfem_cg_create refuses the
// rest), in the energy kernel's two register tilings: 3 nodes and 3 slots per thread (the default tile shape) or 4 and 4.
void launch_quad4_cg_apply(const Quad4CgArgs &A, const double2 *z, double2 *pbuf0, double2 *pbuf1, double2 *q, double *partials,
                           unsigned *ticket, double *st, double *host, double *pq_out) {
    const HostPlan &h = A.plan->host;
    const PlanDev pd = plan_dev(A.plan);
#define HFEM_Q4CG_APPLY(NPT, EPT, PH)                                                                                        \
    hipLaunchKernelGGL((quad4_cg_apply_kernel<256, NPT, EPT, PH>), dim3(A.n_tiles), dim3(256), A.lds, A.s, pd, A.n_tiles,    \
                       A.x_free, A.x_fixed, z, pbuf0, pbuf1, q, A.k, partials, ticket, st, host, pq_out, h.max_nodes,        \
                       h.max_owned)
    if (h.max_nodes <= 3 * 256 && h.max_elems <= 3 * 256) {
        if (A.phys) HFEM_Q4CG_APPLY(3, 3, true);
        else HFEM_Q4CG_APPLY(3, 3, false);
    } else {
        if (A.phys) HFEM_Q4CG_APPLY(4, 4, true);
        else HFEM_Q4CG_APPLY(4, 4, false);
    }
#undef HFEM_Q4CG_APPLY
}

void launch_quad4_cg_diag(const Quad4CgArgs &A, double *diag, double *dinv, int precond) {
    const HostPlan &h = A.plan->host;
    const PlanDev pd = plan_dev(A.plan);
#define HFEM_Q4CG_DIAG(PH)                                                                                                   \
    hipLaunchKernelGGL((quad4_cg_diag_kernel<256, 4, 4, PH>), dim3(A.n_tiles), dim3(256), A.lds, A.s, pd, A.x_free,          \
                       A.x_fixed, A.k, diag, dinv, precond, h.max_nodes, h.max_owned)
    if (A.phys) HFEM_Q4CG_DIAG(true);
    else HFEM_Q4CG_DIAG(false);
#undef HFEM_Q4CG_DIAG
}

void launch_quad4_amg_assemble(int32_t n, const int32_t *fan_ptr, const int32_t *fan_elem, const int32_t *fan_corner,
                               const int32_t *fan_slot, const int32_t *conn_x, const double2 *x_free, const double2 *x_fixed,
                               const int32_t *a_ptr, double *a_val, const Tri3Consts &k, bool phys, hipStream_t s) {
    const dim3 grid((unsigned)((n + kAsmBlock - 1) / kAsmBlock));
#define HFEM_Q4_ASM(PH)                                                                                                      \
    hipLaunchKernelGGL(quad4_amg_assemble_kernel<PH>, grid, dim3(kAsmBlock), 0, s, n, fan_ptr, fan_elem, fan_corner, fan_slot, \
                       conn_x, x_free, x_fixed, a_ptr, a_val, k)
    if (phys) HFEM_Q4_ASM(true);
    else HFEM_Q4_ASM(false);
#undef HFEM_Q4_ASM
}

}  // namespace hfem
