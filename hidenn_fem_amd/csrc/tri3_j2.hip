// Small-strain J2 elastoplasticity of a TRI3 model, gfx950 (MI355X) (hidenn_fem_amd/plasticity.py): the element
// kernels of the PCG driver's J2 operator kind (cg.hip, after hfem_cg_setup_j2) and the update launch of the state handle
// hfem_j2.  Siblings of the Neo-Hookean kernels (tri3_hyper.hip, tri3_hyper_cg.hip) on the same one-element-per-slot plan
// (plan_elem_order 3), with the phases of hfem_cg_dev.h; the element is hfem_j2_dev.h's.
//   tri3_j2_update_kernel   gathers the x and u rows; per slot: eps, the committed record of the element (by global element id
//                           through the handle's copy of elem_gid; home and halo copies read the same record), the return map,
//                           A B^T sigma into the owned rows with LDS atomics, A Psi of the home elements into the tile partial.
//                           On storing the owned rows it adds load * g_ext to the row and load * g_ext . u to the energy: the
//                           external load is not recomputed.  With `write`, home slots also store the trial state and the
//                           stress by element id.  Tile partials {energy, plastic home elements, max dgamma}; j2_finish_kernel
//                           (one block) reduces them to out = {Pi, plastic count, max dgamma}.
//   tri3_j2_diag_kernel     the linearisation launch: the same return map at u_lin; writes one tangent record
//                           {theta, theta_bar, n_xx, n_yy, n_xy} per slot, home and halo alike, as planes
//                           [n_tiles][5][elem_stride] (quad4_hyper_cg.hip's cq layout: coalesced, no index stream), the 2x2
//                           diagonal blocks through store_jacobi_block, and info = {plastic count, 0}.
//   tri3_j2_apply_kernel    q = K_T p, every CG iteration: gathers the x and p rows only (at small strain B depends on the
//                           coordinates alone), reads the slot's record in the round of elem_pack and holds it in registers:
//                           no u rows, no return map, no state by element id.  Home elements contribute 1/2 p_e . q_e.  The
//                           record of a skipped or padded slot is loaded and never used.
// The commit is a device copy trial -> committed: no kernel.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>

#include "hfem_cg_dev.h"
#include "hfem_j2_dev.h"

namespace hfem {
namespace {

constexpr int kBlock = 512, kNpt = 2, kEpt = 4, kFinishBlock = 256;

__device__ __forceinline__ double wave_max(double v) { return -wave_min(-v); }

// ---------------------------------------------------------------- update / energy
// LDS: xy[cap_nodes] double2 | uv[cap_nodes] double2 | acc[2][cap_owned] | red[3][BLOCK / 64]
template <int BLOCK, int NPT, int EPT>
__global__ __launch_bounds__(BLOCK) void tri3_j2_update_kernel(
    PlanDev pd, int n_tiles, const double2 *__restrict__ x_free, const double2 *__restrict__ x_fixed,
    const double2 *__restrict__ u_free, const double2 *__restrict__ u_fixed, J2Consts k, const int32_t *__restrict__ gid,
    const double4 *__restrict__ committed, double4 *__restrict__ trial, double4 *__restrict__ stress, int write,
    const double2 *__restrict__ g_ext, double load, double *__restrict__ work, double2 *__restrict__ g_out, int cap_nodes,
    int cap_owned) {
    static_assert(NPT * BLOCK >= kMaxLocal, "the row maps of a whole tile (<= 1024 local nodes) are held in registers");
    extern __shared__ double2 lds[];
    double2 *nd_xy = lds, *nd_uv = lds + cap_nodes;
    double *acc0 = reinterpret_cast<double *>(lds + 2 * cap_nodes), *acc1 = acc0 + cap_owned;
    double *red = acc1 + cap_owned;
    const int tid = threadIdx.x;
    const int slot = xcd_tile((int)blockIdx.x, n_tiles);
    int2 s[NPT];
    uint32_t pk[EPT];
    int32_t ge[EPT];
    const int2 *src = pd.node_src + (size_t)slot * pd.node_stride;
    const size_t rec0 = (size_t)slot * pd.elem_stride;
    const uint32_t *ep = pd.elem_pack + rec0;
#pragma unroll
    for (int j = 0; j < NPT; ++j) s[j] = src[min(tid + j * BLOCK, pd.node_stride - 1)];
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const int i = min(tid + j * BLOCK, pd.elem_stride - 1);
        pk[j] = ep[i];
        ge[j] = gid[rec0 + i];
    }
    const TileDesc d = pd.tiles[slot];
    const int n_owned = d.n_owned;
#pragma unroll
    for (int j = 0; j < EPT; ++j)
        if (tid + j * BLOCK >= d.n_elem) pk[j] = kSkipBit;
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int l = tid + j * BLOCK;
        const double2 vx = *(s[j].x >= 0 ? x_free + s[j].x : x_fixed + ~s[j].x);
        const double2 vu = *(s[j].y >= 0 ? u_free + s[j].y : u_fixed + ~s[j].y);
        if (l < d.n_node) { nd_xy[l] = vx; nd_uv[l] = vu; }
        if (l < n_owned) { acc0[l] = 0.0; acc1[l] = 0.0; }
    }
    __syncthreads();

    double e_loc = 0.0, n_pl = 0.0, dg_max = 0.0;
    auto element = [&](uint32_t p, int32_t g) {
        if ((p & kSkipBit) || g < 0) return;
        const int l0 = (int)(p & kLocalMask), l1 = (int)((p >> kLocalBits) & kLocalMask),
                  l2 = (int)((p >> (2 * kLocalBits)) & kLocalMask);
        const J2Geom ge_ = j2_geom(nd_xy[l0], nd_xy[l1], nd_xy[l2], k.W);
        double exx, eyy, exy;
        j2_strain(ge_, nd_uv[l0], nd_uv[l1], nd_uv[l2], exx, eyy, exy);
        const double4 c = committed[g];
        const J2Point r = j2_return_map(exx, eyy, exy, c.x, c.y, c.z, c.w, k);
        double2 q[3];
        j2_force(ge_, r.sxx, r.syy, r.sxy, q);
        if (p & kHomeBit) {
            e_loc += ge_.A * r.psi;
            n_pl += r.dgamma > 0.0 ? 1.0 : 0.0;
            dg_max = fmax(dg_max, r.dgamma);
            if (write) {
                trial[g] = make_double4(r.exx, r.eyy, r.exy, r.alpha);
                stress[g] = make_double4(r.sxx, r.syy, r.sxy, r.szz);
            }
        }
        if (l0 < n_owned) { unsafeAtomicAdd(&acc0[l0], q[0].x); unsafeAtomicAdd(&acc1[l0], q[0].y); }
        if (l1 < n_owned) { unsafeAtomicAdd(&acc0[l1], q[1].x); unsafeAtomicAdd(&acc1[l1], q[1].y); }
        if (l2 < n_owned) { unsafeAtomicAdd(&acc0[l2], q[2].x); unsafeAtomicAdd(&acc1[l2], q[2].y); }
    };
#pragma unroll
    for (int j = 0; j < EPT; ++j) element(pk[j], ge[j]);
    for (int i = tid + EPT * BLOCK; i < d.n_elem; i += BLOCK) element(ep[i], gid[rec0 + i]);
    __syncthreads();
    // ---- every owned free row is written exactly once, with the external load's row and its work
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int l = tid + j * BLOCK;
        if (l < n_owned && s[j].y >= 0) {
            double2 v = make_double2(acc0[l], acc1[l]);
            if (g_ext) {
                const double2 ge_ = g_ext[s[j].y], u = nd_uv[l];
                v.x = __builtin_fma(load, ge_.x, v.x); v.y = __builtin_fma(load, ge_.y, v.y);
                e_loc += load * (ge_.x * u.x + ge_.y * u.y);
            }
            g_out[s[j].y] = v;
        }
    }
    {
        const double we = wave_sum(e_loc), wc = wave_sum(n_pl), wm = wave_max(dg_max);
        if ((tid & 63) == 0) {
            red[tid >> 6] = we;
            red[BLOCK / 64 + (tid >> 6)] = wc;
            red[2 * (BLOCK / 64) + (tid >> 6)] = wm;
        }
    }
    __syncthreads();
    if (tid == 0) {                                     // wave order: the tile energy is bit-reproducible given the rows
        double te = 0.0, tc = 0.0, tm = 0.0;
#pragma unroll
        for (int w = 0; w < BLOCK / 64; ++w) {
            te += red[w];
            tc += red[BLOCK / 64 + w];
            tm = fmax(tm, red[2 * (BLOCK / 64) + w]);
        }
        work[slot] = te;
        work[n_tiles + slot] = tc;
        work[2 * n_tiles + slot] = tm;
    }
}

// out = {sum of the tile energies in tile order per thread and block_sum's order, plastic count, max dgamma}
__global__ __launch_bounds__(kFinishBlock) void j2_finish_kernel(const double *__restrict__ work, int n, double *__restrict__ out) {
    __shared__ double red_e[kFinishBlock / 64], red_c[kFinishBlock / 64], red_m[kFinishBlock / 64];
    double e = 0.0, c = 0.0, m = 0.0;
    for (int i = threadIdx.x; i < n; i += kFinishBlock) {
        e += work[i];
        c += work[n + i];
        m = fmax(m, work[2 * n + i]);
    }
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red_m[threadIdx.x >> 6] = m;
    const double te = block_sum(e, red_e), tc = block_sum(c, red_c);   // their barriers also order red_m
    if (threadIdx.x == 0) {
        double tm = red_m[0];
        for (int w = 1; w < kFinishBlock / 64; ++w) tm = fmax(tm, red_m[w]);
        out[0] = te;
        out[1] = tc;
        out[2] = tm;
    }
}

// ---------------------------------------------------------------- linearisation: tangent records + block Jacobi
// LDS: xy[cap_nodes] double2 | uv[cap_nodes] double2 | acc[3][cap_owned] | red[BLOCK / 64]
template <int BLOCK, int NPT>
__global__ __launch_bounds__(BLOCK) void tri3_j2_diag_kernel(
    PlanDev pd, int n_tiles, const double2 *__restrict__ x_free, const double2 *__restrict__ x_fixed,
    const double2 *__restrict__ u_free, const double2 *__restrict__ u_fixed, J2Consts k, const int32_t *__restrict__ gid,
    const double4 *__restrict__ committed, double *__restrict__ tan, double *__restrict__ diag, double *__restrict__ dinv,
    int precond, double *__restrict__ work, int cap_nodes, int cap_owned) {
    extern __shared__ double2 lds[];
    double2 *nd_xy = lds, *nd_uv = lds + cap_nodes;
    double *acc0 = reinterpret_cast<double *>(lds + 2 * cap_nodes), *acc1 = acc0 + cap_owned, *acc2 = acc1 + cap_owned;
    double *red = acc2 + cap_owned;
    const int tid = threadIdx.x;
    const int slot = (int)blockIdx.x;
    int2 s[NPT];
    const int2 *src = pd.node_src + (size_t)slot * pd.node_stride;
    const size_t rec0 = (size_t)slot * pd.elem_stride;
    const uint32_t *ep = pd.elem_pack + rec0;
    double *plane = tan + 5 * rec0;                         // this tile's five planes of elem_stride doubles
    const size_t es = (size_t)pd.elem_stride;
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
    double n_pl = 0.0;
    for (int i = tid; i < d.n_elem; i += BLOCK) {
        const uint32_t p = ep[i];
        const int32_t g = gid[rec0 + i];
        if ((p & kSkipBit) || g < 0) continue;
        const int l0 = (int)(p & kLocalMask), l1 = (int)((p >> kLocalBits) & kLocalMask),
                  l2 = (int)((p >> (2 * kLocalBits)) & kLocalMask);
        const J2Geom ge = j2_geom(nd_xy[l0], nd_xy[l1], nd_xy[l2], k.W);
        double exx, eyy, exy;
        j2_strain(ge, nd_uv[l0], nd_uv[l1], nd_uv[l2], exx, eyy, exy);
        const double4 c = committed[g];
        const J2Point r = j2_return_map(exx, eyy, exy, c.x, c.y, c.z, c.w, k);
        plane[i] = r.theta; plane[es + i] = r.theta_bar; plane[2 * es + i] = r.nxx; plane[3 * es + i] = r.nyy;
        plane[4 * es + i] = r.nxy;
        if (p & kHomeBit) n_pl += r.dgamma > 0.0 ? 1.0 : 0.0;
        // the corner blocks: column c of K_aa = row a of the apply at p_a = e_c, p_b = 0 (b != a)
        const double2 o = make_double2(0.0, 0.0), ex = make_double2(1.0, 0.0), ey = make_double2(0.0, 1.0);
        double2 gu[3], hu[3];
        if (l0 < n_owned) {
            j2_tangent_apply(ge, k, r.theta, r.theta_bar, r.nxx, r.nyy, r.nxy, ex, o, o, gu);
            j2_tangent_apply(ge, k, r.theta, r.theta_bar, r.nxx, r.nyy, r.nxy, ey, o, o, hu);
            unsafeAtomicAdd(&acc0[l0], gu[0].x); unsafeAtomicAdd(&acc1[l0], 0.5 * (gu[0].y + hu[0].x)); unsafeAtomicAdd(&acc2[l0], hu[0].y);
        }
        if (l1 < n_owned) {
            j2_tangent_apply(ge, k, r.theta, r.theta_bar, r.nxx, r.nyy, r.nxy, o, ex, o, gu);
            j2_tangent_apply(ge, k, r.theta, r.theta_bar, r.nxx, r.nyy, r.nxy, o, ey, o, hu);
            unsafeAtomicAdd(&acc0[l1], gu[1].x); unsafeAtomicAdd(&acc1[l1], 0.5 * (gu[1].y + hu[1].x)); unsafeAtomicAdd(&acc2[l1], hu[1].y);
        }
        if (l2 < n_owned) {
            j2_tangent_apply(ge, k, r.theta, r.theta_bar, r.nxx, r.nyy, r.nxy, o, o, ex, gu);
            j2_tangent_apply(ge, k, r.theta, r.theta_bar, r.nxx, r.nyy, r.nxy, o, o, ey, hu);
            unsafeAtomicAdd(&acc0[l2], gu[2].x); unsafeAtomicAdd(&acc1[l2], 0.5 * (gu[2].y + hu[2].x)); unsafeAtomicAdd(&acc2[l2], hu[2].y);
        }
    }
    {
        const double wc = wave_sum(n_pl);
        if ((tid & 63) == 0) red[tid >> 6] = wc;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int l = tid + j * BLOCK;
        if (l < n_owned && s[j].y >= 0) store_jacobi_block(diag, dinv, s[j].y, precond, acc0[l], acc1[l], acc2[l]);
    }
    if (tid == 0) {
        double tc = 0.0;
#pragma unroll
        for (int w = 0; w < BLOCK / 64; ++w) tc += red[w];
        work[slot] = tc;
    }
}

// info = {plastic home elements of the linearisation point, 0} from the diag launch's tile partials work[n]
__global__ __launch_bounds__(kFinishBlock) void j2_info_kernel(const double *__restrict__ work, int n, double *__restrict__ info) {
    __shared__ double red[kFinishBlock / 64];
    double c = 0.0;
    for (int i = threadIdx.x; i < n; i += kFinishBlock) c += work[i];
    const double tc = block_sum(c, red);
    if (threadIdx.x == 0) {
        info[0] = tc;
        info[1] = 0.0;
    }
}

// ---------------------------------------------------------------- q = K_T p
// st != NULL: an iteration; st == NULL: the standalone apply (tri3_hyper_cg_apply_kernel's contract).
// LDS: xy[cap_nodes] double2 | p[cap_nodes] double2 | acc[2][cap_owned] | red[BLOCK / 64 + 2]
template <int BLOCK, int NPT, int EPT>
__global__ __launch_bounds__(BLOCK) void tri3_j2_apply_kernel(
    PlanDev pd, int n_tiles, const double2 *__restrict__ x_free, const double2 *__restrict__ x_fixed,
    const double2 *__restrict__ z, double2 *pbuf0, double2 *pbuf1, double2 *__restrict__ q, J2Consts k,
    const double *__restrict__ tan, double *__restrict__ partials, unsigned *ticket, double *st, double *host, double *pq_out,
    int cap_nodes, int cap_owned) {
    static_assert(NPT * BLOCK >= kMaxLocal, "the row maps of a whole tile (<= 1024 local nodes) are held in registers");
    if (st && st[kHalted] != 0.0) return;                   // uniform over the grid: nothing is written after a halt
    extern __shared__ double2 lds[];
    double2 *nd_xy = lds, *nd_p = lds + cap_nodes;
    double *acc0 = reinterpret_cast<double *>(lds + 2 * cap_nodes), *acc1 = acc0 + cap_owned;
    double *red = acc1 + cap_owned;                         // BLOCK / 64 doubles + one flag word
    const int tid = threadIdx.x;
    const CgIter it = cg_iter(st, pbuf0, pbuf1);
    const int slot = xcd_tile((int)blockIdx.x, (int)gridDim.x);
    int2 s[NPT];
    uint32_t pk[EPT];
    double th[EPT], tb[EPT], nx[EPT], ny[EPT], nz[EPT];     // the slots' records (plain doubles, constant indices)
    const int2 *src = pd.node_src + (size_t)slot * pd.node_stride;
    const size_t rec0 = (size_t)slot * pd.elem_stride, es = (size_t)pd.elem_stride;
    const uint32_t *ep = pd.elem_pack + rec0;
    const double *plane = tan + 5 * rec0;
#pragma unroll
    for (int j = 0; j < NPT; ++j) s[j] = src[min(tid + j * BLOCK, pd.node_stride - 1)];
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const int i = min(tid + j * BLOCK, pd.elem_stride - 1);
        pk[j] = ep[i];
        th[j] = plane[i]; tb[j] = plane[es + i]; nx[j] = plane[2 * es + i]; ny[j] = plane[3 * es + i]; nz[j] = plane[4 * es + i];
    }
    const TileDesc d = pd.tiles[slot];
    const int n_owned = d.n_owned;
#pragma unroll
    for (int j = 0; j < EPT; ++j)
        if (tid + j * BLOCK >= d.n_elem) pk[j] = kSkipBit;
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int l = tid + j * BLOCK;
        const double2 vx = *(s[j].x >= 0 ? x_free + s[j].x : x_fixed + ~s[j].x);
        const double2 vp = gather_p(it, z, s[j].y);
        if (l < d.n_node) { nd_xy[l] = vx; nd_p[l] = vp; }
        if (l < n_owned) { acc0[l] = 0.0; acc1[l] = 0.0; }
    }
    __syncthreads();

    double e_loc = 0.0;
    auto element = [&](uint32_t p, double theta, double theta_bar, double nxx, double nyy, double nxy) {
        if (p & kSkipBit) return;
        const int l0 = (int)(p & kLocalMask), l1 = (int)((p >> kLocalBits) & kLocalMask),
                  l2 = (int)((p >> (2 * kLocalBits)) & kLocalMask);
        const J2Geom g = j2_geom(nd_xy[l0], nd_xy[l1], nd_xy[l2], k.W);
        double2 qe[3];
        const double pq = j2_tangent_apply(g, k, theta, theta_bar, nxx, nyy, nxy, nd_p[l0], nd_p[l1], nd_p[l2], qe);
        if (p & kHomeBit) e_loc += 0.5 * pq;
        if (l0 < n_owned) { unsafeAtomicAdd(&acc0[l0], qe[0].x); unsafeAtomicAdd(&acc1[l0], qe[0].y); }
        if (l1 < n_owned) { unsafeAtomicAdd(&acc0[l1], qe[1].x); unsafeAtomicAdd(&acc1[l1], qe[1].y); }
        if (l2 < n_owned) { unsafeAtomicAdd(&acc0[l2], qe[2].x); unsafeAtomicAdd(&acc1[l2], qe[2].y); }
    };
#pragma unroll
    for (int j = 0; j < EPT; ++j) element(pk[j], th[j], tb[j], nx[j], ny[j], nz[j]);
    for (int i = tid + EPT * BLOCK; i < d.n_elem; i += BLOCK) {
        const uint32_t p = ep[i];
        if (p & kSkipBit) continue;                         // the record of a skipped slot is not even loaded here
        element(p, plane[i], plane[es + i], plane[2 * es + i], plane[3 * es + i], plane[4 * es + i]);
    }
    wave_energy(e_loc, red);
    __syncthreads();
    store_q_p<BLOCK>(s, n_owned, acc0, acc1, nd_p, q, it.p_new);
    apply_finish<BLOCK>(red, partials, slot, ticket, n_tiles, st, host, pq_out);
}

}  // namespace

// ---------------------------------------------------------------- launchers of the driver's J2 kind (A.lds: the driver's)
void launch_tri3_j2_apply(const CgElemArgs &A, const double2 *z, double2 *pbuf0, double2 *pbuf1, double2 *q, double *partials,
                          unsigned *ticket, double *st, double *host, double *pq_out) {
    const HostPlan &h = A.plan->host;
    if (A.n_tiles <= 0) return;
    hipLaunchKernelGGL((tri3_j2_apply_kernel<kBlock, kNpt, kEpt>), dim3(A.n_tiles), dim3(kBlock), A.lds, A.s, plan_dev(A.plan),
                       A.n_tiles, A.x_free, A.x_fixed, z, pbuf0, pbuf1, q, A.j2->k, A.j2_tan, partials, ticket, st, host, pq_out,
                       h.max_nodes, h.max_owned);
}

void launch_tri3_j2_diag(const CgElemArgs &A, double *diag, double *dinv, int precond, double *work, double *info) {
    const HostPlan &h = A.plan->host;
    if (A.n_tiles > 0)
        hipLaunchKernelGGL((tri3_j2_diag_kernel<kBlock, kNpt>), dim3(A.n_tiles), dim3(kBlock), A.lds, A.s, plan_dev(A.plan),
                           A.n_tiles, A.x_free, A.x_fixed, A.u_lin_free, A.u_fixed, A.j2->k, A.j2->gid,
                           (const double4 *)A.j2->committed, A.j2_tan, diag, dinv, precond, work, h.max_nodes, h.max_owned);
    if (info) hipLaunchKernelGGL(j2_info_kernel, dim3(1), dim3(kFinishBlock), 0, A.s, work, A.n_tiles, info);
}

}  // namespace hfem

using namespace hfem;

// ---------------------------------------------------------------- the state handle
extern "C" int hfem_j2_create(hfem_plan *plan, int64_t ne, const double mat[4], double W, hfem_j2 **out) {
    HFEM_ARG_CHECK(plan && mat && out, "null pointer");
    *out = nullptr;
    HFEM_ARG_CHECK(plan->device >= 0, "host-only plan (created with device < 0) cannot launch");
    const HostPlan &h = plan->host;
    HFEM_ARG_CHECK(h.npe == 3 && !h.paired, "the J2 kernels read a TRI3 plan with one element per slot (plan_elem_order 3)");
    HFEM_ARG_CHECK(h.max_nodes <= kMaxLocal && h.max_owned <= h.max_nodes, "tile shape outside the J2 kernels' instance");
    HFEM_ARG_CHECK(std::isfinite(mat[0]) && std::isfinite(mat[1]) && mat[0] > 0.0 && mat[1] > 0.0, "mu and kappa must be finite and > 0");
    HFEM_ARG_CHECK(std::isfinite(mat[2]) && mat[2] > 0.0, "sigma_y must be finite and > 0");
    HFEM_ARG_CHECK(std::isfinite(mat[3]) && mat[3] >= 0.0, "the hardening modulus must be finite and >= 0");
    HFEM_ARG_CHECK(std::isfinite(W) && W > 0.0, "W must be finite and > 0");
    HFEM_ARG_CHECK(ne > 0 && ne < ((int64_t)1 << 31), "ne must be in [1, 2^31)");
    const size_t n_slots = h.tiles.size() * (size_t)h.elem_stride;
    HFEM_ARG_CHECK(h.elem_gid.size() >= n_slots, "the plan holds no element ids per slot");
    int64_t top = -1;
    for (size_t i = 0; i < n_slots; ++i) top = std::max<int64_t>(top, h.elem_gid[i]);
    HFEM_ARG_CHECK(top < ne, "ne is smaller than the plan's element count");
    const size_t lds = (size_t)h.max_nodes * 32 + (size_t)h.max_owned * 16 + 3 * (kBlock / 64) * sizeof(double);
    HFEM_ARG_CHECK(lds <= 64 * 1024, "tile needs more than 64 KiB of LDS");
    if (int rc = use_device(plan->device)) return rc;
    std::unique_ptr<hfem_j2> j(new hfem_j2);
    j->plan = plan; j->device = plan->device; j->ne = ne; j->n_slots = (int64_t)n_slots; j->n_tiles = (int)h.tiles.size();
    j->k.mu = mat[0]; j->k.kappa = mat[1]; j->k.sigma_y = mat[2]; j->k.hard = mat[3]; j->k.W = W;
    j->lds_update = lds;
    const size_t st_bytes = 3 * (size_t)ne * 32, wk_bytes = 3 * (size_t)std::max(j->n_tiles, 1) * 8;
    bool bad = hipMalloc((void **)&j->gid, std::max<size_t>(n_slots, 1) * 4) != hipSuccess ||
               (n_slots && hipMemcpy(j->gid, h.elem_gid.data(), n_slots * 4, hipMemcpyHostToDevice) != hipSuccess) ||
               hipMalloc((void **)&j->committed, st_bytes + wk_bytes) != hipSuccess ||
               hipMemset(j->committed, 0, st_bytes + wk_bytes) != hipSuccess;
    if (bad) {
        if (j->gid) (void)hipFree(j->gid);
        if (j->committed) (void)hipFree(j->committed);
        set_error("hfem_j2_create: device allocation or upload failed");
        return 1;
    }
    j->trial = j->committed + 4 * (size_t)ne;
    j->stress = j->trial + 4 * (size_t)ne;
    j->work = j->stress + 4 * (size_t)ne;
    *out = j.release();
    return 0;
}

extern "C" int hfem_j2_destroy(hfem_j2 *j) {
    if (!j) return 0;
    if (j->device >= 0) (void)hipSetDevice(j->device);
    if (j->gid) (void)hipFree(j->gid);
    if (j->committed) (void)hipFree(j->committed);
    delete j;
    return 0;
}

extern "C" int64_t hfem_j2_slots(const hfem_j2 *j) {
    if (!j) {
        set_error("hfem_j2_slots: null pointer");
        return -1;
    }
    return 5 * j->n_slots;
}

extern "C" int hfem_j2_update(hfem_j2 *j, const double *x_free, const double *x_fixed, const double *u_free, const double *u_fixed,
                              const double *g_ext, double load, int32_t write_state, double *out, double *g_out, void *stream) {
    HFEM_ARG_CHECK(j && out && g_out, "null pointer");
    HFEM_ARG_CHECK(x_free && u_free, "x_free / u_free must be given");
    HFEM_ARG_CHECK(std::isfinite(load), "load must be finite");
    HFEM_ARG_CHECK(write_state == 0 || write_state == 1, "write_state: 0 or 1");
    bool fixed_x = false, fixed_u = false;
    const HostPlan &h = j->plan->host;
    for (size_t i = 0; i + 1 < h.node_src.size(); i += 2) {
        fixed_x = fixed_x || h.node_src[i] < 0;
        fixed_u = fixed_u || h.node_src[i + 1] < 0;
    }
    HFEM_ARG_CHECK(x_fixed || !fixed_x, "the plan reads fixed coordinate rows: x_fixed must be given");
    HFEM_ARG_CHECK(u_fixed || !fixed_u, "the plan reads Dirichlet rows: u_fixed must be given");
    if (int rc = use_device(j->device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (j->n_tiles > 0) {
        hipLaunchKernelGGL((tri3_j2_update_kernel<kBlock, kNpt, kEpt>), dim3(j->n_tiles), dim3(kBlock), j->lds_update, s,
                           plan_dev(j->plan), j->n_tiles, (const double2 *)x_free, (const double2 *)x_fixed, (const double2 *)u_free,
                           (const double2 *)u_fixed, j->k, j->gid, (const double4 *)j->committed, (double4 *)j->trial,
                           (double4 *)j->stress, (int)write_state, (const double2 *)g_ext, load, j->work, (double2 *)g_out,
                           h.max_nodes, h.max_owned);
        if (int rc = launch_status("hfem_j2_update")) return rc;
    }
    hipLaunchKernelGGL(j2_finish_kernel, dim3(1), dim3(kFinishBlock), 0, s, j->work, j->n_tiles, out);
    return launch_status("hfem_j2_update(finish)");
}

// which: 0 committed, 1 trial, 2 stress
static double *j2_array(hfem_j2 *j, int32_t which) { return which == 0 ? j->committed : which == 1 ? j->trial : j->stress; }

extern "C" int hfem_j2_commit(hfem_j2 *j, void *stream) {
    HFEM_ARG_CHECK(j, "null pointer");
    if (int rc = use_device(j->device)) return rc;
    HFEM_HIP_CHECK(hipMemcpyAsync(j->committed, j->trial, (size_t)j->ne * 32, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

extern "C" int hfem_j2_get(hfem_j2 *j, int32_t which, double *out, void *stream) {
    HFEM_ARG_CHECK(j && out, "null pointer");
    HFEM_ARG_CHECK(which >= 0 && which <= 2, "which: 0 committed, 1 trial, 2 stress");
    if (int rc = use_device(j->device)) return rc;
    HFEM_HIP_CHECK(hipMemcpyAsync(out, j2_array(j, which), (size_t)j->ne * 32, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

extern "C" int hfem_j2_set(hfem_j2 *j, const double *state, void *stream) {
    HFEM_ARG_CHECK(j, "null pointer");
    if (int rc = use_device(j->device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (state) {
        HFEM_HIP_CHECK(hipMemcpyAsync(j->committed, state, (size_t)j->ne * 32, hipMemcpyDeviceToDevice, s));
        HFEM_HIP_CHECK(hipMemcpyAsync(j->trial, state, (size_t)j->ne * 32, hipMemcpyDeviceToDevice, s));
    } else {
        HFEM_HIP_CHECK(hipMemsetAsync(j->committed, 0, 2 * (size_t)j->ne * 32, s));   // committed | trial
    }
    HFEM_HIP_CHECK(hipMemsetAsync(j->stress, 0, (size_t)j->ne * 32, s));
    return 0;
}
