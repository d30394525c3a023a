// Compressible Neo-Hookean total potential of a QUAD4 model on the owner-computes tile plan, gfx950.
// No reference counterpart: every energy of the reference is small-strain linear elasticity.
//
// The model's own QUAD4 plan: one cell per slot, two words per record ({l0 | l1<<10 | l2<<20 | home | skip} in elem_pack,
// {l3} in elem_pack_hi), uniform node and slot strides.  Phases as in tri3_hyper_kernel and quad4_energy_fast_kernel: row maps
// and slot records requested up front from the tile index alone (NPT / EPT of them into registers, unguarded clamped loads into
// the plan's padding), rows gathered to LDS (float rows widened), the four owned-row accumulators cleared, the slot loop
// accumulating the owned corners with LDS atomics, edges (dead loads, edge2_element unchanged) on boundary tiles, every owned
// row written exactly once, the tile partials summed in wave order.  NPT x BLOCK covers the 1024 local nodes a tile can have; a
// tile with more than EPT x BLOCK slots goes on in a plain loop behind the prefetched records, so every plan shape within
// 64 KiB of LDS runs through the one kernel (the linear QUAD4 kernel refuses such tiles).  The register budget is the
// compiler's (DESIGN 19 quotes it).
//
// Three partials per tile -- energy, min J over the Gauss points, number of inverted cells, over HOME cells -- go to a
// caller-provided workspace work[3][n_tiles]; quad4_hyper_finish_kernel (one block) sums the energies in
// hyper_finish_thread's order and reduces the other two.  The plan's partials banks and bank state are not touched.  The entry
// point only launches.
#include <hip/hip_runtime.h>

#include "hfem_device.h"
#include "hfem_plan_dev.h"
#include "hfem_quad4_hyper_dev.h"

namespace hfem {

constexpr int kQHyperBlock = 256, kQHyperNpt = 4, kQHyperEpt = 3, kQHyperFinish = 256;

// LDS: xy[cap_nodes] double2 | uv[cap_nodes] double2 | acc[4][cap_owned] double | red[3][BLOCK/64]
template <int BLOCK, int NPT, int EPT, typename V2, bool HASB>
__global__ __launch_bounds__(BLOCK) void quad4_hyper_kernel(
    PlanDev pd, const V2 *__restrict__ x_free, const V2 *__restrict__ x_fixed, const V2 *__restrict__ u_free,
    const V2 *__restrict__ u_fixed, Quad4HyperConsts k, const double4 *__restrict__ T_edge, double4 Tconst,
    double *__restrict__ work, int n_tiles, V2 *__restrict__ gx_free, V2 *__restrict__ gu_free, int cap_nodes,
    int cap_owned, int skip_edges) {
    static_assert(NPT * BLOCK >= kMaxLocal, "the row maps of a whole tile (<= 1024 local nodes) are held in registers");
    extern __shared__ double2 lds[];
    double2 *nd_xy = lds;
    double2 *nd_uv = lds + cap_nodes;
    double *acc0 = reinterpret_cast<double *>(lds + 2 * cap_nodes);
    double *acc1 = acc0 + cap_owned, *acc2 = acc1 + cap_owned, *acc3 = acc2 + cap_owned;
    double *red = acc3 + cap_owned;

    const int tid = threadIdx.x;
    const int slot = xcd_tile((int)blockIdx.x, n_tiles);
    // ---- row maps and slot records from the tile index alone (uniform strides; lanes past a stride repeat its last record)
    int2 s[NPT];
    uint32_t pk[EPT], pk3[EPT];
    const int2 *src = pd.node_src + (size_t)slot * pd.node_stride;
    const uint32_t *ep = pd.elem_pack + (size_t)slot * pd.elem_stride;
    const uint32_t *ep3 = pd.elem_pack_hi + (size_t)slot * pd.elem_stride;
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

    // ---- gather into LDS (rows widened on load), clear the accumulators
    auto gather = [&](int l, int2 r) {
        const V2 *px = r.x >= 0 ? x_free + r.x : x_fixed + ~r.x;
        const V2 *pu = r.y >= 0 ? u_free + r.y : u_fixed + ~r.y;
        const V2 vx = *px, vu = *pu;
        if (l < d.n_node) {
            nd_xy[l] = make_double2((double)vx.x, (double)vx.y);
            nd_uv[l] = make_double2((double)vu.x, (double)vu.y);
        }
        if (l < n_owned) { acc0[l] = 0.0; acc1[l] = 0.0; acc2[l] = 0.0; acc3[l] = 0.0; }
    };
#pragma unroll
    for (int j = 0; j < NPT; ++j) gather(tid + j * BLOCK, s[j]);
    __syncthreads();

    // ---- cells (home + halo): registers + LDS only
    double e_loc = 0.0, j_min = (double)INFINITY, n_inv = 0.0;
    auto add_row = [&](int l, const double2 gx, const double2 gu) {
        if (l < n_owned) {
            unsafeAtomicAdd(&acc0[l], gx.x); unsafeAtomicAdd(&acc1[l], gx.y);
            unsafeAtomicAdd(&acc2[l], gu.x); unsafeAtomicAdd(&acc3[l], gu.y);
        }
    };
    auto element = [&](uint32_t p, uint32_t p3) {
        if (p & kSkipBit) return;
        const int l0 = (int)(p & kLocalMask), l1 = (int)((p >> kLocalBits) & kLocalMask),
                  l2 = (int)((p >> (2 * kLocalBits)) & kLocalMask), l3 = (int)(p3 & kLocalMask);
        const double2 Xn[4] = {nd_xy[l0], nd_xy[l1], nd_xy[l2], nd_xy[l3]};
        const double2 Un[4] = {nd_uv[l0], nd_uv[l1], nd_uv[l2], nd_uv[l3]};
        double2 gx[4], gu[4];
        double jm1;
        bool inv;
        const double e = quad4_neo_hookean_element<HASB>(Xn, Un, k, gx, gu, jm1, inv);
        if (p & kHomeBit) {
            e_loc += e;
            j_min = fmin(j_min, 1.0 + jm1);
            n_inv += inv ? 1.0 : 0.0;
        }
        add_row(l0, gx[0], gu[0]);
        add_row(l1, gx[1], gu[1]);
        add_row(l2, gx[2], gu[2]);
        add_row(l3, gx[3], gu[3]);
    };
#pragma unroll
    for (int j = 0; j < EPT; ++j) element(pk[j], pk3[j]);
    for (int i = tid + EPT * BLOCK; i < d.n_elem; i += BLOCK) element(ep[i], ep3[i]);
    const int n_edge = skip_edges ? 0 : d.n_edge;
    for (int i = tid; i < n_edge; i += BLOCK) {          // boundary tiles only
        const uint32_t p = pd.edge_pack[d.edge_off + i];
        const int l0 = (int)(p & kLocalMask), l1 = (int)((p >> kLocalBits) & kLocalMask);
        const double4 tt = T_edge ? T_edge[pd.edge_gid[d.edge_off + i]] : Tconst;
        double2 gx[2], gu[2];
        const double wk = edge2_element<true>(nd_xy[l0], nd_xy[l1], nd_uv[l0], nd_uv[l1], tt, gx, gu);
        if (p & kHomeBit) e_loc -= wk;
        add_row(l0, gx[0], gu[0]);
        add_row(l1, gx[1], gu[1]);
    }
    {
        const double we = wave_sum(e_loc), wj = wave_min(j_min), wc = wave_sum(n_inv);
        if ((tid & 63) == 0) {
            red[tid >> 6] = we;
            red[BLOCK / 64 + (tid >> 6)] = wj;
            red[2 * (BLOCK / 64) + (tid >> 6)] = wc;
        }
    }
    __syncthreads();

    // ---- every owned gradient row is written exactly once (one rounding for float rows)
    auto store = [&](int l, int2 r) {
        if (l < n_owned) {
            if (gx_free && r.x >= 0) {
                V2 v;
                v.x = acc0[l]; v.y = acc1[l];
                gx_free[r.x] = v;
            }
            if (gu_free && r.y >= 0) {
                V2 v;
                v.x = acc2[l]; v.y = acc3[l];
                gu_free[r.y] = v;
            }
        }
    };
#pragma unroll
    for (int j = 0; j < NPT; ++j) store(tid + j * BLOCK, s[j]);
    if (tid == 0) {                                     // wave order: the tile energy is bit-reproducible
        double te = 0.0, tj = (double)INFINITY, tc = 0.0;
#pragma unroll
        for (int w = 0; w < BLOCK / 64; ++w) {
            te += red[w];
            tj = fmin(tj, red[BLOCK / 64 + w]);
            tc += red[2 * (BLOCK / 64) + w];
        }
        work[slot] = te;
        work[n_tiles + slot] = tj;
        work[2 * n_tiles + slot] = tc;
    }
}

// loss = sum of the tile energies in hyper_finish_thread's order (256 adders, shuffle tree, wave sums in wave order);
// info = {min J, inverted count} (may be NULL).  tri3_hyper.hip's finishing launch, restated over the shared per-thread part.
__global__ __launch_bounds__(kQHyperFinish) void quad4_hyper_finish_kernel(const double *__restrict__ work, int n,
                                                                            double *__restrict__ loss_out,
                                                                            double *__restrict__ info_out) {
    __shared__ double red_e[kQHyperFinish / 64], red_j[kQHyperFinish / 64], red_c[kQHyperFinish / 64];
    double e, mj, cnt;
    hyper_finish_thread(work, n, (int)threadIdx.x, kQHyperFinish, e, mj, cnt);
    mj = wave_min(mj);
    if ((threadIdx.x & 63) == 0) red_j[threadIdx.x >> 6] = mj;
    const double tot = block_sum(e, red_e), tc = block_sum(cnt, red_c);
    if (threadIdx.x == 0) {
        loss_out[0] = tot;
        if (info_out) {
            double tj = red_j[0];
            for (int w = 1; w < kQHyperFinish / 64; ++w) tj = fmin(tj, red_j[w]);
            info_out[0] = tj;
            info_out[1] = tc;
        }
    }
}

template <typename V2, bool HASB>
static void launch_quad4_hyper(const hfem_plan *plan, const void *x_free, const void *x_fixed, const void *u_free,
                               const void *u_fixed, const Quad4HyperConsts &k, const double4 *T_edge, double4 tc, double *work,
                               void *gx, void *gu, int skip_edges, size_t lds, hipStream_t s) {
    const HostPlan &h = plan->host;
    const int nt = (int)h.tiles.size();
    hipLaunchKernelGGL((quad4_hyper_kernel<kQHyperBlock, kQHyperNpt, kQHyperEpt, V2, HASB>), dim3(nt), dim3(kQHyperBlock), lds, s,
                       plan_dev(plan), (const V2 *)x_free, (const V2 *)x_fixed, (const V2 *)u_free, (const V2 *)u_fixed, k,
                       T_edge, tc, work, nt, (V2 *)gx, (V2 *)gu, h.max_nodes, h.max_owned, skip_edges);
}

}  // namespace hfem

using namespace hfem;

extern "C" int hfem_quad4_hyper_energy_plan(hfem_plan *plan, int32_t dtype, const void *x_free, const void *x_fixed,
                                            const void *u_free, const void *u_fixed, const double lame[2], const double Bq[8],
                                            const double *T_edge, const double Tconst[4], double *loss_out, double *info_out,
                                            double *work, void *gx_free, void *gu_free, int32_t flags, void *stream) {
    HFEM_ARG_CHECK(plan && lame && loss_out && work, "null pointer");
    HFEM_ARG_CHECK(dtype == 0 || dtype == 1, "dtype must be 0 (fp64 rows) or 1 (fp32 rows)");
    HFEM_ARG_CHECK(!(flags & ~(HFEM_FLAG_NO_GX | HFEM_FLAG_NO_GU | HFEM_FLAG_NO_EDGES)),
                   "flags: HFEM_FLAG_NO_GX, HFEM_FLAG_NO_GU and HFEM_FLAG_NO_EDGES only");
    HFEM_ARG_CHECK(plan->device >= 0, "host-only plan (created with device < 0) cannot launch");
    HFEM_ARG_CHECK(plan->host.npe == 4, "this plan was built for TRI3: use hfem_tri3_hyper_energy_plan");
    HFEM_ARG_CHECK(x_free && u_free, "x_free / u_free must be given");
    HFEM_ARG_CHECK(gx_free || (flags & HFEM_FLAG_NO_GX), "gx_free is NULL without HFEM_FLAG_NO_GX");
    HFEM_ARG_CHECK(gu_free || (flags & HFEM_FLAG_NO_GU), "gu_free is NULL without HFEM_FLAG_NO_GU");
    const HostPlan &h = plan->host;
    const bool skip_edges = (flags & HFEM_FLAG_NO_EDGES) != 0;
    HFEM_ARG_CHECK(h.ned == 0 || skip_edges || T_edge || Tconst, "plan has Neumann edges: need a traction table");
    HFEM_ARG_CHECK(h.max_nodes <= kQHyperNpt * kQHyperBlock, "tile has more local nodes than the kernel's row-map registers hold");
    const size_t lds = (size_t)h.max_nodes * 32 + (size_t)h.max_owned * 32 + 3 * (kQHyperBlock / 64) * sizeof(double);
    HFEM_ARG_CHECK(lds <= 64 * 1024, "tile needs more than 64 KiB of LDS");
    const int nt = (int)h.tiles.size();
    if (int rc = use_device(plan->device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    Quad4HyperConsts k;
    k.lambda = lame[0]; k.mu = lame[1];
    bool hasb = false;
    for (int q = 0; q < 4; ++q) {
        k.b[q] = Bq ? make_double2(Bq[2 * q], Bq[2 * q + 1]) : make_double2(0.0, 0.0);
        hasb = hasb || k.b[q].x != 0.0 || k.b[q].y != 0.0;
    }
    const double4 tc = Tconst ? make_double4(Tconst[0], Tconst[1], Tconst[2], Tconst[3]) : make_double4(0, 0, 0, 0);
    if (nt > 0) {
        void *gx = (flags & HFEM_FLAG_NO_GX) ? nullptr : gx_free, *gu = (flags & HFEM_FLAG_NO_GU) ? nullptr : gu_free;
#define HFEM_QHYPER(V, B) \
    launch_quad4_hyper<V, B>(plan, x_free, x_fixed, u_free, u_fixed, k, (const double4 *)T_edge, tc, work, gx, gu, skip_edges, lds, s)
        if (dtype == 1) { if (hasb) HFEM_QHYPER(float2, true); else HFEM_QHYPER(float2, false); }
        else { if (hasb) HFEM_QHYPER(double2, true); else HFEM_QHYPER(double2, false); }
#undef HFEM_QHYPER
        if (int rc = launch_status("hfem_quad4_hyper_energy_plan")) return rc;
    }
    hipLaunchKernelGGL(quad4_hyper_finish_kernel, dim3(1), dim3(kQHyperFinish), 0, s, work, nt, loss_out, info_out);
    return launch_status("hfem_quad4_hyper_energy_plan(finish)");
}
