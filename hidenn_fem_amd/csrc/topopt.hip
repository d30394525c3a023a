// Topology optimisation on the element-scaled stiffness K(w) = sum_e w_e K_e, gfx950 (MI355X) (hidenn_fem_amd/solve.py
// set_element_scale): the design handle and its kernels.  The operator itself is no kernel of this file: q = K(w) p
// and the diagonal blocks of K(w) are the Scaled instances of the element kernels of tri3_cg.hip / quad4_cg.hip (bound by
// hfem_cg_setup_scaled, cg.hip), and the AMG fine level of K(w) is the Scaled instance of amg_assemble_kernel (tri3_amg.hip).
// Of hfem_cg_dev.h this file uses the reduction pieces (put_partial, last_block, ordered_sum, block_sum) and the element
// closed forms (tri3_element, quad4_element_u) only.
//
// The design handle hfem_topt holds what maps a density design onto those weights:
//   topt_weights_kernel   w_e = e_min + rho_e^penal (1 - e_min): once by element id into w_elem, once per slot of the plan into
//                         w_slot through the plan's elem_gid / elem_gid_b (padded or absent entries 0)
//   topt_filter_kernel    the linear density filter, one thread per element gathering its CSR row (built on the host with a
//                         uniform grid of cell size radius; H_ej = max(0, radius - |x_e - x_j|), columns sorted): no atomics,
//                         bit-reproducible.  forward out_e = sum_j H_ej v_j in_j / s_e, s_e = sum_j H_ej v_j; transpose
//                         out_j = v_j sum_e H_je in_e / s_e (H is symmetric: the same gather with other scalings).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "hfem_cg_dev.h"
#include "hfem_device.h"
#include "hfem_plan_dev.h"

namespace hfem {
namespace {

// ---------------------------------------------------------------- the design handle's kernels
constexpr int kToptBlock = 256;

// SIMP: w = e_min + rho^penal (1 - e_min); penal = 1 keeps rho itself (an element scale is passed through unchanged)
__device__ __forceinline__ double simp_weight(double rho, double penal, double e_min) {
    const double rp = penal == 1.0 ? rho : pow(rho, penal);
    return __builtin_fma(rp, 1.0 - e_min, e_min);
}

// Thread i < ne: w_elem[i]; thread i < n_slots: the record of slot i (PAIRED: double2 {w_A, w_B}), 0 where the plan holds no
// element.  The slot value is recomputed from rho, not read back: the same function of the same input, the same bits.
template <bool PAIRED>
__global__ __launch_bounds__(kToptBlock) void topt_weights_kernel(int64_t ne, int64_t n_slots, const int32_t *__restrict__ gid,
                                                                  const int32_t *__restrict__ gid_b,
                                                                  const double *__restrict__ rho, double penal, double e_min,
                                                                  double *__restrict__ w_elem, double *__restrict__ w_slot) {
    const int64_t i = (int64_t)blockIdx.x * kToptBlock + threadIdx.x;
    if (i < ne && w_elem) w_elem[i] = simp_weight(rho[i], penal, e_min);
    if (i < n_slots && w_slot) {
        const int32_t ga = gid[i];
        const double wa = ga >= 0 ? simp_weight(rho[ga], penal, e_min) : 0.0;
        if constexpr (PAIRED) {
            const int32_t gb = gid_b[i];
            const double wb = gb >= 0 ? simp_weight(rho[gb], penal, e_min) : 0.0;
            reinterpret_cast<double2 *>(w_slot)[i] = make_double2(wa, wb);
        } else {
            w_slot[i] = wa;
        }
    }
}

// One thread per element gathers its filter row.  TRANSPOSE = false: out_e = sum_j H_ej v_j in_j / s_e;
// TRANSPOSE = true: out_e = v_e sum_j H_ej in_j / s_j.
template <bool TRANSPOSE>
__global__ __launch_bounds__(kToptBlock) void topt_filter_kernel(int64_t ne, const int32_t *__restrict__ ptr,
                                                                 const int32_t *__restrict__ col, const double *__restrict__ H,
                                                                 const double *__restrict__ vol, const double *__restrict__ ssum,
                                                                 const double *__restrict__ in, double *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * kToptBlock + threadIdx.x;
    if (e >= ne) return;
    double acc = 0.0;
    for (int32_t t = ptr[e]; t < ptr[e + 1]; ++t) {
        const int32_t j = col[t];
        acc += TRANSPOSE ? H[t] * (in[j] / ssum[j]) : H[t] * (vol[j] * in[j]);
    }
    out[e] = TRANSPOSE ? vol[e] * acc : acc / ssum[e];
}

// ---------------------------------------------------------------- element energies and the compliance sensitivity
// The apply's gather and slot loop with no accumulation: at each element's HOME slot (every element has exactly one)
//   ce[e] = u_e^T K_e u_e (unscaled: twice the element's strain energy),  dc[e] = -penal rho_e^(penal-1) (1 - e_min) ce[e]
// by global element id (the handle's copy of the plan's elem_gid / elem_gid_b).  Fixed u rows read as 0.  Tile shapes as the
// diag kernels (slot rows: the diag kernels' 2 | 6 | 4, a run-time loop).  LDS: xy[cap_nodes] double2 | u[cap_nodes] double2.
__device__ __forceinline__ void put_energy(int32_t g, double e, const double *__restrict__ rho, double penal, double e_min,
                                           double *__restrict__ ce, double *__restrict__ dc) {
    const double c = 2.0 * e;
    ce[g] = c;
    if (dc) {
        const double r = rho[g];
        const double d = penal == 1.0 ? 1.0 : (penal == 2.0 ? r : pow(r, penal - 1.0));
        dc[g] = -(penal * d * (1.0 - e_min)) * c;
    }
}

template <int BLOCK, int NPT, bool PHYS>
__global__ __launch_bounds__(BLOCK) void tri3_topt_energy_kernel(PlanDev pd, const double2 *__restrict__ x_free,
                                                                 const double2 *__restrict__ x_fixed,
                                                                 const double2 *__restrict__ u_free, Tri3Consts k,
                                                                 const int32_t *__restrict__ gid, const int32_t *__restrict__ gid_b,
                                                                 const double *__restrict__ rho, double penal, double e_min,
                                                                 double *__restrict__ ce, double *__restrict__ dc, int cap_nodes,
                                                                 int col_stride, int rows) {
    extern __shared__ double2 lds[];
    double2 *nd_xy = lds, *nd_u = lds + cap_nodes;
    const int tid = threadIdx.x;
    const int slot = (int)blockIdx.x;
    const int2 *src = pd.node_src + (size_t)slot * pd.node_stride;
    const TileDesc d = pd.tiles[slot];
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int l = tid + j * BLOCK;
        if (l < d.n_node) {
            const int2 s = src[l];
            nd_xy[l] = s.x >= 0 ? x_free[s.x] : x_fixed[~s.x];
            nd_u[l] = s.y >= 0 ? u_free[s.y] : make_double2(0.0, 0.0);
        }
    }
    __syncthreads();
    for (int j = 0; j < rows; ++j) {
        if (!(tid < col_stride && tid + j * col_stride < d.n_elem)) continue;
        const size_t i = (size_t)slot * pd.elem_stride + tid + j * col_stride;
        const uint32_t a = pd.elem_pack[i], b = pd.elem_pack_hi[i];
        if (a & kSkipBit) continue;
        const int ln = (int)(a & kLocalMask), lb = (int)((a >> kLocalBits) & kLocalMask),
                  lc = (int)((a >> (2 * kLocalBits)) & kLocalMask);
        double2 gx[3], gu[3];
        if (a & kHomeBit)
            put_energy(gid[i], tri3_element<true, false, PHYS>(nd_xy[ln], nd_xy[lb], nd_xy[lc], nd_u[ln], nd_u[lb], nd_u[lc], k, gx, gu),
                       rho, penal, e_min, ce, dc);
        if ((b & kHasBBit) && (b & kHomeBBit)) {
            const int ld = (int)(b & kLocalMask);
            put_energy(gid_b[i], tri3_element<true, false, PHYS>(nd_xy[ln], nd_xy[lc], nd_xy[ld], nd_u[ln], nd_u[lc], nd_u[ld], k, gx, gu),
                       rho, penal, e_min, ce, dc);
        }
    }
}

template <int BLOCK, int NPT, bool PHYS>
__global__ __launch_bounds__(BLOCK) void quad4_topt_energy_kernel(PlanDev pd, const double2 *__restrict__ x_free,
                                                                  const double2 *__restrict__ x_fixed,
                                                                  const double2 *__restrict__ u_free, Tri3Consts k,
                                                                  const int32_t *__restrict__ gid, const double *__restrict__ rho,
                                                                  double penal, double e_min, double *__restrict__ ce,
                                                                  double *__restrict__ dc, int cap_nodes, int rows) {
    extern __shared__ double2 lds[];
    double2 *nd_xy = lds, *nd_u = lds + cap_nodes;
    const int tid = threadIdx.x;
    const int slot = (int)blockIdx.x;
    const int2 *src = pd.node_src + (size_t)slot * pd.node_stride;
    const TileDesc d = pd.tiles[slot];
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int l = tid + j * BLOCK;
        if (l < d.n_node) {
            const int2 s = src[l];
            nd_xy[l] = *(s.x >= 0 ? x_free + s.x : x_fixed + ~s.x);
            nd_u[l] = s.y >= 0 ? u_free[s.y] : make_double2(0.0, 0.0);
        }
    }
    __syncthreads();
    for (int j = 0; j < rows; ++j) {
        if (tid + j * BLOCK >= d.n_elem) continue;
        const size_t i = (size_t)slot * pd.elem_stride + tid + j * BLOCK;
        const uint32_t p = pd.elem_pack[i];
        if ((p & kSkipBit) || !(p & kHomeBit)) continue;
        const int l[4] = {(int)(p & kLocalMask), (int)((p >> kLocalBits) & kLocalMask),
                          (int)((p >> (2 * kLocalBits)) & kLocalMask), (int)(pd.elem_pack_hi[i] & kLocalMask)};
        const double2 Xn[4] = {nd_xy[l[0]], nd_xy[l[1]], nd_xy[l[2]], nd_xy[l[3]]};
        const double2 Un[4] = {nd_u[l[0]], nd_u[l[1]], nd_u[l[2]], nd_u[l[3]]};
        double2 gu[4];
        put_energy(gid[i], quad4_element_u<PHYS>(Xn, Un, k, gu), rho, penal, e_min, ce, dc);
    }
}

// ---------------------------------------------------------------- the optimality-criteria update
// rho_new,e(lambda) = clamp(rho_e sqrt(r_e / lambda), max(0, rho_e - move), min(1, rho_e + move)),  r_e = max(0, -dc_e / dv_e)
// lambda by bisection so that V(lambda) = sum_e v_e (F rho_new(lambda))_e <= vol_target.  Everything the search decides lives
// in the handle's status record (device), so the whole update is a fixed list of launches:
//   init    R = max_e r_e (a maximum: order-free); bracket [0, R] (R = 0: [0, 1]), phase "expand".  At lambda = R every
//           rho_e sqrt(r_e / lambda) <= rho_e, so the design does not grow anywhere: feasible whenever the current design is.
//   step    one launch evaluates V at one lambda: in phase "expand" at lambda_hi -- feasible: phase "bisect"; not:
//           lambda_lo = lambda_hi, lambda_hi x= 4 -- and in phase "bisect" at the midpoint m = (lambda_lo + lambda_hi) / 2 --
//           V(m) <= vol_target: lambda_hi = m, else lambda_lo = m; a midpoint that equals an end (the bracket is one ulp
//           wide) returns at once.  The filter gather evaluates each neighbour's update on the fly; the block partials of V
//           are summed in block order by the ticket workgroup, whose thread 0 decides.
//   final   rho_new = the update at lambda_hi (the feasible end), rho_f_new = F rho_new; publishes the record.
enum { oLo = 0, oHi, oVolHi, oSteps, oFeasible, oPhase, oVolTarget, oR, oVolLo, oStatusN = 16 };

__device__ __forceinline__ double oc_value(double rho, double dc, double dv, double lambda, double move) {
    const double r = fmax(0.0, -dc / dv);
    const double b = rho * sqrt(r / lambda);
    return fmin(fmin(1.0, rho + move), fmax(fmax(0.0, rho - move), b));
}

__global__ __launch_bounds__(kToptBlock) void topt_oc_init_kernel(int64_t ne, const double *__restrict__ dc,
                                                                  const double *__restrict__ dv, double vol_target,
                                                                  double *__restrict__ part, unsigned *ticket, double *st) {
    __shared__ double red[kToptBlock / 64 + 1];
    const int tid = threadIdx.x, nb = (int)gridDim.x;
    double m = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * kToptBlock + tid; e < ne; e += (int64_t)nb * kToptBlock) m = fmax(m, fmax(0.0, -dc[e] / dv[e]));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_down(m, off, 64));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kToptBlock / 64; ++w) m = fmax(m, red[w]);
        put_partial(part + blockIdx.x, m);
    }
    if (!last_block(ticket, (unsigned)nb, reinterpret_cast<int *>(red + kToptBlock / 64))) return;
    if (tid != 0) return;
    double R = 0.0;
    for (int i = 0; i < nb; ++i) R = fmax(R, get_partial(part + i));
    for (int i = 0; i < oStatusN; ++i) st[i] = 0.0;
    st[oR] = R;
    st[oHi] = R > 0.0 && isfinite(R) ? R : 1.0;
    st[oVolTarget] = vol_target;
    st[oVolHi] = __builtin_nan("");                          // neither end has been evaluated yet
    st[oVolLo] = __builtin_nan("");
}

// the filtered update of element e at lambda (IDENT: no filter)
template <bool IDENT>
__device__ __forceinline__ double oc_filtered(int64_t e, const int32_t *__restrict__ ptr, const int32_t *__restrict__ col,
                                              const double *__restrict__ H, const double *__restrict__ vol,
                                              const double *__restrict__ ssum, const double *__restrict__ rho,
                                              const double *__restrict__ dc, const double *__restrict__ dv, double lambda,
                                              double move) {
    if constexpr (IDENT) return oc_value(rho[e], dc[e], dv[e], lambda, move);
    double acc = 0.0;
    for (int32_t t = ptr[e]; t < ptr[e + 1]; ++t) {
        const int32_t j = col[t];
        acc += H[t] * (vol[j] * oc_value(rho[j], dc[j], dv[j], lambda, move));
    }
    return acc / ssum[e];
}

template <bool IDENT>
__global__ __launch_bounds__(kToptBlock) void topt_oc_step_kernel(int64_t ne, const int32_t *__restrict__ ptr,
                                                                  const int32_t *__restrict__ col, const double *__restrict__ H,
                                                                  const double *__restrict__ vol, const double *__restrict__ ssum,
                                                                  const double *__restrict__ rho, const double *__restrict__ dc,
                                                                  const double *__restrict__ dv, double move,
                                                                  double *__restrict__ part, unsigned *ticket, double *st) {
    __shared__ double red[kToptBlock / 64 + 1];
    const int tid = threadIdx.x, nb = (int)gridDim.x;
    const double lo = st[oLo], hi = st[oHi];
    const bool expand = st[oPhase] == 0.0;
    const double lambda = expand ? hi : 0.5 * (lo + hi);
    if (!expand && !(lambda > lo && lambda < hi)) return;     // uniform: the bracket cannot be halved any more
    const int64_t e = (int64_t)blockIdx.x * kToptBlock + tid;
    double v = 0.0;
    if (e < ne) v = vol[e] * oc_filtered<IDENT>(e, ptr, col, H, vol, ssum, rho, dc, dv, lambda, move);
    const double bs = block_sum(v, red);
    if (tid == 0) put_partial(part + blockIdx.x, bs);
    if (!last_block(ticket, (unsigned)nb, reinterpret_cast<int *>(red + kToptBlock / 64))) return;
    const double V = ordered_sum<kToptBlock>(part, nb, red);
    if (tid != 0) return;
    const bool ok = V <= st[oVolTarget];
    st[oSteps] += 1.0;
    // oVolHi / oVolLo are V at the bracket's ends as they stand: an end that was never evaluated holds NaN
    if (expand) {
        st[oVolHi] = V;
        if (ok) { st[oFeasible] = 1.0; st[oPhase] = 1.0; }
        else if (isfinite(4.0 * hi)) { st[oLo] = hi; st[oVolLo] = V; st[oHi] = 4.0 * hi; st[oVolHi] = __builtin_nan(""); }
    } else if (ok) {
        st[oHi] = lambda; st[oVolHi] = V;
    } else {
        st[oLo] = lambda; st[oVolLo] = V;
    }
}

template <bool IDENT>
__global__ __launch_bounds__(kToptBlock) void topt_oc_final_kernel(int64_t ne, const int32_t *__restrict__ ptr,
                                                                   const int32_t *__restrict__ col, const double *__restrict__ H,
                                                                   const double *__restrict__ vol, const double *__restrict__ ssum,
                                                                   const double *__restrict__ rho, const double *__restrict__ dc,
                                                                   const double *__restrict__ dv, double move, const double *st,
                                                                   double *host, double *__restrict__ rho_new,
                                                                   double *__restrict__ rho_f_new) {
    const int64_t e = (int64_t)blockIdx.x * kToptBlock + threadIdx.x;
    const double lambda = st[oHi];
    if (e == 0 && host)
        for (int i = 0; i < oStatusN; ++i) host[i] = st[i];
    if (e >= ne) return;
    rho_new[e] = oc_value(rho[e], dc[e], dv[e], lambda, move);
    rho_f_new[e] = oc_filtered<IDENT>(e, ptr, col, H, vol, ssum, rho, dc, dv, lambda, move);
}

}  // namespace
}  // namespace hfem

// ---------------------------------------------------------------- the design handle
struct hfem_topt {
    int device = -1;
    int64_t ne = 0, n_slots = 0, nnz = 0;
    bool paired = false, identity = true;
    int32_t *gid = nullptr, *gid_b = nullptr;              // the plan's elem_gid / elem_gid_b, n_slots each
    int32_t *f_ptr = nullptr, *f_col = nullptr;            // the filter's CSR (identity: none)
    double *f_h = nullptr, *vol = nullptr, *ssum = nullptr;
    // the optimality-criteria search: block partials, status record, ticket (device); pinned mirror of the record
    int oc_blocks = 1;
    double *oc_part = nullptr, *oc_st = nullptr, *host = nullptr;
    unsigned *oc_ticket = nullptr;
    const hfem_plan *plan = nullptr;
};

namespace {
void topt_release(hfem_topt *t) {
    for (void *p : {(void *)t->gid, (void *)t->gid_b, (void *)t->f_ptr, (void *)t->f_col, (void *)t->f_h, (void *)t->vol,
                    (void *)t->ssum, (void *)t->oc_part})
        if (p) (void)hipFree(p);
    if (t->host) (void)hipHostFree(t->host);
}

template <typename T>
int topt_upload(T **dst, const T *src, size_t n) {
    if (hipMalloc((void **)dst, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess ||
        (n && hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)) {
        hfem::set_error("hfem_topt_create: device allocation or upload failed");
        return 1;
    }
    return 0;
}

dim3 topt_grid(int64_t n) { return dim3((unsigned)std::max<int64_t>(1, (n + hfem::kToptBlock - 1) / hfem::kToptBlock)); }

// The filter's CSR: row e holds every j with |x_e - x_j| < radius (H_ej > 0), columns ascending.  Uniform grid of cells no
// smaller than radius, so a row's candidates lie in the 3 x 3 cells around its own.  Returns the entry count; fills the
// arrays only when `fill` (the count is checked against int32 first).
int64_t filter_rows(const double *c, int64_t ne, double radius, bool fill, std::vector<int32_t> &ptr, std::vector<int32_t> &col,
                    std::vector<double> &H) {
    double lo[2] = {c[0], c[1]}, hi[2] = {c[0], c[1]};
    for (int64_t e = 0; e < ne; ++e)
        for (int d = 0; d < 2; ++d) { lo[d] = std::min(lo[d], c[2 * e + d]); hi[d] = std::max(hi[d], c[2 * e + d]); }
    double cell = radius;
    while ((std::floor((hi[0] - lo[0]) / cell) + 1.0) * (std::floor((hi[1] - lo[1]) / cell) + 1.0) > 4.0 * (double)ne + 64.0) cell *= 2.0;
    const int64_t nx = (int64_t)std::floor((hi[0] - lo[0]) / cell) + 1, ny = (int64_t)std::floor((hi[1] - lo[1]) / cell) + 1;
    auto cell_of = [&](int64_t e, int d) {
        const int64_t n = d ? ny : nx;
        return std::min<int64_t>(n - 1, std::max<int64_t>(0, (int64_t)std::floor((c[2 * e + d] - lo[d]) / cell)));
    };
    std::vector<int64_t> start((size_t)(nx * ny) + 1, 0);
    for (int64_t e = 0; e < ne; ++e) ++start[(size_t)(cell_of(e, 1) * nx + cell_of(e, 0)) + 1];
    for (size_t i = 1; i < start.size(); ++i) start[i] += start[i - 1];
    std::vector<int32_t> member((size_t)ne);
    {
        std::vector<int64_t> at(start.begin(), start.end() - 1);
        for (int64_t e = 0; e < ne; ++e) member[(size_t)at[(size_t)(cell_of(e, 1) * nx + cell_of(e, 0))]++] = (int32_t)e;
    }
    int64_t total = 0;
    std::vector<std::pair<int32_t, double>> row;
    if (fill) ptr.assign((size_t)ne + 1, 0);
    for (int64_t e = 0; e < ne; ++e) {
        row.clear();
        const int64_t cx = cell_of(e, 0), cy = cell_of(e, 1);
        for (int64_t y = std::max<int64_t>(0, cy - 1); y <= std::min(ny - 1, cy + 1); ++y)
            for (int64_t x = std::max<int64_t>(0, cx - 1); x <= std::min(nx - 1, cx + 1); ++x)
                for (int64_t m = start[(size_t)(y * nx + x)]; m < start[(size_t)(y * nx + x) + 1]; ++m) {
                    const int32_t j = member[(size_t)m];
                    const double h = radius - std::hypot(c[2 * e] - c[2 * (int64_t)j], c[2 * e + 1] - c[2 * (int64_t)j + 1]);
                    if (h > 0.0) row.emplace_back(j, h);
                }
        total += (int64_t)row.size();
        if (fill) {
            std::sort(row.begin(), row.end());
            for (const auto &r : row) { col.push_back(r.first); H.push_back(r.second); }
            ptr[(size_t)e + 1] = (int32_t)col.size();
        }
    }
    return total;
}
}  // namespace

extern "C" int hfem_topt_create(hfem_plan *plan, const double *centroids, const double *volumes, int64_t ne, double radius,
                                hfem_topt **out) {
    HFEM_ARG_CHECK(plan && out, "null pointer");
    *out = nullptr;
    HFEM_ARG_CHECK(plan->device >= 0, "host-only plan (created with device < 0) cannot launch");
    HFEM_ARG_CHECK(ne > 0 && ne < ((int64_t)1 << 31), "ne must be in [1, 2^31)");
    HFEM_ARG_CHECK(!std::isnan(radius) && radius < std::numeric_limits<double>::infinity(), "radius must be finite (<= 0: the identity filter)");
    const bool identity = !(radius > 0.0);
    HFEM_ARG_CHECK(identity || (centroids && volumes), "a filter radius > 0 needs centroids[ne][2] and volumes[ne]");
    if (volumes)
        for (int64_t e = 0; e < ne; ++e) HFEM_ARG_CHECK(std::isfinite(volumes[e]) && volumes[e] > 0.0, "volumes must be finite and > 0");
    const hfem::HostPlan &h = plan->host;
    const bool quad = h.npe == 4;
    HFEM_ARG_CHECK(quad || h.paired, "the design handle needs a paired-slot TRI3 plan or a QUAD4 plan (hfem_cg_create's)");
    const size_t n_slots = h.tiles.size() * (size_t)h.elem_stride;
    HFEM_ARG_CHECK(h.elem_gid.size() >= n_slots && (quad || h.elem_gid_b.size() >= n_slots), "the plan holds no element ids per slot");
    int64_t top = -1;
    for (size_t i = 0; i < n_slots; ++i) top = std::max<int64_t>(top, std::max(h.elem_gid[i], quad ? -1 : h.elem_gid_b[i]));
    HFEM_ARG_CHECK(top < ne, "ne is smaller than the plan's element count");
    std::vector<int32_t> ptr, col;
    std::vector<double> H, ssum;
    if (!identity) {
        for (int64_t e = 0; e < ne; ++e)
            HFEM_ARG_CHECK(std::isfinite(centroids[2 * e]) && std::isfinite(centroids[2 * e + 1]), "centroids must be finite");
        const int64_t total = filter_rows(centroids, ne, radius, false, ptr, col, H);
        if (total > (int64_t)std::numeric_limits<int32_t>::max()) {
            hfem::set_error("hfem_topt_create: the filter has " + std::to_string(total) + " entries, more than 2^31 - 1: use a smaller radius");
            return -1;
        }
        col.reserve((size_t)total); H.reserve((size_t)total);
        filter_rows(centroids, ne, radius, true, ptr, col, H);
        ssum.assign((size_t)ne, 0.0);
        for (int64_t e = 0; e < ne; ++e)
            for (int32_t t = ptr[(size_t)e]; t < ptr[(size_t)e + 1]; ++t) ssum[(size_t)e] += H[(size_t)t] * volumes[col[(size_t)t]];
    }
    if (int rc = hfem::use_device(plan->device)) return rc;
    std::unique_ptr<hfem_topt> t(new hfem_topt);
    t->device = plan->device; t->ne = ne; t->n_slots = (int64_t)n_slots; t->paired = !quad; t->identity = identity;
    t->nnz = (int64_t)col.size(); t->plan = plan;
    t->oc_blocks = (int)((ne + hfem::kToptBlock - 1) / hfem::kToptBlock);
    bool bad = topt_upload(&t->gid, h.elem_gid.data(), n_slots) || (!quad && topt_upload(&t->gid_b, h.elem_gid_b.data(), n_slots));
    if (!bad && volumes) bad = topt_upload(&t->vol, volumes, (size_t)ne);
    if (!bad && !identity)
        bad = topt_upload(&t->f_ptr, ptr.data(), ptr.size()) || topt_upload(&t->f_col, col.data(), col.size()) ||
              topt_upload(&t->f_h, H.data(), H.size()) || topt_upload(&t->ssum, ssum.data(), ssum.size());
    if (!bad) {                                               // partials | status record | ticket, zeroed (the ticket must be)
        const size_t bytes = ((size_t)t->oc_blocks + hfem::oStatusN + 8) * sizeof(double);
        bad = hipMalloc((void **)&t->oc_part, bytes) != hipSuccess || hipMemset(t->oc_part, 0, bytes) != hipSuccess ||
              hipHostMalloc((void **)&t->host, hfem::oStatusN * sizeof(double)) != hipSuccess;
        if (bad) hfem::set_error("hfem_topt_create: device allocation failed");
        else {
            t->oc_st = t->oc_part + t->oc_blocks;
            t->oc_ticket = reinterpret_cast<unsigned *>(t->oc_st + hfem::oStatusN);
            for (int i = 0; i < hfem::oStatusN; ++i) t->host[i] = 0.0;
        }
    }
    if (bad) {
        topt_release(t.get());
        return 1;
    }
    *out = t.release();
    return 0;
}

extern "C" int hfem_topt_destroy(hfem_topt *t) {
    if (!t) return 0;
    if (t->device >= 0) (void)hipSetDevice(t->device);
    topt_release(t);
    delete t;
    return 0;
}

extern "C" int64_t hfem_topt_slots(const hfem_topt *t) {
    if (!t) {
        hfem::set_error("hfem_topt_slots: null pointer");
        return -1;
    }
    return t->n_slots * (t->paired ? 2 : 1);
}

extern "C" int hfem_topt_weights(hfem_topt *t, const double *rho_f, double penal, double e_min, double *w_elem, double *w_slot,
                                 void *stream) {
    HFEM_ARG_CHECK(std::isfinite(penal) && penal >= 1.0, "penal must be finite and >= 1");
    HFEM_ARG_CHECK(std::isfinite(e_min) && e_min >= 0.0 && e_min < 1.0, "e_min must be in [0, 1)");
    HFEM_ARG_CHECK(t && rho_f && (w_elem || w_slot), "null pointer");
    if (int rc = hfem::use_device(t->device)) return rc;
    const int64_t n = std::max(w_elem ? t->ne : 0, w_slot ? t->n_slots : 0);
    if (t->paired)
        hipLaunchKernelGGL(hfem::topt_weights_kernel<true>, topt_grid(n), dim3(hfem::kToptBlock), 0, (hipStream_t)stream, t->ne,
                           t->n_slots, t->gid, t->gid_b, rho_f, penal, e_min, w_elem, w_slot);
    else
        hipLaunchKernelGGL(hfem::topt_weights_kernel<false>, topt_grid(n), dim3(hfem::kToptBlock), 0, (hipStream_t)stream, t->ne,
                           t->n_slots, t->gid, t->gid_b, rho_f, penal, e_min, w_elem, w_slot);
    return hfem::launch_status("hfem_topt_weights");
}

extern "C" int hfem_topt_filter(hfem_topt *t, const double *in, double *out, int32_t transpose, void *stream) {
    HFEM_ARG_CHECK(t && in && out, "null pointer");
    HFEM_ARG_CHECK(in != out, "out must not alias in (a row gather reads its neighbours)");
    HFEM_ARG_CHECK(transpose == 0 || transpose == 1, "transpose: 0 forward, 1 transpose");
    if (int rc = hfem::use_device(t->device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (t->identity) {
        HFEM_HIP_CHECK(hipMemcpyAsync(out, in, (size_t)t->ne * sizeof(double), hipMemcpyDeviceToDevice, s));
        return 0;
    }
    if (transpose)
        hipLaunchKernelGGL(hfem::topt_filter_kernel<true>, topt_grid(t->ne), dim3(hfem::kToptBlock), 0, s, t->ne, t->f_ptr, t->f_col,
                           t->f_h, t->vol, t->ssum, in, out);
    else
        hipLaunchKernelGGL(hfem::topt_filter_kernel<false>, topt_grid(t->ne), dim3(hfem::kToptBlock), 0, s, t->ne, t->f_ptr, t->f_col,
                           t->f_h, t->vol, t->ssum, in, out);
    return hfem::launch_status("hfem_topt_filter");
}

extern "C" int hfem_topt_energy(hfem_topt *t, const double *x_free, const double *x_fixed, const double *u_free, const double mat[4],
                                double W, int32_t flags, const double *rho_f, double penal, double e_min, double *ce_out,
                                double *dc_out, void *stream) {
    HFEM_ARG_CHECK(std::isfinite(penal) && penal >= 1.0, "penal must be finite and >= 1");
    HFEM_ARG_CHECK(std::isfinite(e_min) && e_min >= 0.0 && e_min < 1.0, "e_min must be in [0, 1)");
    HFEM_ARG_CHECK((flags & ~HFEM_FLAG_PHYSICAL_GRAD) == 0, "flags: only HFEM_FLAG_PHYSICAL_GRAD");
    HFEM_ARG_CHECK(t && x_free && u_free && mat && ce_out, "null pointer");
    HFEM_ARG_CHECK(rho_f || !dc_out, "dc_out needs rho_f");
    const hfem::HostPlan &h = t->plan->host;
    bool fixed_rows = false;
    for (size_t i = 0; i < h.node_src.size(); i += 2) fixed_rows = fixed_rows || h.node_src[i] < 0;
    HFEM_ARG_CHECK(x_fixed || !fixed_rows, "the plan reads fixed coordinate rows: x_fixed must be given");
    const bool quad = !t->paired, b512 = t->paired && h.pair_block == 512;
    HFEM_ARG_CHECK(quad ? h.max_nodes <= 4 * 256 : b512 ? h.max_nodes <= 2 * 512 : h.max_nodes <= 4 * 256,
                   "tile shape outside the energy kernels' instances");
    if (int rc = hfem::use_device(t->device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const bool phys = (flags & HFEM_FLAG_PHYSICAL_GRAD) != 0;
    const hfem::Tri3Consts k = hfem::make_consts(mat, quad ? 1.0 : W, nullptr);
    const hfem::PlanDev pd = hfem::plan_dev(t->plan);
    const int n_tiles = (int)h.tiles.size();
    const size_t lds = (size_t)h.max_nodes * 32;
    const double2 *xf = (const double2 *)x_free, *xx = (const double2 *)x_fixed, *uf = (const double2 *)u_free;
#define HFEM_TOPT_E3(BLOCK, NPT, PH)                                                                                          \
    hipLaunchKernelGGL((hfem::tri3_topt_energy_kernel<BLOCK, NPT, PH>), dim3(n_tiles), dim3(BLOCK), lds, s, pd, xf, xx, uf, k, \
                       t->gid, t->gid_b, rho_f, penal, e_min, ce_out, dc_out, h.max_nodes, h.col_stride, BLOCK == 512 ? 2 : 6)
#define HFEM_TOPT_E4(PH)                                                                                                      \
    hipLaunchKernelGGL((hfem::quad4_topt_energy_kernel<256, 4, PH>), dim3(n_tiles), dim3(256), lds, s, pd, xf, xx, uf, k,      \
                       t->gid, rho_f, penal, e_min, ce_out, dc_out, h.max_nodes, 4)
    if (n_tiles > 0) {
        if (quad) {
            if (phys) HFEM_TOPT_E4(true);
            else HFEM_TOPT_E4(false);
        } else if (b512) {
            if (phys) HFEM_TOPT_E3(512, 2, true);
            else HFEM_TOPT_E3(512, 2, false);
        } else {
            if (phys) HFEM_TOPT_E3(256, 4, true);
            else HFEM_TOPT_E3(256, 4, false);
        }
    }
#undef HFEM_TOPT_E3
#undef HFEM_TOPT_E4
    return hfem::launch_status("hfem_topt_energy");
}

extern "C" int hfem_topt_oc(hfem_topt *t, const double *rho, const double *dc, const double *dv, double vol_target, double move,
                            int32_t n_bisect, double *rho_new, double *rho_f_new, void *stream) {
    HFEM_ARG_CHECK(std::isfinite(vol_target) && vol_target > 0.0, "vol_target must be finite and > 0");
    HFEM_ARG_CHECK(std::isfinite(move) && move > 0.0 && move <= 1.0, "move must be in (0, 1]");
    HFEM_ARG_CHECK(n_bisect >= 1 && n_bisect <= 4096, "n_bisect must be in [1, 4096]");
    HFEM_ARG_CHECK(t && rho && dc && dv && rho_new && rho_f_new, "null pointer");
    HFEM_ARG_CHECK(rho_new != rho && rho_f_new != rho && rho_new != rho_f_new, "rho_new and rho_f_new must not alias rho or each other");
    HFEM_ARG_CHECK(t->vol, "the handle was created without volumes");
    if (int rc = hfem::use_device(t->device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)t->oc_blocks), block(hfem::kToptBlock);
    hipLaunchKernelGGL(hfem::topt_oc_init_kernel, grid, block, 0, s, t->ne, dc, dv, vol_target, t->oc_part, t->oc_ticket, t->oc_st);
    for (int i = 0; i <= n_bisect; ++i) {                     // the evaluation at lambda_hi, then n_bisect halvings
        if (t->identity)
            hipLaunchKernelGGL(hfem::topt_oc_step_kernel<true>, grid, block, 0, s, t->ne, t->f_ptr, t->f_col, t->f_h, t->vol, t->ssum,
                               rho, dc, dv, move, t->oc_part, t->oc_ticket, t->oc_st);
        else
            hipLaunchKernelGGL(hfem::topt_oc_step_kernel<false>, grid, block, 0, s, t->ne, t->f_ptr, t->f_col, t->f_h, t->vol, t->ssum,
                               rho, dc, dv, move, t->oc_part, t->oc_ticket, t->oc_st);
    }
    if (t->identity)
        hipLaunchKernelGGL(hfem::topt_oc_final_kernel<true>, grid, block, 0, s, t->ne, t->f_ptr, t->f_col, t->f_h, t->vol, t->ssum, rho,
                           dc, dv, move, t->oc_st, t->host, rho_new, rho_f_new);
    else
        hipLaunchKernelGGL(hfem::topt_oc_final_kernel<false>, grid, block, 0, s, t->ne, t->f_ptr, t->f_col, t->f_h, t->vol, t->ssum, rho,
                           dc, dv, move, t->oc_st, t->host, rho_new, rho_f_new);
    return hfem::launch_status("hfem_topt_oc");
}

extern "C" int hfem_topt_status(hfem_topt *t, double *status_host, void *stream) {
    HFEM_ARG_CHECK(t && status_host, "null pointer");
    if (int rc = hfem::use_device(t->device)) return rc;
    HFEM_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    for (int i = 0; i < hfem::oStatusN; ++i) status_host[i] = t->host[i];
    return 0;
}
