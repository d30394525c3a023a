// Device-side pieces the frozen-mesh solve's kernels share.  For every kernel with a last workgroup (cg.hip, tri3_cg.hip,
// quad4_cg.hip, tri3_hyper_cg.hip, quad4_hyper_cg.hip): the status publication, the hand-off and the fixed-order partial sum.
// For the element kernels (apply and block diagonal of tri3_cg.hip, quad4_cg.hip, tri3_hyper_cg.hip and quad4_hyper_cg.hip) the phases that do not depend on
// the element: the iteration state, one gathered p row, the write-out of q and p, the p^T q epilogue with alpha and the breakdown halt, and the Jacobi
// block store.  For the diag kernels and the AMG fine-level assembly (tri3_amg.hip): the unit-displacement columns of one
// element, 3 or 4 corners, and the x row code.  For the shifted operator of implicit dynamics (the MASS instances of the
// kernels of tri3_cg.hip, quad4_cg.hip, tri3_hyper_cg.hip and quad4_hyper_cg.hip and of amg_assemble_kernel, tri3_amg.hip): the
// mass coefficients, the QUAD4 Gauss point determinants and shape values, one element's mass row, and one element's mass
// part of an apply.  For the five kernels that also apply the element-scaled operator K(w) (tri3_cg.hip, quad4_cg.hip,
// amg_assemble_kernel): the operator tag ElemOp { Plain, Mass, Scaled } that replaces their MASS.  Last, the launchers of the element kernels, which the PCG
// driver (cg.hip) calls by element kind.  What stays in the element files is what mirrors each element's energy kernel: the
// index loads, the staging of coordinates and p, and the slot loop.
#pragma once
#include <hip/hip_runtime.h>

#include "hfem_amg.h"
#include "hfem_device.h"
#include "hfem_hyper_dev.h"
#include "hfem_plan_dev.h"
#include "hfem_quad4_dev.h"

struct hfem_j2;                      // the J2 state handle (hfem_j2_dev.h)

namespace hfem {

__device__ __forceinline__ void publish(const double *st, double *host) {
    if (host)
        for (int i = 0; i < kStatusN; ++i) host[i] = st[i];
}

// The last-workgroup hand-off (cdna_hip_programming.md section 6, Guideline 16, write-through form): every partial is stored
// with put_partial (agent-scope relaxed store: write-through, no release fence -- a release in every workgroup writes back its
// XCD's L2 under the running tiles), every wave drains its stores, lane 0 takes a relaxed agent-scope ticket; the workgroup
// that draws n - 1 is the reducer and reads the partials with agent-scope loads (get_partial).  `flag` is one word of the
// block's own LDS array.  Returns true in every thread of the last block.
__device__ __forceinline__ void put_partial(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double get_partial(const double *p) {
    return __hip_atomic_load(const_cast<double *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ bool last_block(unsigned *ticket, unsigned n, int *flag) {
    __builtin_amdgcn_s_waitcnt(0x0F70);                     // vmcnt(0): this wave's stores have been acknowledged
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = t == n - 1;
        if (last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
        *flag = last;
    }
    __syncthreads();
    return *flag != 0;
}

// Fixed-order sum of the n partials by one block (strided lanes, then block_sum's wave order).  Result in thread 0.
template <int BLOCK>
__device__ __forceinline__ double ordered_sum(const double *v, int n, double *red) {
    double a = 0.0;
    for (int i = threadIdx.x; i < n; i += BLOCK) a += get_partial(v + i);
    __syncthreads();                                        // red[] may still be read by the caller's earlier reduction
    return block_sum(a, red);
}

// ---------------------------------------------------------------- q = K p: the phases both elements share
// What an apply launch is: an iteration (st != NULL: p = z + beta p_old, stored to the other buffer of the ping-pong pair
// picked by the parity of kIter) or the standalone apply (st == NULL: p = z as given, nothing stored).
struct CgIter {
    double beta = 0.0;
    const double2 *p_old = nullptr;
    double2 *p_new = nullptr;
};

__device__ __forceinline__ CgIter cg_iter(const double *st, double2 *pbuf0, double2 *pbuf1) {
    CgIter it;
    if (st) {
        const int par = ((long long)st[kIter]) & 1;
        it.beta = st[kBeta];
        it.p_old = par ? pbuf1 : pbuf0;
        it.p_new = par ? pbuf0 : pbuf1;
    }
    return it;
}

// One gathered row of p through the u row map: 0 on a fixed row (row < 0), else z, plus beta p_old when iterating.
__device__ __forceinline__ double2 gather_p(const CgIter &it, const double2 *__restrict__ z, int row) {
    double2 p = make_double2(0.0, 0.0);
    if (row >= 0) {
        p = z[row];
        if (it.p_old) {
            const double2 o = it.p_old[row];
            p.x = __builtin_fma(it.beta, o.x, p.x);
            p.y = __builtin_fma(it.beta, o.y, p.y);
        }
    }
    return p;
}

// Owned free rows: q (one 16-byte store per row), and (iterations) the new p into the other buffer.
template <int BLOCK, int NPT>
__device__ __forceinline__ void store_q_p(const int2 (&s)[NPT], int n_owned, const double *acc0, const double *acc1,
                                          const double2 *nd_p, double2 *__restrict__ q, double2 *p_new) {
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int l = threadIdx.x + j * BLOCK;
        if (l < n_owned && s[j].y >= 0) {
            q[s[j].y] = make_double2(acc0[l], acc1[l]);
            if (p_new) p_new[s[j].y] = nd_p[l];
        }
    }
}

// The epilogue, in two parts around the caller's barrier and write-out.  First: every wave's sum of the home elements'
// energy into red[].
__device__ __forceinline__ void wave_energy(double e_loc, double *red) {
    const double w = wave_sum(e_loc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
}

// Second: the tile's partial of p^T q; the last workgroup (ticket) sums the partials in tile order and writes pq_out[0]
// (standalone) or alpha and kPq, and halts with breakdown where K is not positive definite on p.  red: BLOCK / 64 doubles
// + one flag word.
template <int BLOCK>
__device__ __forceinline__ void apply_finish(double *red, double *__restrict__ partials, int slot, unsigned *ticket, int n_tiles,
                                             double *st, double *host, double *pq_out) {
    const int tid = threadIdx.x;
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

// ---------------------------------------------------------------- block Jacobi and the AMG fine level
// The symmetric 2x2 block [[a, b], [b, c]] of free row `row` (3 doubles) into diag (optional), its inverse into dinv; the
// identity for precond "none" or a block that is not positive definite.
__device__ __forceinline__ void store_jacobi_block(double *__restrict__ diag, double *__restrict__ dinv, int row, int precond,
                                                   double a, double b, double c) {
    const size_t r = (size_t)row * 3;
    if (diag) { diag[r] = a; diag[r + 1] = b; diag[r + 2] = c; }
    const double det = a * c - b * b;
    if (precond && a > 0.0 && det > 0.0 && isfinite(det)) {
        const double inv = 1.0 / det;
        dinv[r] = c * inv; dinv[r + 1] = -b * inv; dinv[r + 2] = a * inv;
    } else {
        dinv[r] = 1.0; dinv[r + 1] = 0.0; dinv[r + 2] = 1.0;
    }
}

// Columns (a, x) and (a, y) of K_e: the element's u-gradient at u_a = e_x (gu) and at u_a = e_y (hu), u_b = 0 (b != a).
// By symmetry these are also rows (a, x) and (a, y).
template <bool PHYS>
__device__ __forceinline__ void unit_columns(const double2 (&X)[3], int a, const Tri3Consts &k, double2 (&gu)[3], double2 (&hu)[3]) {
    const double2 o = make_double2(0.0, 0.0), ex = make_double2(1.0, 0.0), ey = make_double2(0.0, 1.0);
    double2 gx[3];
    tri3_element<true, false, PHYS>(X[0], X[1], X[2], a == 0 ? ex : o, a == 1 ? ex : o, a == 2 ? ex : o, k, gx, gu);
    tri3_element<true, false, PHYS>(X[0], X[1], X[2], a == 0 ? ey : o, a == 1 ? ey : o, a == 2 ? ey : o, k, gx, hu);
}

template <bool PHYS>
__device__ __forceinline__ void unit_columns(const double2 (&X)[4], int a, const Tri3Consts &k, double2 (&gu)[4], double2 (&hu)[4]) {
    const double2 o = make_double2(0.0, 0.0), ex = make_double2(1.0, 0.0), ey = make_double2(0.0, 1.0);
    const double2 Ux[4] = {a == 0 ? ex : o, a == 1 ? ex : o, a == 2 ? ex : o, a == 3 ? ex : o};
    const double2 Uy[4] = {a == 0 ? ey : o, a == 1 ? ey : o, a == 2 ? ey : o, a == 3 ? ey : o};
    quad4_element_u<PHYS>(X, Ux, k, gu);
    quad4_element_u<PHYS>(X, Uy, k, hu);
}

// A coordinate row by its x row code: a free row, or fixed row -1 - code.
__device__ __forceinline__ double2 x_row(const double2 *x_free, const double2 *x_fixed, int32_t code) {
    return code >= 0 ? x_free[code] : x_fixed[-1 - code];
}

// ---------------------------------------------------------------- the shifted operator A = c_K K + c_M M
// The mass part of the MASS instances (tri3_cg.hip, quad4_cg.hip, amg_assemble_kernel) as two run-time coefficients (c_M
// includes the density), so consistent and lumped mass are one instance.  K's part is scaled on the host: the material
// constants times c_K.  Every instance takes a DynMass by value; MASS = false does not read it.
//   TRI3   M_e[a][b] = |det J| (m_off + m_dd delta_ab):  consistent m_off = m_dd = c_M / 24;  lumped m_off = 0, m_dd = c_M / 6
//   QUAD4  M_e[a][b] = sum_q |det J_q| N_a(q) (m_off N_b(q) + m_dd delta_ab):  consistent m_off = c_M, m_dd = 0;  lumped the reverse
struct DynMass {
    double m_off = 0.0, m_dd = 0.0;
};
inline DynMass dyn_mass(bool quad, double c_m, bool lumped) {
    DynMass m;
    if (quad) { m.m_off = lumped ? 0.0 : c_m; m.m_dd = lumped ? c_m : 0.0; }
    else { m.m_off = lumped ? 0.0 : c_m / 24.0; m.m_dd = lumped ? c_m / 6.0 : c_m / 24.0; }
    return m;
}
// A stiffness entry plus its mass entry in the MASS instance, the stiffness entry itself otherwise: never "+ 0.0" in a plain
// instance (without fast-math that is a real add, and it changes a -0.0).
template <bool MASS>
__device__ __forceinline__ double with_mass(double v, double m) {
    if constexpr (MASS) return v + m;
    else return v;
}
// Which operator an instance of tri3_cg_apply_kernel, tri3_cg_diag_kernel, quad4_cg_apply_kernel, quad4_cg_diag_kernel or
// amg_assemble_kernel applies: K, the shifted c_K K + c_M M, or the element-scaled K(w) = sum_e w_e K_e.  One tag,
// so a mass-and-scaled instance cannot be written.  Mass and Scaled code sits behind if constexpr: the Plain instance gains
// neither "+ 0.0" nor "* 1.0", and no instance reads the other's argument (DynMass dm | the weight pointer).
enum class ElemOp { Plain, Mass, Scaled };
// A stiffness entry times the element's weight in the Scaled instance, the entry itself otherwise
template <ElemOp OP>
__device__ __forceinline__ double with_weight(double v, double w) {
    if constexpr (OP == ElemOp::Scaled) return w * v;
    else return v;
}
inline Tri3Consts scaled_consts(Tri3Consts k, double c_k) {
    k.c11 *= c_k; k.c12 *= c_k; k.c22 *= c_k; k.c33 *= c_k;
    return k;
}

// |det J_q| at the four 2x2 Gauss points, in quad4_element_u's order (-,-) (+,-) (-,+) (+,+) and from its bilinear
// coefficients (the unscaled ones carry 16 |det|).
__device__ __forceinline__ void quad4_abs_dets(const double2 (&Xn)[4], double (&ad)[4]) {
    const double gp = 0.57735026918962576451;   // 1/sqrt(3)
    double a1[2], a2[2], a3[2];
    {
        const double v[2][4] = {{Xn[0].x, Xn[1].x, Xn[2].x, Xn[3].x}, {Xn[0].y, Xn[1].y, Xn[2].y, Xn[3].y}};
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const double s = v[i][1] - v[i][0], t = v[i][2] - v[i][3];
            a1[i] = s + t;
            a3[i] = t - s;
            a2[i] = (v[i][3] - v[i][0]) + (v[i][2] - v[i][1]);
        }
    }
    const double am = a1[0] - gp * a3[0], ap = a1[0] + gp * a3[0], cm = a1[1] - gp * a3[1], cp = a1[1] + gp * a3[1];
    const double bm = a2[0] - gp * a3[0], bp = a2[0] + gp * a3[0], dm = a2[1] - gp * a3[1], dp = a2[1] + gp * a3[1];
    ad[0] = 0.0625 * fabs(am * dm - bm * cm); ad[1] = 0.0625 * fabs(am * dp - bp * cm);
    ad[2] = 0.0625 * fabs(ap * dm - bm * cp); ad[3] = 0.0625 * fabs(ap * dp - bp * cp);
}

// N_a(q) of the 2x2 rule: one of three values by how many of the two reference coordinates of corner a and point q agree
__device__ __forceinline__ constexpr double quad4_n(int a, int q) {
    const double gp = 0.57735026918962576451;
    const double xi = (q & 1) ? gp : -gp, eta = (q & 2) ? gp : -gp;
    return 0.25 * (1.0 + corner_xi(a) * xi) * (1.0 + corner_eta(a) * eta);
}

// Row a of one element's mass in the two coefficients, a a run-time corner (selects and signs, never an index of a local
// array): mrow[b] = M_e[a][b].  For the AMG fine level of A (tri3_amg.hip); the diag kernels form their M_e[a][a] inline.
__device__ __forceinline__ void dyn_mass_row(const double2 (&X)[3], int a, const DynMass &m, double (&mrow)[3]) {
    const double A = fabs((X[0].x - X[2].x) * (X[1].y - X[2].y) - (X[1].x - X[2].x) * (X[0].y - X[2].y));
#pragma unroll
    for (int b = 0; b < 3; ++b) mrow[b] = A * (m.m_off + (b == a ? m.m_dd : 0.0));
}
__device__ __forceinline__ void dyn_mass_row(const double2 (&X)[4], int a, const DynMass &m, double (&mrow)[4]) {
    double ad[4];
    quad4_abs_dets(X, ad);
#pragma unroll
    for (int b = 0; b < 4; ++b) mrow[b] = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double wa = ad[q] * quad4_n(a, q);
#pragma unroll
        for (int b = 0; b < 4; ++b) mrow[b] += wa * (m.m_off * quad4_n(b, q) + (b == a ? m.m_dd : 0.0));
    }
}

// One element's mass part in the slot loop of an apply kernel (tri3_cg.hip, quad4_cg.hip and the Neo-Hookean tangent's
// tri3_hyper_cg.hip, quad4_hyper_cg.hip): from the corner coordinates and the corner values of p the slot already holds.
// TRI3: adds (M_e p)_a to the three rows, returns 1/2 p^T M_e p.
__device__ __forceinline__ double tri3_mass_rows(const double2 X0, const double2 X1, const double2 X2, const double2 P0,
                                                 const double2 P1, const double2 P2, const DynMass &m, double2 (&gu)[3]) {
    const double det = (X0.x - X2.x) * (X1.y - X2.y) - (X1.x - X2.x) * (X0.y - X2.y);
    const double A = fabs(det);
    const double wo = A * m.m_off, wd = A * m.m_dd;
    const double sx = wo * (P0.x + P1.x + P2.x), sy = wo * (P0.y + P1.y + P2.y);
    const double2 r0 = make_double2(__builtin_fma(wd, P0.x, sx), __builtin_fma(wd, P0.y, sy));
    const double2 r1 = make_double2(__builtin_fma(wd, P1.x, sx), __builtin_fma(wd, P1.y, sy));
    const double2 r2 = make_double2(__builtin_fma(wd, P2.x, sx), __builtin_fma(wd, P2.y, sy));
    gu[0].x += r0.x; gu[0].y += r0.y; gu[1].x += r1.x; gu[1].y += r1.y; gu[2].x += r2.x; gu[2].y += r2.y;
    return 0.5 * (P0.x * r0.x + P0.y * r0.y + P1.x * r1.x + P1.y * r1.y + P2.x * r2.x + P2.y * r2.y);
}

// QUAD4: adds (M_e p)_a to the four rows, returns 1/2 p^T M_e p.
__device__ __forceinline__ double quad4_mass_rows(const double2 (&Xn)[4], const double2 (&Pn)[4], const DynMass &m,
                                                  double2 (&gu)[4]) {
    double ad[4];
    quad4_abs_dets(Xn, ad);
    double2 r[4];
    double nl[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) { r[a] = make_double2(0.0, 0.0); nl[a] = 0.0; }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        double hx = 0.0, hy = 0.0;
#pragma unroll
        for (int b = 0; b < 4; ++b) { hx += quad4_n(b, q) * Pn[b].x; hy += quad4_n(b, q) * Pn[b].y; }
        const double w = ad[q] * m.m_off;
        hx *= w; hy *= w;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            r[a].x += quad4_n(a, q) * hx; r[a].y += quad4_n(a, q) * hy;
            nl[a] += quad4_n(a, q) * ad[q];
        }
    }
    double e = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const double wl = nl[a] * m.m_dd;
        r[a].x = __builtin_fma(wl, Pn[a].x, r[a].x); r[a].y = __builtin_fma(wl, Pn[a].y, r[a].y);
        gu[a].x += r[a].x; gu[a].y += r[a].y;
        e += Pn[a].x * r[a].x + Pn[a].y * r[a].y;
    }
    return 0.5 * e;
}

// ---------------------------------------------------------------- element launchers (tri3_cg.hip, quad4_cg.hip)
// What the driver binds of a solve, by value.  block: threads per tile of a paired TRI3 plan (QUAD4 tiles are 256).
struct CgElemArgs {
    const hfem_plan *plan = nullptr;
    int n_tiles = 0, block = 256;
    bool phys = false;
    const double2 *x_free = nullptr, *x_fixed = nullptr;
    Tri3Consts k{};
    size_t lds = 0;
    hipStream_t s = nullptr;
    // the Neo-Hookean tangent (tri3_hyper_cg.hip, quad4_hyper_cg.hip): the linearisation point's rows and the material
    const double2 *u_lin_free = nullptr, *u_fixed = nullptr;
    HyperConsts hk{};
    // quad4_hyper_cg.hip: c = mu - lambda L per slot and Gauss point, [n_tiles][4][elem_stride]; the diag launch of a
    // linearisation writes it, its apply launches read it instead of calling log1p
    double *cq = nullptr;
    // shifted: the operator A = c_K K + c_M M (the MASS instances of tri3_cg.hip, quad4_cg.hip): k carries c_K, dm the mass
    // coefficients; on the Neo-Hookean tangent A = c_K K_T + c_M M (the MASS instances of tri3_hyper_cg.hip,
    // quad4_hyper_cg.hip): hk's lambda and mu carry c_K
    bool shifted = false;
    DynMass dm{};
    // non-null: the element-scaled operator K(w) = sum_e w_e K_e (the Scaled instances of tri3_cg.hip, quad4_cg.hip): one
    // weight record per slot of the plan, addressed as elem_pack (a paired TRI3 plan: double2 {w_A, w_B}; a QUAD4 plan: one
    // double).  Never together with shifted: every setup entry point that binds one clears the other (cg.hip)
    const double *w_slot = nullptr;
    // the J2 elastoplastic tangent (tri3_j2.hip): the state handle (material, committed state, element ids: read by the
    // linearisation launch only) and the tangent records [n_tiles][5][elem_stride] it writes and the apply launches read
    const hfem_j2 *j2 = nullptr;
    double *j2_tan = nullptr;
};
// The operator tag of a launch, where the launch macros of tri3_cg.hip and quad4_cg.hip picked MASS: LAUNCH(..., tag)
#define HFEM_CG_OP(LAUNCH, ...)                                                                                               \
    do {                                                                                                                      \
        if (A.shifted) LAUNCH(__VA_ARGS__, Mass);                                                                             \
        else if (A.w_slot) LAUNCH(__VA_ARGS__, Scaled);                                                                       \
        else LAUNCH(__VA_ARGS__, Plain);                                                                                      \
    } while (0)
// q = K p, q = A p where A.shifted, q = K(w) p where A.w_slot (st != NULL an iteration, st == NULL the standalone apply)
void launch_tri3_cg_apply(const CgElemArgs &A, const double2 *z, double2 *pbuf0, double2 *pbuf1, double2 *q, double *partials,
                          unsigned *ticket, double *st, double *host, double *pq_out);
void launch_quad4_cg_apply(const CgElemArgs &A, const double2 *z, double2 *pbuf0, double2 *pbuf1, double2 *q, double *partials,
                           unsigned *ticket, double *st, double *host, double *pq_out);
// 2x2 diagonal blocks of K (of A where A.shifted, of K(w) where A.w_slot) and their inverses (store_jacobi_block)
void launch_tri3_cg_diag(const CgElemArgs &A, double *diag, double *dinv, int precond);
void launch_quad4_cg_diag(const CgElemArgs &A, double *diag, double *dinv, int precond);
// The Neo-Hookean tangent at A.u_lin_free (tri3_hyper_cg.hip, one-element-per-slot TRI3 plan): q = K_T p, and the blocks with
// info[2] = {min J, inverted count} of the linearisation point (work: 3 * n_tiles doubles; info may be NULL)
void launch_tri3_hyper_cg_apply(const CgElemArgs &A, const double2 *z, double2 *pbuf0, double2 *pbuf1, double2 *q,
                                double *partials, unsigned *ticket, double *st, double *host, double *pq_out);
void launch_tri3_hyper_cg_diag(const CgElemArgs &A, double *diag, double *dinv, int precond, double *work, double *info);
// info[2] = {min J, inverted count} from a diag launch's tile partials work[3][n] (one block; tri3_hyper_cg.hip)
void launch_hyper_info(const double *work, int n, double *info, hipStream_t s);
// The same two on the QUAD4 Neo-Hookean tangent (quad4_hyper_cg.hip, the model's own QUAD4 plan; A.hk carries lambda and mu,
// W is not read).  Threads per tile of both kernels: the driver sizes their LDS with it.
constexpr int kQuad4HyperCgBlock = 256;
void launch_quad4_hyper_cg_apply(const CgElemArgs &A, const double2 *z, double2 *pbuf0, double2 *pbuf1, double2 *q,
                                 double *partials, unsigned *ticket, double *st, double *host, double *pq_out);
void launch_quad4_hyper_cg_diag(const CgElemArgs &A, double *diag, double *dinv, int precond, double *work, double *info);
// The J2 elastoplastic tangent (tri3_j2.hip; A.j2 and A.j2_tan bound; the one-element-per-slot TRI3 plan): q = K_T p from the
// stored records, and the linearisation at A.u_lin_free -- records, blocks and info[2] = {plastic count, 0} (work: n_tiles
// doubles; info may be NULL)
void launch_tri3_j2_apply(const CgElemArgs &A, const double2 *z, double2 *pbuf0, double2 *pbuf1, double2 *q, double *partials,
                          unsigned *ticket, double *st, double *host, double *pq_out);
void launch_tri3_j2_diag(const CgElemArgs &A, double *diag, double *dinv, int precond, double *work, double *info);

}  // namespace hfem
