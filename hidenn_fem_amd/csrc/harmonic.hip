// Harmonic frequency response, gfx950 (MI355X) (hidenn_fem_amd/harmonic.py): the steady state of
// M u'' + C u' + K u = Re(b e^{i w t}), C = alpha_R M + beta_R K (+ structural damping i eta K), over the free u rows:
//   A u^ = b^,   A = z_K K + z_M M,   z_K = 1 + i (w beta_R + eta),   z_M = rho (-w^2 + i w alpha_R)
// A is complex SYMMETRIC (not Hermitian) and its real part is indefinite above the first resonance, so neither the shifted
// operator of cg.hip (coefficients >= 0) nor its PCG driver (halts on p^T A p <= 0) applies.  This file holds both new pieces:
//   tri3_harm_apply_kernel / quad4_harm_apply_kernel   q = A p on complex vectors: siblings of the Mass instances of
//                     tri3_cg.hip / quad4_cg.hip on the same tile plans, built from the same phases (hfem_cg_dev.h).  A complex
//                     vector is an fp64 block vector [2][n_u][2]: plane 0 real, plane 1 imaginary, each in the storage order of
//                     u_free (a plane is what hfem_amg_vcycle takes).  Coordinates and index records are read once per tile;
//                     both planes of p go into LDS; per element K_e p_r, K_e p_i (tri3_element / quad4_element_u on the
//                     UNSCALED material), M_e p_r, M_e p_i (tri3_mass_rows / quad4_mass_rows, unit coefficient, consistent or
//                     lumped as DynMass, always |det J|) are formed from the corner rows the slot holds and combined with the
//                     four run-time coefficients (device memory: a captured launch serves every frequency):
//                       q_r = Re z_K K p_r - Im z_K K p_i + Re z_M M p_r - Im z_M M p_i
//                       q_i = Im z_K K p_r + Re z_K K p_i + Im z_M M p_r + Re z_M M p_i
//                     into four LDS accumulators per owned row.  One complex partial of the UNCONJUGATED p^T A p per tile over
//                     its home elements; the ticket workgroup sums the partials in tile order (mu) and, in an iteration, forms
//                     alpha = rho / mu and the breakdown halt.
//                     LDS bytes of a tile: 48 x max local nodes + 32 x max owned rows + 8 x (2 x threads / 64 + 2).
//   COCG driver       preconditioned conjugate orthogonal conjugate gradients with a REAL SPD preconditioner T (T A stays
//                     complex symmetric in the bilinear form):
//                       r = b - A x0, z = T r, p = z, rho = r^T z
//                       loop: q = A p, mu = p^T q, alpha = rho / mu;  x += alpha p, r -= alpha q, stop on |r|_2;
//                             z = T r, rho' = r^T z, beta = rho' / rho, p = z + beta p
//                     every product unconjugated, the stopping norm Hermitian.  All scalars are reduced and consumed on the
//                     device in a fixed order; once the status record says halted every later launch returns at once, so x keeps
//                     the last good iterate.  Launches per iteration: T = none / block Jacobi: 3 (apply, vector update with z,
//                     rho, beta and the stopping test fused, p update); T = AMG: 6 (apply, vector update, one V-cycle per plane,
//                     rho and beta, p update).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>

#include "hfem_amg.h"
#include "hfem_cg_dev.h"
#include "hfem_device.h"
#include "hfem_plan_dev.h"

namespace hfem {
namespace {

constexpr int kHarmVecBlock = 256, kHarmVecMaxBlocks = 1024;

// The status record: hfem_cg_status's slots where the two solvers mean the same thing (iterations, |r|, |b|, reason, tolerance,
// max_iter, halted, rtol-wins; the real parts of rho, alpha, beta, mu in the slots of rho, alpha, beta, p^T K p), the imaginary
// parts in the four slots the real driver leaves unused.
enum { hIter = kIter, hRnorm = kRnorm, hBnorm = kFnorm, hRhoRe = kRho, hReason = kReason, hAlphaRe = kAlpha, hBetaRe = kBeta,
       hMuRe = kPq, hTol = kTol, hMaxIter = kMaxIter, hHalted = kHalted, hRtolWins = kRtolWins, hRhoIm = 12, hAlphaIm = 13,
       hBetaIm = 14, hMuIm = 15 };
static_assert(kStatusN == 16, "the harmonic status record fills the CG record's 16 slots");

// coef[4] (device) = {Re z_K, Im z_K, Re z_M, Im z_M}
struct HarmCoef {
    double kr, ki, mr, mi;
};
__device__ __forceinline__ HarmCoef load_coef(const double *__restrict__ c) {
    HarmCoef z;
    z.kr = c[0]; z.ki = c[1]; z.mr = c[2]; z.mi = c[3];
    return z;
}

__global__ void harm_set_coef_kernel(double *coef, double kr, double ki, double mr, double mi) {
    coef[0] = kr; coef[1] = ki; coef[2] = mr; coef[3] = mi;
}

// One corner row of q from the four real element products, and its share of the unconjugated p^T q.
__device__ __forceinline__ void harm_combine(const HarmCoef c, const double2 kr, const double2 ki, const double2 mr,
                                             const double2 mi, const double2 pr, const double2 pi, double2 &qr, double2 &qi,
                                             double &er, double &ei) {
    qr.x = c.kr * kr.x - c.ki * ki.x + c.mr * mr.x - c.mi * mi.x;
    qr.y = c.kr * kr.y - c.ki * ki.y + c.mr * mr.y - c.mi * mi.y;
    qi.x = c.ki * kr.x + c.kr * ki.x + c.mi * mr.x + c.mr * mi.x;
    qi.y = c.ki * kr.y + c.kr * ki.y + c.mi * mr.y + c.mr * mi.y;
    er += pr.x * qr.x + pr.y * qr.y - pi.x * qi.x - pi.y * qi.y;
    ei += pr.x * qi.x + pr.y * qi.y + pi.x * qr.x + pi.y * qr.y;
}

// One TRI3 element: q_e = A_e p_e on both planes; adds p_e^T A_e p_e (complex, unconjugated) to (er, ei).
template <bool PHYS>
__device__ __forceinline__ void tri3_harm_element(const double2 X0, const double2 X1, const double2 X2, const double2 R0,
                                                  const double2 R1, const double2 R2, const double2 I0, const double2 I1,
                                                  const double2 I2, const Tri3Consts &k, const DynMass &dm, const HarmCoef c,
                                                  double2 (&qr)[3], double2 (&qi)[3], double &er, double &ei) {
    const double2 o = make_double2(0.0, 0.0);
    double2 gx[3], kr[3], ki[3], mr[3] = {o, o, o}, mi[3] = {o, o, o};
    tri3_element<true, false, PHYS>(X0, X1, X2, R0, R1, R2, k, gx, kr);
    tri3_element<true, false, PHYS>(X0, X1, X2, I0, I1, I2, k, gx, ki);
    tri3_mass_rows(X0, X1, X2, R0, R1, R2, dm, mr);
    tri3_mass_rows(X0, X1, X2, I0, I1, I2, dm, mi);
    harm_combine(c, kr[0], ki[0], mr[0], mi[0], R0, I0, qr[0], qi[0], er, ei);
    harm_combine(c, kr[1], ki[1], mr[1], mi[1], R1, I1, qr[1], qi[1], er, ei);
    harm_combine(c, kr[2], ki[2], mr[2], mi[2], R2, I2, qr[2], qi[2], er, ei);
}

// The epilogue of both apply kernels (the complex apply_finish): the tile's partial of p^T A p from the waves' sums in
// red[0 .. BLOCK/64) (real) and red[BLOCK/64 .. 2 BLOCK/64) (imaginary); the ticket workgroup sums the partials in tile order
// and writes pq_out[2] (standalone) or mu and alpha = rho / mu, and halts with breakdown on |mu| = 0, |rho| = 0 or a
// non-finite alpha -- before x moves.  red: 2 BLOCK / 64 doubles + one flag word.
template <int BLOCK>
__device__ __forceinline__ void harm_apply_finish(double *red, double *__restrict__ partials, int slot, unsigned *ticket,
                                                  int n_tiles, double *st, double *host, double *pq_out) {
    constexpr int NW = BLOCK / 64;
    const int tid = threadIdx.x;
    if (tid == 0) {
        double tr = 0.0, ti = 0.0;
#pragma unroll
        for (int w = 0; w < NW; ++w) { tr += red[w]; ti += red[NW + w]; }
        put_partial(partials + slot, tr);
        put_partial(partials + n_tiles + slot, ti);
    }
    if (!last_block(ticket, (unsigned)n_tiles, reinterpret_cast<int *>(red + 2 * NW))) return;
    const double mr = ordered_sum<BLOCK>(partials, n_tiles, red);
    const double mi = ordered_sum<BLOCK>(partials + n_tiles, n_tiles, red);
    if (tid == 0) {
        if (!st) {
            pq_out[0] = mr;
            pq_out[1] = mi;
            return;
        }
        const double rr = st[hRhoRe], ri = st[hRhoIm];
        const double den = mr * mr + mi * mi;
        const double ar = (rr * mr + ri * mi) / den, ai = (ri * mr - rr * mi) / den;
        st[hMuRe] = mr; st[hMuIm] = mi;
        st[hAlphaRe] = ar; st[hAlphaIm] = ai;
        if (den == 0.0 || (rr == 0.0 && ri == 0.0) || !isfinite(ar) || !isfinite(ai)) {
            st[hHalted] = 1.0;
            st[hReason] = kBreakdown;
            publish(st, host);
        }
    }
}

// Owned free rows of q, both planes (one 16-byte store per row and plane).
template <int BLOCK, int NPT>
__device__ __forceinline__ void harm_store_q(const int2 (&s)[NPT], int n_owned, const double *acc, int cap_owned,
                                             double2 *__restrict__ q, int64_t n_u) {
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int l = threadIdx.x + j * BLOCK;
        if (l < n_owned && s[j].y >= 0) {
            q[s[j].y] = make_double2(acc[l], acc[cap_owned + l]);
            q[n_u + s[j].y] = make_double2(acc[2 * cap_owned + l], acc[3 * cap_owned + l]);
        }
    }
}

// ---------------------------------------------------------------- q = A p, TRI3 (paired plan; tri3_cg_apply_kernel's frame)
// st != NULL: an iteration (mu, alpha written, breakdown halt); st == NULL: the standalone apply (pq_out[2] = p^T q).
// LDS: xy[cap_nodes] double2 | p_r[cap_nodes] double2 | p_i[cap_nodes] double2 | acc[4][cap_owned] | red[2 BLOCK / 64 + 2]
template <int BLOCK, int NPT, int EPT, bool PHYS>
__global__ __launch_bounds__(BLOCK) void tri3_harm_apply_kernel(
    PlanDev pd, int n_tiles, const double2 *__restrict__ x_free, const double2 *__restrict__ x_fixed,
    const double2 *__restrict__ p, double2 *__restrict__ q, int64_t n_u, Tri3Consts k, DynMass dm,
    const double *__restrict__ coef, double *__restrict__ partials, unsigned *ticket, double *st, double *host, double *pq_out,
    int cap_nodes, int cap_owned, int col_stride) {
    if (st && st[hHalted] != 0.0) return;                   // uniform over the grid: nothing is written after a halt
    extern __shared__ double2 lds[];
    double2 *nd_xy = lds, *nd_pr = lds + cap_nodes, *nd_pi = lds + 2 * cap_nodes;
    double *acc = reinterpret_cast<double *>(lds + 3 * cap_nodes);
    double *red = acc + 4 * cap_owned;
    const int tid = threadIdx.x;
    const HarmCoef zc = load_coef(coef);
    const int slot = xcd_tile((int)blockIdx.x, (int)gridDim.x);
    int2 s[NPT];
    const int2 *src = pd.node_src + (size_t)slot * pd.node_stride;
#pragma unroll
    for (int j = 0; j < NPT; ++j) s[j] = src[min(tid + j * BLOCK, pd.node_stride - 1)];
    const TileDesc d = pd.tiles[slot];
    uint32_t w0[EPT], w1[EPT];
    const size_t rec0 = (size_t)slot * pd.elem_stride;
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const size_t i = rec0 + min(tid + j * col_stride, pd.elem_stride - 1);
        w0[j] = pd.elem_pack[i];
        w1[j] = pd.elem_pack_hi[i];
    }
    const int n_owned = d.n_owned;
    // gather: coordinates through the x row map, both planes of p through the u row map (fixed u rows are 0)
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int l = tid + j * BLOCK;
        const double2 vx = *(s[j].x >= 0 ? x_free + s[j].x : x_fixed + ~s[j].x);
        double2 vr = make_double2(0.0, 0.0), vi = make_double2(0.0, 0.0);
        if (s[j].y >= 0) { vr = p[s[j].y]; vi = p[n_u + s[j].y]; }
        if (l < d.n_node) { nd_xy[l] = vx; nd_pr[l] = vr; nd_pi[l] = vi; }
        if (l < n_owned) { acc[l] = 0.0; acc[cap_owned + l] = 0.0; acc[2 * cap_owned + l] = 0.0; acc[3 * cap_owned + l] = 0.0; }
    }
#pragma unroll
    for (int j = 0; j < EPT; ++j)
        if (!(tid < col_stride && tid + j * col_stride < d.n_elem)) { w0[j] = kSkipBit; w1[j] = 0u; }
    __syncthreads();
    auto add_row = [&](int l, const double2 gr, const double2 gi) {
        unsafeAtomicAdd(&acc[l], gr.x);
        unsafeAtomicAdd(&acc[cap_owned + l], gr.y);
        unsafeAtomicAdd(&acc[2 * cap_owned + l], gi.x);
        unsafeAtomicAdd(&acc[3 * cap_owned + l], gi.y);
    };
    double er_loc = 0.0, ei_loc = 0.0;
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const uint32_t a = w0[j], b = w1[j];
        if (!(a & kSkipBit)) {
            const int ln = (int)(a & kLocalMask), lb = (int)((a >> kLocalBits) & kLocalMask),
                      lc = (int)((a >> (2 * kLocalBits)) & kLocalMask);
            const double2 Xn = nd_xy[ln], Rn = nd_pr[ln], In = nd_pi[ln], Xc = nd_xy[lc], Rc = nd_pr[lc], Ic = nd_pi[lc];
            double2 snr, sni, scr, sci;
            {
                const double2 Xb = nd_xy[lb], Rb = nd_pr[lb], Ib = nd_pi[lb];
                double2 qr[3], qi[3];
                double er = 0.0, ei = 0.0;
                tri3_harm_element<PHYS>(Xn, Xb, Xc, Rn, Rb, Rc, In, Ib, Ic, k, dm, zc, qr, qi, er, ei);
                if (a & kHomeBit) { er_loc += er; ei_loc += ei; }
                if (lb < n_owned) add_row(lb, qr[1], qi[1]);
                snr = qr[0]; sni = qi[0]; scr = qr[2]; sci = qi[2];
            }
            if (b & kHasBBit) {                             // B = (n, c, d)
                const int ld = (int)(b & kLocalMask);
                const double2 Xd = nd_xy[ld], Rd = nd_pr[ld], Id = nd_pi[ld];
                double2 qr[3], qi[3];
                double er = 0.0, ei = 0.0;
                tri3_harm_element<PHYS>(Xn, Xc, Xd, Rn, Rc, Rd, In, Ic, Id, k, dm, zc, qr, qi, er, ei);
                if (b & kHomeBBit) { er_loc += er; ei_loc += ei; }
                if (ld < n_owned) add_row(ld, qr[2], qi[2]);
                snr.x += qr[0].x; snr.y += qr[0].y; sni.x += qi[0].x; sni.y += qi[0].y;
                scr.x += qr[1].x; scr.y += qr[1].y; sci.x += qi[1].x; sci.y += qi[1].y;
            }
            if (ln < n_owned) add_row(ln, snr, sni);
            if (lc < n_owned) add_row(lc, scr, sci);
        }
    }
    wave_energy(er_loc, red);
    wave_energy(ei_loc, red + BLOCK / 64);
    __syncthreads();
    harm_store_q<BLOCK>(s, n_owned, acc, cap_owned, q, n_u);
    harm_apply_finish<BLOCK>(red, partials, slot, ticket, n_tiles, st, host, pq_out);
}

// ---------------------------------------------------------------- q = A p, QUAD4 (the model's own plan; quad4_cg_apply_kernel's frame)
template <int BLOCK, int NPT, int EPT, bool PHYS>
__global__ __launch_bounds__(BLOCK) void quad4_harm_apply_kernel(
    PlanDev pd, int n_tiles, const double2 *__restrict__ x_free, const double2 *__restrict__ x_fixed,
    const double2 *__restrict__ p, double2 *__restrict__ q, int64_t n_u, Tri3Consts k, DynMass dm,
    const double *__restrict__ coef, double *__restrict__ partials, unsigned *ticket, double *st, double *host, double *pq_out,
    int cap_nodes, int cap_owned) {
    if (st && st[hHalted] != 0.0) return;                   // uniform over the grid: nothing is written after a halt
    extern __shared__ double2 lds[];
    double2 *nd_xy = lds, *nd_pr = lds + cap_nodes, *nd_pi = lds + 2 * cap_nodes;
    double *acc = reinterpret_cast<double *>(lds + 3 * cap_nodes);
    double *red = acc + 4 * cap_owned;
    const int tid = threadIdx.x;
    const HarmCoef zc = load_coef(coef);
    const int slot = xcd_tile((int)blockIdx.x, (int)gridDim.x);
    mem_phase_begin();
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
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int l = tid + j * BLOCK;
        const double2 vx = *(s[j].x >= 0 ? x_free + s[j].x : x_fixed + ~s[j].x);
        double2 vr = make_double2(0.0, 0.0), vi = make_double2(0.0, 0.0);
        if (s[j].y >= 0) { vr = p[s[j].y]; vi = p[n_u + s[j].y]; }
        if (l < d.n_node) { nd_xy[l] = vx; nd_pr[l] = vr; nd_pi[l] = vi; }
        if (l < n_owned) { acc[l] = 0.0; acc[cap_owned + l] = 0.0; acc[2 * cap_owned + l] = 0.0; acc[3 * cap_owned + l] = 0.0; }
    }
#pragma unroll
    for (int j = 0; j < EPT; ++j)
        if (tid + j * BLOCK >= d.n_elem) { pk[j] = kSkipBit; pk3[j] = 0u; }
    __syncthreads();
    mem_phase_end();
    double er_loc = 0.0, ei_loc = 0.0;
#pragma unroll
    for (int jj = 0; jj < EPT; ++jj) {
        const uint32_t pw = pk[jj];
        if (!(pw & kSkipBit)) {
            const int l[4] = {(int)(pw & kLocalMask), (int)((pw >> kLocalBits) & kLocalMask),
                              (int)((pw >> (2 * kLocalBits)) & kLocalMask), (int)(pk3[jj] & kLocalMask)};
            const double2 o = make_double2(0.0, 0.0);
            double2 Xn[4], Rn[4], In[4], kr[4], ki[4], mr[4] = {o, o, o, o}, mi[4] = {o, o, o, o};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                Xn[j] = nd_xy[l[j]];
                Rn[j] = nd_pr[l[j]];
                In[j] = nd_pi[l[j]];
            }
            quad4_element_u<PHYS>(Xn, Rn, k, kr);
            quad4_element_u<PHYS>(Xn, In, k, ki);
            quad4_mass_rows(Xn, Rn, dm, mr);
            quad4_mass_rows(Xn, In, dm, mi);
            double er = 0.0, ei = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                double2 qr, qi;
                harm_combine(zc, kr[j], ki[j], mr[j], mi[j], Rn[j], In[j], qr, qi, er, ei);
                if (l[j] < n_owned) {
                    unsafeAtomicAdd(&acc[l[j]], qr.x);
                    unsafeAtomicAdd(&acc[cap_owned + l[j]], qr.y);
                    unsafeAtomicAdd(&acc[2 * cap_owned + l[j]], qi.x);
                    unsafeAtomicAdd(&acc[3 * cap_owned + l[j]], qi.y);
                }
            }
            if (pw & kHomeBit) { er_loc += er; ei_loc += ei; }
        }
    }
    wave_energy(er_loc, red);
    wave_energy(ei_loc, red + BLOCK / 64);
    __syncthreads();
    harm_store_q<BLOCK>(s, n_owned, acc, cap_owned, q, n_u);
    harm_apply_finish<BLOCK>(red, partials, slot, ticket, n_tiles, st, host, pq_out);
}

// ---------------------------------------------------------------- COCG vector kernels
// The inverses of the 2x2 blocks {a, b, c} of diag [n][3] (the identity for a block that is not positive definite): what
// store_jacobi_block keeps for the real driver.
__global__ __launch_bounds__(kHarmVecBlock) void harm_dinv_kernel(int64_t n, const double *__restrict__ diag,
                                                                  double *__restrict__ dinv) {
    for (int64_t i = (int64_t)blockIdx.x * kHarmVecBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kHarmVecBlock) {
        const double a = diag[3 * i], b = diag[3 * i + 1], c = diag[3 * i + 2];
        const double det = a * c - b * b;
        double o0 = 1.0, o1 = 0.0, o2 = 1.0;
        if (a > 0.0 && det > 0.0 && isfinite(det)) {
            const double inv = 1.0 / det;
            o0 = c * inv; o1 = -b * inv; o2 = a * inv;
        }
        dinv[3 * i] = o0; dinv[3 * i + 1] = o1; dinv[3 * i + 2] = o2;
    }
}

// Thread 0 of the last workgroup: beta = rho' / rho (0 on the first direction), rho <- rho'; true on a non-finite scalar.
__device__ __forceinline__ bool harm_rho_step(double *st, double nr, double ni) {
    double br = 0.0, bi = 0.0;
    if (st[hIter] != 0.0) {
        const double rr = st[hRhoRe], ri = st[hRhoIm];
        const double den = rr * rr + ri * ri;
        br = (nr * rr + ni * ri) / den;
        bi = (ni * rr - nr * ri) / den;
    }
    st[hBetaRe] = br; st[hBetaIm] = bi;
    st[hRhoRe] = nr; st[hRhoIm] = ni;
    return !isfinite(nr) || !isfinite(ni) || !isfinite(br) || !isfinite(bi);
}

// PRE: 0 none (z = r), 1 block Jacobi (z = D^-1 r on both planes), 2 AMG (the update without z: the V-cycles and harm_rz_kernel
// follow).  START: r = b - q0 (q0 = A x0; NULL: r = b), the reset of the record; otherwise x += alpha p, r -= alpha q.
// Then |r|_2 (Hermitian), rho' = r^T z (unconjugated; PRE != 2), beta, and the halt decision: breakdown before a met tolerance
// before max_iter.  n rows; plane 1 of every vector starts n rows after plane 0.
template <bool START, int PRE>
__global__ __launch_bounds__(kHarmVecBlock) void harm_vec_kernel(
    int64_t n, double2 *__restrict__ x, double2 *__restrict__ r, double2 *__restrict__ z, const double2 *__restrict__ p,
    const double2 *__restrict__ q, const double *__restrict__ dinv, const double2 *__restrict__ b, double *__restrict__ part,
    unsigned *ticket, double *st, double *host, double rtol, double atol, double max_iter) {
    __shared__ double red[kHarmVecBlock / 64 + 1];
    const int tid = threadIdx.x;
    const int nb = (int)gridDim.x;
    if (!START && st[hHalted] != 0.0) return;
    double ar = 0.0, ai = 0.0;
    if (!START) { ar = st[hAlphaRe]; ai = st[hAlphaIm]; }
    double zr = 0.0, zi = 0.0, rr = 0.0, bb = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kHarmVecBlock + tid; i < n; i += (int64_t)nb * kHarmVecBlock) {
        double2 r0, r1;
        if (START) {
            r0 = b[i]; r1 = b[n + i];
            bb += r0.x * r0.x + r0.y * r0.y + r1.x * r1.x + r1.y * r1.y;
            if (q) {
                const double2 q0 = q[i], q1 = q[n + i];
                r0.x -= q0.x; r0.y -= q0.y; r1.x -= q1.x; r1.y -= q1.y;
            }
        } else {
            const double2 p0 = p[i], p1 = p[n + i], q0 = q[i], q1 = q[n + i];
            double2 x0 = x[i], x1 = x[n + i];
            r0 = r[i]; r1 = r[n + i];
            x0.x += ar * p0.x - ai * p1.x; x0.y += ar * p0.y - ai * p1.y;
            x1.x += ar * p1.x + ai * p0.x; x1.y += ar * p1.y + ai * p0.y;
            r0.x -= ar * q0.x - ai * q1.x; r0.y -= ar * q0.y - ai * q1.y;
            r1.x -= ar * q1.x + ai * q0.x; r1.y -= ar * q1.y + ai * q0.y;
            x[i] = x0; x[n + i] = x1;
        }
        r[i] = r0; r[n + i] = r1;
        if constexpr (PRE != 2) {
            double2 z0 = r0, z1 = r1;
            if constexpr (PRE == 1) {
                const double d0 = dinv[3 * i], d1 = dinv[3 * i + 1], d2 = dinv[3 * i + 2];
                z0 = make_double2(d0 * r0.x + d1 * r0.y, d1 * r0.x + d2 * r0.y);
                z1 = make_double2(d0 * r1.x + d1 * r1.y, d1 * r1.x + d2 * r1.y);
            }
            z[i] = z0; z[n + i] = z1;
            zr += r0.x * z0.x + r0.y * z0.y - r1.x * z1.x - r1.y * z1.y;
            zi += r0.x * z1.x + r0.y * z1.y + r1.x * z0.x + r1.y * z0.y;
        }
        rr += r0.x * r0.x + r0.y * r0.y + r1.x * r1.x + r1.y * r1.y;
    }
    const double s_zr = block_sum(zr, red);
    __syncthreads();
    const double s_zi = block_sum(zi, red);
    __syncthreads();
    const double s_rr = block_sum(rr, red);
    __syncthreads();
    const double s_bb = block_sum(bb, red);
    if (tid == 0) {
        put_partial(part + blockIdx.x, s_zr);
        put_partial(part + nb + blockIdx.x, s_zi);
        put_partial(part + 2 * nb + blockIdx.x, s_rr);
        put_partial(part + 3 * nb + blockIdx.x, s_bb);
    }
    if (!last_block(ticket, (unsigned)nb, reinterpret_cast<int *>(red + kHarmVecBlock / 64))) return;
    const double rho_r = ordered_sum<kHarmVecBlock>(part, nb, red);
    const double rho_i = ordered_sum<kHarmVecBlock>(part + nb, nb, red);
    const double r2 = ordered_sum<kHarmVecBlock>(part + 2 * nb, nb, red);
    const double b2 = ordered_sum<kHarmVecBlock>(part + 3 * nb, nb, red);
    if (tid != 0) return;
    const double rnorm = sqrt(r2);
    int reason = kRunning;
    if (START) {
        for (int i = 0; i < kStatusN; ++i) st[i] = 0.0;
        st[hBnorm] = sqrt(b2);
        st[hTol] = fmax(rtol * st[hBnorm], atol);
        st[hMaxIter] = max_iter;
        st[hRtolWins] = rtol * st[hBnorm] >= atol ? 1.0 : 0.0;
    } else {
        st[hIter] += 1.0;
    }
    const bool bad = PRE != 2 && harm_rho_step(st, rho_r, rho_i);
    st[hRnorm] = rnorm;
    if (bad || !isfinite(rnorm)) reason = kBreakdown;
    else if (rnorm <= st[hTol]) reason = st[hRtolWins] != 0.0 ? kRtol : kAtol;
    else if (st[hIter] >= st[hMaxIter]) reason = kMaxIterHit;
    if (reason != kRunning) {
        st[hHalted] = 1.0;
        st[hReason] = reason;
    }
    publish(st, host);
}

// rho' = r^T z (unconjugated, both planes) in block order, then the rho step (PRE = AMG)
__global__ __launch_bounds__(kHarmVecBlock) void harm_rz_kernel(int64_t n, const double2 *__restrict__ r,
                                                                const double2 *__restrict__ z, double *__restrict__ part,
                                                                unsigned *ticket, double *st, double *host) {
    __shared__ double red[kHarmVecBlock / 64 + 1];
    const int tid = threadIdx.x;
    const int nb = (int)gridDim.x;
    if (st[hHalted] != 0.0) return;
    double zr = 0.0, zi = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kHarmVecBlock + tid; i < n; i += (int64_t)nb * kHarmVecBlock) {
        const double2 r0 = r[i], r1 = r[n + i], z0 = z[i], z1 = z[n + i];
        zr += r0.x * z0.x + r0.y * z0.y - r1.x * z1.x - r1.y * z1.y;
        zi += r0.x * z1.x + r0.y * z1.y + r1.x * z0.x + r1.y * z0.y;
    }
    const double s_zr = block_sum(zr, red);
    __syncthreads();
    const double s_zi = block_sum(zi, red);
    if (tid == 0) {
        put_partial(part + blockIdx.x, s_zr);
        put_partial(part + nb + blockIdx.x, s_zi);
    }
    if (!last_block(ticket, (unsigned)nb, reinterpret_cast<int *>(red + kHarmVecBlock / 64))) return;
    const double rho_r = ordered_sum<kHarmVecBlock>(part, nb, red);
    const double rho_i = ordered_sum<kHarmVecBlock>(part + nb, nb, red);
    if (tid != 0) return;
    if (harm_rho_step(st, rho_r, rho_i)) {
        st[hHalted] = 1.0;
        st[hReason] = kBreakdown;
    }
    publish(st, host);
}

// p = z + beta p (complex beta) on both planes; nothing once halted
__global__ __launch_bounds__(kHarmVecBlock) void harm_p_kernel(int64_t n, const double2 *__restrict__ z, double2 *__restrict__ p,
                                                               const double *st) {
    if (st[hHalted] != 0.0) return;
    const double br = st[hBetaRe], bi = st[hBetaIm];
    for (int64_t i = (int64_t)blockIdx.x * kHarmVecBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kHarmVecBlock) {
        const double2 z0 = z[i], z1 = z[n + i], p0 = p[i], p1 = p[n + i];
        p[i] = make_double2(z0.x + (br * p0.x - bi * p1.x), z0.y + (br * p0.y - bi * p1.y));
        p[n + i] = make_double2(z1.x + (br * p1.x + bi * p0.x), z1.y + (br * p1.y + bi * p0.y));
    }
}

}  // namespace
}  // namespace hfem

// ---------------------------------------------------------------- host side
struct hfem_harm {
    hfem_plan *plan = nullptr;
    int device = -1;
    int64_t n_u = 0;
    int n_tiles = 0, block = 256, vec_blocks = 1;
    bool phys = false, quad = false;
    size_t lds = 0;
    // device memory, one allocation: p, r, z, q (complex block vectors [2][n_u] double2), dinv (3 doubles per row), tile
    // partials [2][n_tiles], vector partials [4][blocks], coefficients, status record, tickets
    char *mem = nullptr;
    double2 *p = nullptr, *r = nullptr, *z = nullptr, *q = nullptr;
    double *dinv = nullptr, *tile_part = nullptr, *vec_part = nullptr, *coef = nullptr, *pq = nullptr, *st = nullptr;
    unsigned *tickets = nullptr;       // [0] apply, [1] vector kernels, [2] standalone apply
    double *host = nullptr;            // pinned mirror of the status record
    // bound by hfem_harm_setup
    const double2 *x_free = nullptr, *x_fixed = nullptr;
    hfem::Tri3Consts k{};
    hfem::DynMass dm{};
    bool ready = false;
    int pre = -1;                      // the preconditioner hfem_harm_start bound: 0 none, 1 block Jacobi, 2 AMG; -1 not started
};

namespace {
using namespace hfem;

// LDS bytes of the apply on a tile shape: 48 per local node, 32 per owned row, the reduction words
size_t harm_lds(int max_nodes, int max_owned, int block) {
    return (size_t)max_nodes * 48 + (size_t)max_owned * 32 + (size_t)(2 * (block / 64) + 2) * 8;
}

void harm_apply(const hfem_harm *c, const double2 *p, double2 *q, unsigned *ticket, double *st, double *host, double *pq_out,
                hipStream_t s) {
    const HostPlan &h = c->plan->host;
    const PlanDev pd = plan_dev(c->plan);
    if (c->quad) {
#define HFEM_Q4H(NPT, EPT, PH)                                                                                                \
    hipLaunchKernelGGL((quad4_harm_apply_kernel<256, NPT, EPT, PH>), dim3(c->n_tiles), dim3(256), c->lds, s, pd, c->n_tiles,  \
                       c->x_free, c->x_fixed, p, q, c->n_u, c->k, c->dm, c->coef, c->tile_part, ticket, st, host, pq_out,    \
                       h.max_nodes, h.max_owned)
        if (h.max_nodes <= 3 * 256 && h.max_elems <= 3 * 256) {
            if (c->phys) HFEM_Q4H(3, 3, true);
            else HFEM_Q4H(3, 3, false);
        } else {
            if (c->phys) HFEM_Q4H(4, 4, true);
            else HFEM_Q4H(4, 4, false);
        }
#undef HFEM_Q4H
        return;
    }
    // the tile shapes of launch_tri3_cg_apply
#define HFEM_T3H(BLOCK, NPT, EPT, PH)                                                                                         \
    hipLaunchKernelGGL((tri3_harm_apply_kernel<BLOCK, NPT, EPT, PH>), dim3(c->n_tiles), dim3(BLOCK), c->lds, s, pd,           \
                       c->n_tiles, c->x_free, c->x_fixed, p, q, c->n_u, c->k, c->dm, c->coef, c->tile_part, ticket, st, host, \
                       pq_out, h.max_nodes, h.max_owned, h.col_stride)
#define HFEM_T3H_A(BLOCK, NPT, EPT)                                                                                           \
    do {                                                                                                                      \
        if (c->phys) HFEM_T3H(BLOCK, NPT, EPT, true);                                                                         \
        else HFEM_T3H(BLOCK, NPT, EPT, false);                                                                                \
    } while (0)
    if (c->block == 512) HFEM_T3H_A(512, 2, 2);
    else if (h.max_nodes <= 3 * 256) {
        if (h.max_rows <= 3) HFEM_T3H_A(256, 3, 3);
        else if (h.max_rows == 4) HFEM_T3H_A(256, 3, 4);
        else HFEM_T3H_A(256, 3, 6);
    } else {
        if (h.max_rows <= 3) HFEM_T3H_A(256, 4, 3);
        else if (h.max_rows == 4) HFEM_T3H_A(256, 4, 4);
        else HFEM_T3H_A(256, 4, 6);
    }
#undef HFEM_T3H_A
#undef HFEM_T3H
}

// The vector update of an iteration (START: the start of a solve), with what follows it for the bound preconditioner.
template <bool START>
void harm_vec(const hfem_harm *c, const hfem_amg *amg, double2 *x, const double2 *q0, const double2 *b, double rtol, double atol,
              double max_iter, hipStream_t s) {
#define HFEM_HARM_VEC(PRE)                                                                                                    \
    hipLaunchKernelGGL((harm_vec_kernel<START, PRE>), dim3(c->vec_blocks), dim3(kHarmVecBlock), 0, s, c->n_u, x, c->r, c->z,  \
                       c->p, START ? q0 : c->q, c->dinv, b, c->vec_part, c->tickets + 1, c->st, c->host, rtol, atol, max_iter)
    if (c->pre == 0) HFEM_HARM_VEC(0);
    else if (c->pre == 1) HFEM_HARM_VEC(1);
    else {
        HFEM_HARM_VEC(2);
        amg_cycle(amg, (const double *)c->r, (double *)c->z, c->st, s);
        amg_cycle(amg, (const double *)(c->r + c->n_u), (double *)(c->z + c->n_u), c->st, s);
        hipLaunchKernelGGL(harm_rz_kernel, dim3(c->vec_blocks), dim3(kHarmVecBlock), 0, s, c->n_u, c->r, c->z, c->vec_part,
                           c->tickets + 1, c->st, c->host);
    }
#undef HFEM_HARM_VEC
    hipLaunchKernelGGL(harm_p_kernel, dim3(c->vec_blocks), dim3(kHarmVecBlock), 0, s, c->n_u, c->z, c->p, c->st);
}

int harm_check_amg(const hfem_harm *c, const hfem_amg *a, const char *who) {
    const char *msg = nullptr;
    if (!amg_ready(a)) msg = "hfem_amg_setup / hfem_amg_set_coarse have not run";
    else if (amg_rows(a) != c->n_u) msg = "the AMG hierarchy and the solver have different free rows";
    else if (amg_device(a) != c->device) msg = "the AMG hierarchy lives on another device";
    if (msg) {
        set_error(std::string(who) + ": " + msg);
        return -1;
    }
    return 0;
}

// len: the doubles of one complex block vector [2][n_u][2]
bool harm_len_ok(int64_t len) { return len >= 0 && (len & 3) == 0; }
const char *kLenMsg = "len must be a multiple of 4 and >= 0 (a complex block vector [2][n_u][2])";
const char *kLenRows = "len is not 4 n_u of hfem_harm_create";
}  // namespace

extern "C" int hfem_harm_create(hfem_plan *plan, int64_t n_u, int32_t flags, hfem_harm **out) {
    HFEM_ARG_CHECK(plan && out, "null pointer");
    *out = nullptr;
    HFEM_ARG_CHECK(plan->device >= 0, "host-only plan (created with device < 0) cannot launch");
    const hfem::HostPlan &h = plan->host;
    const bool quad = h.npe == 4;
    HFEM_ARG_CHECK(quad || (h.paired && plan->d_elem_pack_hi && h.n_chained == 0),
                   "the harmonic apply needs a paired-slot TRI3 plan (plan_elem_order 5) or a QUAD4 plan; the one-element-per-slot "
                   "plan of the Neo-Hookean tangent is refused");
    HFEM_ARG_CHECK(!quad || plan->d_elem_pack_hi, "QUAD4 plan without its fourth-corner records");
    HFEM_ARG_CHECK((flags & ~HFEM_FLAG_PHYSICAL_GRAD) == 0, "flags: only HFEM_FLAG_PHYSICAL_GRAD");
    const bool b512 = !quad && h.pair_block == 512;
    HFEM_ARG_CHECK(quad    ? (h.max_nodes <= 4 * 256 && h.max_elems <= 4 * 256)
                   : b512 ? (h.max_nodes <= 2 * 512 && h.max_rows <= 2)
                          : (h.max_nodes <= 4 * 256 && h.max_rows <= 6),
                   "tile shape outside the apply kernels' instances");
    HFEM_ARG_CHECK(h.max_owned <= h.max_nodes, "plan owns more rows than a tile holds");
    const int block = b512 ? 512 : 256;
    const size_t lds = harm_lds(h.max_nodes, h.max_owned, block);
    if (lds > 64 * 1024) {
        hfem::set_error("hfem_harm_create: tile needs more than 64 KiB of LDS: 48 x " + std::to_string(h.max_nodes) +
                        " local nodes + 32 x " + std::to_string(h.max_owned) + " owned rows + " +
                        std::to_string((2 * (block / 64) + 2) * 8) + " = " + std::to_string(lds) + " bytes > 65536");
        return -1;
    }
    int64_t rows = 0;
    for (size_t i = 1; i < h.node_src.size(); i += 2) rows = std::max<int64_t>(rows, (int64_t)h.node_src[i] + 1);
    HFEM_ARG_CHECK(n_u >= rows, "n_u is smaller than the plan's free u rows");
    HFEM_ARG_CHECK(n_u < ((int64_t)1 << 30), "n_u too large");
    std::unique_ptr<hfem_harm> c(new hfem_harm);
    c->plan = plan; c->device = plan->device; c->n_u = n_u; c->phys = (flags & HFEM_FLAG_PHYSICAL_GRAD) != 0; c->quad = quad;
    c->n_tiles = (int)h.tiles.size(); c->block = block; c->lds = lds;
    c->vec_blocks = (int)std::max<int64_t>(1, std::min<int64_t>(hfem::kHarmVecMaxBlocks,
                                                                (n_u + hfem::kHarmVecBlock - 1) / hfem::kHarmVecBlock));
    if (int rc = hfem::use_device(c->device)) return rc;
    const size_t vec32 = (size_t)std::max<int64_t>(n_u, 1) * 32;      // one complex block vector
    const size_t off_d = 4 * vec32;
    const size_t off_tp = off_d + (size_t)std::max<int64_t>(n_u, 1) * 24;
    const size_t off_vp = off_tp + 2 * (size_t)std::max(c->n_tiles, 1) * 8;
    const size_t off_cf = off_vp + 4 * (size_t)hfem::kHarmVecMaxBlocks * 8;
    const size_t off_pq = off_cf + 4 * 8;
    const size_t off_st = off_pq + 2 * 8;
    const size_t off_tk = off_st + hfem::kStatusN * 8;
    const size_t bytes = off_tk + 64;
    HFEM_HIP_CHECK(hipMalloc((void **)&c->mem, bytes));
    if (hipHostMalloc((void **)&c->host, hfem::kStatusN * sizeof(double)) != hipSuccess) {
        (void)hipFree(c->mem);
        hfem::set_error("hfem_harm_create: hipHostMalloc failed");
        return 1;
    }
    for (int i = 0; i < hfem::kStatusN; ++i) c->host[i] = 0.0;
    c->p = (double2 *)c->mem; c->r = (double2 *)(c->mem + vec32); c->z = (double2 *)(c->mem + 2 * vec32);
    c->q = (double2 *)(c->mem + 3 * vec32);
    c->dinv = (double *)(c->mem + off_d); c->tile_part = (double *)(c->mem + off_tp); c->vec_part = (double *)(c->mem + off_vp);
    c->coef = (double *)(c->mem + off_cf); c->pq = (double *)(c->mem + off_pq); c->st = (double *)(c->mem + off_st);
    c->tickets = (unsigned *)(c->mem + off_tk);
    const hipError_t e = hipMemset(c->mem, 0, bytes);                 // tickets zero
    if (e != hipSuccess) {
        (void)hipFree(c->mem); (void)hipHostFree(c->host);
        hfem::set_error(std::string("hfem_harm_create: hipMemset -> ") + hipGetErrorString(e));
        return (int)e;
    }
    *out = c.release();
    return 0;
}

extern "C" int hfem_harm_destroy(hfem_harm *c) {
    if (!c) return 0;
    if (c->device >= 0) (void)hipSetDevice(c->device);
    if (c->mem) (void)hipFree(c->mem);
    if (c->host) (void)hipHostFree(c->host);
    delete c;
    return 0;
}

extern "C" int hfem_harm_setup(hfem_harm *c, const double *x_free, const double *x_fixed, const double mat[4], double W,
                               const double zk[2], const double zm[2], int32_t lumped, void *stream) {
    HFEM_ARG_CHECK(zk && zm, "null pointer");
    HFEM_ARG_CHECK(std::isfinite(zk[0]) && std::isfinite(zk[1]) && std::isfinite(zm[0]) && std::isfinite(zm[1]) &&
                       (zk[0] != 0.0 || zk[1] != 0.0 || zm[0] != 0.0 || zm[1] != 0.0),
                   "z_k and z_m must be finite and not all zero");
    HFEM_ARG_CHECK(c && x_free && mat, "null pointer");
    bool fixed_rows = false;
    const hfem::HostPlan &h = c->plan->host;
    for (size_t i = 0; i < h.node_src.size(); i += 2) fixed_rows = fixed_rows || h.node_src[i] < 0;
    HFEM_ARG_CHECK(x_fixed || !fixed_rows, "the plan reads fixed coordinate rows: x_fixed must be given");
    if (int rc = hfem::use_device(c->device)) return rc;
    c->x_free = (const double2 *)x_free; c->x_fixed = (const double2 *)x_fixed;
    c->k = hfem::make_consts(mat, c->quad ? 1.0 : W, nullptr);        // QUAD4: the 2x2 rule's weights are 1
    c->dm = hfem::dyn_mass(c->quad, 1.0, lumped != 0);
    hipLaunchKernelGGL(hfem::harm_set_coef_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, c->coef, zk[0], zk[1], zm[0], zm[1]);
    if (int rc = hfem::launch_status("hfem_harm_setup")) return rc;
    c->ready = true;
    return 0;
}

extern "C" int hfem_harm_apply(hfem_harm *c, const double *p, double *q, int64_t len, double *pq_out, void *stream) {
    HFEM_ARG_CHECK(harm_len_ok(len), kLenMsg);
    HFEM_ARG_CHECK(c && p && q && pq_out, "null pointer");
    HFEM_ARG_CHECK(p != q, "q must not alias p");
    HFEM_ARG_CHECK(c->ready, "hfem_harm_setup has not run");
    HFEM_ARG_CHECK(len == 4 * c->n_u, kLenRows);
    if (int rc = hfem::use_device(c->device)) return rc;
    harm_apply(c, (const double2 *)p, (double2 *)q, c->tickets + 2, nullptr, nullptr, pq_out, (hipStream_t)stream);
    return hfem::launch_status("hfem_harm_apply");
}

extern "C" int hfem_harm_start(hfem_harm *c, hfem_amg *amg, const double *diag, const double *b, const double *x0, int64_t len,
                               double rtol, double atol, int64_t max_iter, void *stream) {
    HFEM_ARG_CHECK(harm_len_ok(len), kLenMsg);
    HFEM_ARG_CHECK(rtol >= 0.0 && atol >= 0.0 && max_iter >= 0, "rtol, atol and max_iter must be >= 0");
    HFEM_ARG_CHECK(c && b, "null pointer");
    HFEM_ARG_CHECK(!(amg && diag), "one preconditioner: the AMG hierarchy or the diagonal blocks, not both");
    HFEM_ARG_CHECK(c->ready, "hfem_harm_setup has not run");
    HFEM_ARG_CHECK(len == 4 * c->n_u, kLenRows);
    if (amg)
        if (int rc = harm_check_amg(c, amg, __func__)) return rc;
    if (int rc = hfem::use_device(c->device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    c->pre = amg ? 2 : diag ? 1 : 0;
    HFEM_HIP_CHECK(hipMemsetAsync(c->p, 0, (size_t)std::max<int64_t>(c->n_u, 1) * 32, s));   // p_old of the first direction
    if (diag)
        hipLaunchKernelGGL(hfem::harm_dinv_kernel, dim3(c->vec_blocks), dim3(hfem::kHarmVecBlock), 0, s, c->n_u, diag, c->dinv);
    if (x0) harm_apply(c, (const double2 *)x0, c->q, c->tickets + 2, nullptr, nullptr, c->pq, s);
    harm_vec<true>(c, amg, nullptr, x0 ? c->q : nullptr, (const double2 *)b, rtol, atol, (double)max_iter, s);
    return hfem::launch_status("hfem_harm_start");
}

extern "C" int hfem_harm_iterate(hfem_harm *c, hfem_amg *amg, double *x, int64_t len, int32_t n_iter, void *stream) {
    HFEM_ARG_CHECK(harm_len_ok(len), kLenMsg);
    HFEM_ARG_CHECK(n_iter > 0, "n_iter must be > 0");
    HFEM_ARG_CHECK(c && (x || c->n_u == 0), "null pointer");
    HFEM_ARG_CHECK(c->ready && c->pre >= 0, "hfem_harm_start has not run");
    HFEM_ARG_CHECK(len == 4 * c->n_u, kLenRows);
    HFEM_ARG_CHECK((c->pre == 2) == (amg != nullptr), "amg: the hierarchy hfem_harm_start was given, NULL when it was given none");
    if (amg)
        if (int rc = harm_check_amg(c, amg, __func__)) return rc;
    if (int rc = hfem::use_device(c->device)) return rc;
    hipStream_t s = (hipStream_t)stream;
    for (int it = 0; it < n_iter; ++it) {                    // launch-only: capturable in one graph
        harm_apply(c, c->p, c->q, c->tickets, c->st, c->host, nullptr, s);
        harm_vec<false>(c, amg, (double2 *)x, nullptr, nullptr, 0.0, 0.0, 0.0, s);
    }
    return hfem::launch_status("hfem_harm_iterate");
}

extern "C" int hfem_harm_status(hfem_harm *c, double *status_host, void *stream) {
    HFEM_ARG_CHECK(c && status_host, "null pointer");
    if (int rc = hfem::use_device(c->device)) return rc;
    HFEM_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    for (int i = 0; i < hfem::kStatusN; ++i) status_host[i] = c->host[i];
    return 0;
}
