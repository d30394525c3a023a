// Smoothed-aggregation AMG for the frozen-mesh solve (TRI3 and QUAD4): the host-side hierarchy (amg.cpp, no GPU), the CG
// status record, and the hooks the CG driver (cg.hip) uses to run the V-cycle of tri3_amg.hip inside its iteration.
#pragma once
#include <cstdint>
#include <vector>

#include "hfem_common.h"

namespace hfem {

constexpr int kAmgMaxCoarseDofs = 1500;   // coarsen until a level has at most this many dofs (or stops shrinking)
constexpr int kAmgMaxLevels = 12;
constexpr int kAmgPowerIters = 30;        // power iterations for lambda_max(D^-1 A) (15 left the estimate at 0.84 of it)

// One level of the hierarchy: block rows of size bs (2 on the fine level, 3 below), CSR patterns with sorted columns.
// Levels other than the coarsest also carry their aggregation and the symbolic products toward the next level.
struct AmgLevel {
    int32_t n = 0, bs = 2;
    std::vector<int32_t> a_ptr, a_col, a_diag;         // A (diagonal slot of each row)
    int32_t n_agg = 0;                                 // = next level's n
    std::vector<int32_t> agg, agg_ptr, agg_rows;       // aggregate of each row; members of each aggregate (ascending)
    std::vector<int32_t> p_ptr, p_col;                 // P = pattern(A) pattern(P_tent): columns are aggregates
    std::vector<int32_t> r_ptr, r_col, r_pidx;         // R = P^T: columns are fine rows, r_pidx = block index into P
    std::vector<int32_t> ap_ptr, ap_col;               // A P
};

}  // namespace hfem

// Host hierarchy: depends on the connectivity, the Dirichlet mask and the u row map only, never on coordinates.
struct hfem_amg_host {
    int64_t ne = 0, nn = 0;
    int32_t n_u = 0, npe = 3;                          // npe: corners per element, 3 (TRI3) or 4 (QUAD4)
    std::vector<int32_t> conn_x;                       // [ne][npe] x row code of every corner (x_src of the node)
    std::vector<int32_t> conn_u;                       // [ne][npe] u row code of every corner (u_src of the node: a free
                                                       // row index, or -1 - k for fixed row k)
    std::vector<int32_t> row_x;                        // [n_u] x row code of every free u row
    // node -> element fan of every free u row, fixed order (element id ascending); per entry: element, corner, and the
    // block slot of row (corner) that each of the npe corners' columns writes to (-1: a Dirichlet corner, dropped)
    std::vector<int32_t> fan_ptr, fan_elem, fan_corner, fan_slot;
    std::vector<hfem::AmgLevel> levels;
    double seconds = 0.0;
};

struct hfem_amg;   // device hierarchy (tri3_amg.hip)

namespace hfem {
// CG status record (device, and its pinned host mirror; hfem_cg_status): doubles
enum { kIter = 0, kRnorm, kFnorm, kRho, kReason, kAlpha, kBeta, kPq, kTol, kMaxIter, kHalted, kRtolWins, kStatusN = 16 };
enum { kRunning = 0, kRtol = 1, kAtol = 2, kMaxIterHit = 3, kBreakdown = 4 };   // st[kReason]
// Enqueue z = M r (one V-cycle) on `s`; every launch returns at once when st != nullptr and st[kHalted] != 0.
void amg_cycle(const hfem_amg *a, const double *r, double *z, const double *st, void *s);
int64_t amg_rows(const hfem_amg *a);
int amg_device(const hfem_amg *a);
bool amg_ready(const hfem_amg *a);
}  // namespace hfem
