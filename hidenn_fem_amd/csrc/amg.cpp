// Smoothed-aggregation AMG, host setup (no GPU): the fine 2x2 block pattern of K_ff with the node -> element fan that the
// assembly kernel walks (npe corners per element: 3 for TRI3, 4 for QUAD4, whose diagonal partners are neighbours too), the aggregation of every level (SA phases 1-3, no strength filter, singletons merged), and the
// symbolic products P = pattern(A) pattern(P_tent), R = P^T (explicit transpose map), A P and A_c = R (A P).  Everything here
// depends on the connectivity, the Dirichlet mask and the u row map only; the numeric setup (tri3_amg.hip) redoes the values
// whenever the coordinates move.  Rows of every pattern are sorted, so a numeric kernel finds its output slot by binary search.
#include <algorithm>
#include <chrono>
#include <memory>
#include <new>
#include <string>

#include "hfem_amg.h"

namespace {
using hfem::AmgLevel;

// C = pattern(A) pattern(B); A: n rows, B: columns < k.  Rows of C sorted.
void pattern_product(int32_t n, int32_t k, const std::vector<int32_t> &a_ptr, const std::vector<int32_t> &a_col,
                     const std::vector<int32_t> &b_ptr, const std::vector<int32_t> &b_col, std::vector<int32_t> &c_ptr,
                     std::vector<int32_t> &c_col) {
    std::vector<int32_t> mark((size_t)std::max(k, 1), -1), row;
    c_ptr.assign((size_t)n + 1, 0);
    c_col.clear();
    for (int32_t i = 0; i < n; ++i) {
        row.clear();
        for (int32_t s = a_ptr[i]; s < a_ptr[i + 1]; ++s) {
            const int32_t j = a_col[s];
            for (int32_t t = b_ptr[j]; t < b_ptr[j + 1]; ++t) {
                const int32_t c = b_col[t];
                if (mark[c] != i) { mark[c] = i; row.push_back(c); }
            }
        }
        std::sort(row.begin(), row.end());
        c_col.insert(c_col.end(), row.begin(), row.end());
        c_ptr[i + 1] = (int32_t)c_col.size();
    }
}

// Transpose of an n-row pattern with k columns: rows ascending within each column, t_idx = index of the entry in the source.
void transpose(int32_t n, int32_t k, const std::vector<int32_t> &ptr, const std::vector<int32_t> &col, std::vector<int32_t> &t_ptr,
               std::vector<int32_t> &t_col, std::vector<int32_t> &t_idx) {
    t_ptr.assign((size_t)k + 1, 0);
    for (int32_t c : col) ++t_ptr[c + 1];
    for (int32_t c = 0; c < k; ++c) t_ptr[c + 1] += t_ptr[c];
    std::vector<int32_t> fill(t_ptr.begin(), t_ptr.end() - 1);
    t_col.assign(col.size(), 0);
    t_idx.assign(col.size(), 0);
    for (int32_t i = 0; i < n; ++i)
        for (int32_t s = ptr[i]; s < ptr[i + 1]; ++s) {
            const int32_t d = fill[col[s]]++;
            t_col[d] = i;
            t_idx[d] = s;
        }
}

// Standard SA aggregation on the graph (ptr, col; the diagonal may be present): phase 1 roots whose whole distance-1
// neighbourhood is free, phase 2 attaches to a phase-1 neighbour's aggregate (first in column order), phase 3 aggregates
// the leftovers with their still-free neighbours; then a singleton with a neighbour joins the first neighbour's aggregate.
// Aggregates are renumbered in order of their first root.  Deterministic.
int32_t aggregate(int32_t n, const std::vector<int32_t> &ptr, const std::vector<int32_t> &col, std::vector<int32_t> &agg) {
    agg.assign((size_t)n, -1);
    int32_t na = 0;
    for (int32_t i = 0; i < n; ++i) {
        if (agg[i] != -1) continue;
        bool free = true;
        for (int32_t s = ptr[i]; s < ptr[i + 1] && free; ++s) free = agg[col[s]] == -1;
        if (!free) continue;
        agg[i] = na;
        for (int32_t s = ptr[i]; s < ptr[i + 1]; ++s) agg[col[s]] = na;
        ++na;
    }
    const std::vector<int32_t> phase1 = agg;
    for (int32_t i = 0; i < n; ++i) {
        if (agg[i] != -1) continue;
        for (int32_t s = ptr[i]; s < ptr[i + 1]; ++s)
            if (phase1[col[s]] != -1) { agg[i] = phase1[col[s]]; break; }
    }
    for (int32_t i = 0; i < n; ++i) {
        if (agg[i] != -1) continue;
        agg[i] = na;
        for (int32_t s = ptr[i]; s < ptr[i + 1]; ++s)
            if (agg[col[s]] == -1) agg[col[s]] = na;
        ++na;
    }
    std::vector<int32_t> size((size_t)na, 0);
    for (int32_t i = 0; i < n; ++i) ++size[agg[i]];
    for (int32_t i = 0; i < n; ++i) {
        if (size[agg[i]] != 1) continue;
        for (int32_t s = ptr[i]; s < ptr[i + 1]; ++s)
            if (agg[col[s]] != agg[i]) {
                size[agg[i]] = 0;
                agg[i] = agg[col[s]];
                ++size[agg[i]];
                break;
            }
    }
    std::vector<int32_t> remap((size_t)na, -1);
    int32_t m = 0;
    for (int32_t i = 0; i < n; ++i)
        if (remap[agg[i]] == -1) remap[agg[i]] = m++;
    for (int32_t i = 0; i < n; ++i) agg[i] = remap[agg[i]];
    return m;
}

// Aggregation and symbolic products of level L (its A pattern set); fills the next level's A pattern.  Returns false when the
// level does not shrink.
bool coarsen(AmgLevel &L, AmgLevel &next) {
    L.n_agg = aggregate(L.n, L.a_ptr, L.a_col, L.agg);
    if (L.n_agg >= L.n) return false;
    std::vector<int32_t> t_ptr((size_t)L.n + 1), t_col(L.agg);     // P_tent: one block per row
    for (int32_t i = 0; i <= L.n; ++i) t_ptr[i] = i;
    std::vector<int32_t> tmp;
    transpose(L.n, L.n_agg, t_ptr, t_col, L.agg_ptr, L.agg_rows, tmp);
    pattern_product(L.n, L.n_agg, L.a_ptr, L.a_col, t_ptr, t_col, L.p_ptr, L.p_col);
    transpose(L.n, L.n_agg, L.p_ptr, L.p_col, L.r_ptr, L.r_col, L.r_pidx);
    pattern_product(L.n, L.n_agg, L.a_ptr, L.a_col, L.p_ptr, L.p_col, L.ap_ptr, L.ap_col);
    next.n = L.n_agg;
    next.bs = 3;
    pattern_product(L.n_agg, L.n_agg, L.r_ptr, L.r_col, L.ap_ptr, L.ap_col, next.a_ptr, next.a_col);
    return true;
}

void diag_slots(AmgLevel &L) {
    L.a_diag.assign((size_t)L.n, -1);
    for (int32_t i = 0; i < L.n; ++i) {
        const auto b = L.a_col.begin() + L.a_ptr[i], e = L.a_col.begin() + L.a_ptr[i + 1];
        const auto it = std::lower_bound(b, e, i);
        L.a_diag[i] = (it != e && *it == i) ? (int32_t)(it - L.a_col.begin()) : -1;
    }
}

int build(const int32_t *conn, int64_t ne, int npe, int64_t nn, const int32_t *x_src, const int32_t *u_src, hfem_amg_host &h) {
    h.ne = ne; h.nn = nn; h.npe = npe;
    int64_t n_u = 0;
    for (int64_t v = 0; v < nn; ++v) n_u += u_src[v] >= 0;
    if (n_u >= ((int64_t)1 << 30)) { hfem::set_error("hfem_amg_host_create: too many free rows"); return -1; }
    h.n_u = (int32_t)n_u;
    std::vector<int32_t> row_node((size_t)n_u, -1);
    for (int64_t v = 0; v < nn; ++v) {
        const int32_t r = u_src[v];
        if (r < 0) continue;
        if (r >= n_u || row_node[r] != -1) { hfem::set_error("hfem_amg_host_create: u_src is not a row map"); return -1; }
        row_node[r] = (int32_t)v;
    }
    h.row_x.resize((size_t)n_u);
    for (int32_t r = 0; r < n_u; ++r) h.row_x[r] = x_src[row_node[r]];
    h.conn_x.resize((size_t)ne * npe);
    h.conn_u.resize((size_t)ne * npe);
    for (int64_t e = 0; e < ne; ++e)
        for (int a = 0; a < npe; ++a) {
            const int32_t v = conn[npe * e + a];
            if (v < 0 || v >= nn) { hfem::set_error("hfem_amg_host_create: connectivity out of range"); return -1; }
            h.conn_x[npe * e + a] = x_src[v];
            h.conn_u[npe * e + a] = u_src[v];
        }
    // node -> element fan of every free row (element ascending)
    h.fan_ptr.assign((size_t)n_u + 1, 0);
    for (int64_t e = 0; e < ne; ++e)
        for (int a = 0; a < npe; ++a)
            if (u_src[conn[npe * e + a]] >= 0) ++h.fan_ptr[u_src[conn[npe * e + a]] + 1];
    for (int32_t r = 0; r < n_u; ++r) h.fan_ptr[r + 1] += h.fan_ptr[r];
    const size_t nf = (size_t)h.fan_ptr[n_u];
    h.fan_elem.resize(nf); h.fan_corner.resize(nf); h.fan_slot.resize((size_t)npe * nf);
    {
        std::vector<int32_t> fill(h.fan_ptr.begin(), h.fan_ptr.end() - 1);
        for (int64_t e = 0; e < ne; ++e)
            for (int a = 0; a < npe; ++a) {
                const int32_t r = u_src[conn[npe * e + a]];
                if (r < 0) continue;
                const int32_t f = fill[r]++;
                h.fan_elem[f] = (int32_t)e;
                h.fan_corner[f] = a;
            }
    }
    // fine block pattern: the diagonal plus every free row sharing an element
    h.levels.clear();
    h.levels.emplace_back();
    AmgLevel &L0 = h.levels[0];
    L0.n = h.n_u; L0.bs = 2;
    L0.a_ptr.assign((size_t)n_u + 1, 0);
    std::vector<int32_t> row;
    for (int32_t r = 0; r < n_u; ++r) {
        row.assign(1, r);
        for (int32_t f = h.fan_ptr[r]; f < h.fan_ptr[r + 1]; ++f)
            for (int b = 0; b < npe; ++b) {
                const int32_t c = u_src[conn[npe * (int64_t)h.fan_elem[f] + b]];
                if (c >= 0) row.push_back(c);
            }
        std::sort(row.begin(), row.end());
        row.erase(std::unique(row.begin(), row.end()), row.end());
        L0.a_col.insert(L0.a_col.end(), row.begin(), row.end());
        L0.a_ptr[r + 1] = (int32_t)L0.a_col.size();
        for (int32_t f = h.fan_ptr[r]; f < h.fan_ptr[r + 1]; ++f)
            for (int b = 0; b < npe; ++b) {
                const int32_t c = u_src[conn[npe * (int64_t)h.fan_elem[f] + b]];
                h.fan_slot[(size_t)npe * f + b] =
                    c < 0 ? -1 : (int32_t)(std::lower_bound(L0.a_col.begin() + L0.a_ptr[r], L0.a_col.end(), c) - L0.a_col.begin());
            }
    }
    diag_slots(L0);
    // levels
    while ((int)h.levels.size() < hfem::kAmgMaxLevels) {
        AmgLevel &L = h.levels.back();
        if ((int64_t)L.n * L.bs <= hfem::kAmgMaxCoarseDofs) break;
        AmgLevel next;
        if (!coarsen(L, next)) {
            L.n_agg = 0;
            L.agg.clear(); L.agg_ptr.clear(); L.agg_rows.clear(); L.p_ptr.clear(); L.p_col.clear();
            L.r_ptr.clear(); L.r_col.clear(); L.r_pidx.clear(); L.ap_ptr.clear(); L.ap_col.clear();
            break;
        }
        diag_slots(next);
        h.levels.push_back(std::move(next));
    }
    return 0;
}

const std::vector<int32_t> *array_of(const hfem_amg_host *h, int32_t level, int32_t which) {
    if (level == -1) {
        switch (which) {
            case 0: return &h->fan_ptr;
            case 1: return &h->fan_elem;
            case 2: return &h->fan_corner;
            case 3: return &h->fan_slot;
            case 4: return &h->conn_u;
            default: return nullptr;
        }
    }
    const AmgLevel &L = h->levels[level];
    switch (which) {
        case 0: return &L.a_ptr;
        case 1: return &L.a_col;
        case 2: return &L.a_diag;
        case 3: return &L.agg;
        case 4: return &L.p_ptr;
        case 5: return &L.p_col;
        case 6: return &L.r_ptr;
        case 7: return &L.r_col;
        case 8: return &L.r_pidx;
        case 9: return &L.ap_ptr;
        case 10: return &L.ap_col;
        default: return nullptr;
    }
}
}  // namespace

extern "C" int hfem_amg_host_create(const int32_t *conn, int64_t ne, int64_t nn, const int32_t *x_src, const int32_t *u_src,
                                    hfem_amg_host **out) {
    return hfem_amg_host_create_ex(conn, ne, 3, nn, x_src, u_src, out);
}

extern "C" int hfem_amg_host_create_ex(const int32_t *conn, int64_t ne, int32_t npe, int64_t nn, const int32_t *x_src,
                                       const int32_t *u_src, hfem_amg_host **out) {
    HFEM_ARG_CHECK(out, "null pointer");
    *out = nullptr;
    HFEM_ARG_CHECK(x_src && u_src && (conn || ne == 0), "null pointer");
    HFEM_ARG_CHECK(npe == 3 || npe == 4, "npe: 3 (TRI3) or 4 (QUAD4)");
    HFEM_ARG_CHECK(ne >= 0 && nn > 0 && ne < ((int64_t)1 << 31) && nn < ((int64_t)1 << 31), "ne / nn out of range");
    const auto t0 = std::chrono::steady_clock::now();
    std::unique_ptr<hfem_amg_host> h(new (std::nothrow) hfem_amg_host);
    HFEM_ARG_CHECK(h != nullptr, "out of memory");
    try {
        if (build(conn, ne, npe, nn, x_src, u_src, *h)) return -1;
    } catch (const std::exception &e) {
        hfem::set_error(std::string("hfem_amg_host_create: ") + e.what());
        return -1;
    }
    HFEM_ARG_CHECK(h->n_u > 0, "no free u rows");
    h->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    *out = h.release();
    return 0;
}

extern "C" int hfem_amg_host_destroy(hfem_amg_host *h) {
    delete h;
    return 0;
}

extern "C" int hfem_amg_host_info(const hfem_amg_host *h, int32_t level, int64_t info[8]) {
    HFEM_ARG_CHECK(h && info, "null pointer");
    HFEM_ARG_CHECK(level >= -1 && level < (int32_t)h->levels.size(), "level out of range");
    for (int i = 0; i < 8; ++i) info[i] = 0;
    if (level < 0) {
        info[0] = (int64_t)h->levels.size();
        info[1] = h->n_u;
        info[2] = h->ne;
        info[3] = h->fan_ptr.back();
        info[4] = (int64_t)(h->seconds * 1e9);
        info[5] = h->npe;
        return 0;
    }
    const AmgLevel &L = h->levels[level];
    info[0] = L.n;
    info[1] = L.bs;
    info[2] = (int64_t)L.a_col.size();
    info[3] = L.n_agg;
    info[4] = (int64_t)L.p_col.size();
    info[5] = (int64_t)L.ap_col.size();
    return 0;
}

extern "C" int hfem_amg_host_copy(const hfem_amg_host *h, int32_t level, int32_t which, int32_t *out, int64_t *n_out) {
    HFEM_ARG_CHECK(h && n_out, "null pointer");
    HFEM_ARG_CHECK(level >= -1 && level < (int32_t)h->levels.size(), "level out of range");
    const std::vector<int32_t> *v = array_of(h, level, which);
    HFEM_ARG_CHECK(v != nullptr, "which out of range");
    *n_out = (int64_t)v->size();
    if (out) std::copy(v->begin(), v->end(), out);
    return 0;
}
