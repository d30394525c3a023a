// Host-only sanitizer harness for the mesh guard's per-element closed forms (csrc/hfem_mesh_elem_dev.h with
// csrc/hfem_crossing_dev.h: the text the kernels of csrc/mesh_guard.hip compile), one loop iteration per device thread.
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I hip_stub \
//         -I ../../hidenn_fem_amd/csrc hyper_mesh_san_main.cpp -o hyper_mesh_san && ./hyper_mesh_san case.bin
// case.bin (tests/test_hyper_radapt_host.py writes it from its numpy closed forms and CPU autograd), little endian:
//     int64 n3, n4;  double eta, weight;
//     double X3[n3][3][2], U3[n3][3][2], D3[n3][3][2];
//         expected: double ref3[n3], def3[n3], J3[n3], q3[n3], ratio3[n3], inv3[n3], Q3[n3], G3[n3][3][2]
//     double X4[n4][4][2], U4[n4][4][2], D4[n4][4][2];  expected: the same eight arrays for the cells
// ref / def: the element's reference crossing and det F crossing; J: det F (QUAD4: the smallest corner ratio).  q, ratio, inv
// (0 or 1): the measure of the rows X + U against the reference rows X.  Q, G: the element's barrier term at the rows X + U
// with the scale weight / (kBarrierTerms n) and its gradient per node.  Exit status 0 = every crossing, J, q and ratio within
// 1e-12 of its expectation, relative to that number (inf must match inf, 0 must be 0), every flag equal, every Q within 1e-11
// of |Q| + scale (the rounding of S / den before the 1 is taken off) and every G entry within 1e-11 of its element's largest.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "hfem_mesh_elem_dev.h"

using namespace hfem;

static bool rd(FILE *f, std::vector<double> &v) { return fread(v.data(), sizeof(double), v.size(), f) == v.size(); }

static int compare(const std::string &what, const std::vector<double> &got, const std::vector<double> &want) {
    int bad = 0;
    for (size_t i = 0; i < want.size(); ++i) {
        const bool same = std::isfinite(want[i]) ? std::fabs(got[i] - want[i]) <= 1e-12 * std::fabs(want[i]) : got[i] == want[i];
        if (!same && bad++ < 5) std::fprintf(stderr, "%s[%zu]: got %.17g want %.17g\n", what.c_str(), i, got[i], want[i]);
    }
    return bad;
}

// |got - want| <= 1e-11 (|scale[i / group]| + floor): the barrier's rule
static int compare_scaled(const std::string &what, const std::vector<double> &got, const std::vector<double> &want,
                          const std::vector<double> &scale, size_t group, double floor) {
    int bad = 0;
    for (size_t i = 0; i < want.size(); ++i)
        if (!(std::fabs(got[i] - want[i]) <= 1e-11 * (std::fabs(scale[i / group]) + floor)) && bad++ < 5)
            std::fprintf(stderr, "%s[%zu]: got %.17g want %.17g\n", what.c_str(), i, got[i], want[i]);
    return bad;
}

template <typename E> static int run(FILE *f, int64_t n, double eta, double weight, const char *kind) {
    constexpr int N = E::kNodes;
    std::vector<double> X(2 * N * n), U(2 * N * n), D(2 * N * n), ref(n), def(n), J(n), q(n), ratio(n), inv(n), Q(n), G(2 * N * n);
    std::vector<double> gref(n), gdef(n), gJ(n), gq(n), gratio(n), ginv(n), gQ(n), gQ0(n), gG(2 * N * n), gmax(n);
    if (!rd(f, X) || !rd(f, U) || !rd(f, D)) return -1;
    for (std::vector<double> *v : {&ref, &def, &J, &q, &ratio, &inv, &Q, &G})
        if (!rd(f, *v)) return -1;
    const double scale = weight / (E::kBarrierTerms * (double)n);
    for (int64_t e = 0; e < n; ++e) {
        double2 x[N], u[N], d[N], y[N], g[N], unused[N];
        for (int k = 0; k < N; ++k) {
            const size_t o = 2 * (N * (size_t)e + k);
            x[k] = make_double2(X[o], X[o + 1]);
            u[k] = make_double2(U[o], U[o + 1]);
            d[k] = make_double2(D[o], D[o + 1]);
            y[k] = add2(x[k], u[k]);
        }
        E::hyper_crossings(x, u, d, eta, gref[e], gdef[e]);
        gJ[e] = E::det_f(x, u);
        if (smaller_crossing(gref[e], gdef[e]) != std::fmin(gref[e], gdef[e])) return -1;
        // the reference crossing does not depend on u and is the small-strain bound's, to the bit
        double2 zero[N] = {};
        double a_ref0, a_def0;
        E::hyper_crossings(x, zero, d, eta, a_ref0, a_def0);
        if (a_ref0 != gref[e] || a_ref0 != E::reference_crossing(x, d, eta)) return -1;
        ginv[e] = E::measure(y, x, gq[e], gratio[e]) ? 1.0 : 0.0;
        gQ[e] = E::barrier(y, x, scale, true, g);
        gQ0[e] = E::barrier(y, x, scale, false, unused);       // the value alone: the gradient is not touched
        if (gQ0[e] != gQ[e]) return -1;
        for (int k = 0; k < N; ++k) {
            gG[2 * (N * (size_t)e + k)] = g[k].x;
            gG[2 * (N * (size_t)e + k) + 1] = g[k].y;
            gmax[e] = std::max({gmax[e], std::fabs(G[2 * (N * (size_t)e + k)]), std::fabs(G[2 * (N * (size_t)e + k) + 1])});
        }
    }
    const std::string k(kind);
    const int bad = compare(k + " ref", gref, ref) + compare(k + " def", gdef, def) + compare(k + " J", gJ, J) +
                    compare(k + " q", gq, q) + compare(k + " ratio", gratio, ratio) + compare(k + " inverted", ginv, inv) +
                    compare_scaled(k + " Q", gQ, Q, Q, 1, scale) + compare_scaled(k + " G", gG, G, gmax, 2 * N, 0.0);
    std::printf("%s: %lld elements -- %s\n", kind, (long long)n, bad ? "MISMATCH" : "ok");
    return bad;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t hdr[2];
    double par[2];
    if (fread(hdr, sizeof(int64_t), 2, f) != 2 || fread(par, sizeof(double), 2, f) != 2) return 2;
    const int b3 = run<Tri3>(f, hdr[0], par[0], par[1], "TRI3");
    if (b3 < 0) return 2;
    const int b4 = run<Quad4>(f, hdr[1], par[0], par[1], "QUAD4");
    if (b4 < 0) return 2;
    std::fclose(f);
    return (b3 || b4) ? 1 : 0;
}
