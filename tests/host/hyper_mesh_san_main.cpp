// Host-only sanitizer harness for the finite-strain mesh guard's closed forms (csrc/hfem_hyper_mesh_dev.h with
// csrc/hfem_crossing_dev.h: the text the kernels of csrc/tri3_hyper_mesh.hip and csrc/quad4_hyper_mesh.hip compile), one
// loop iteration per device thread.
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I hip_stub \
//         -I ../../hidenn_fem_amd/csrc hyper_mesh_san_main.cpp -o hyper_mesh_san && ./hyper_mesh_san case.bin
// case.bin (tests/test_hyper_radapt_host.py writes it from its numpy closed forms), little endian:
//     int64 n3, n4;  double eta;
//     double X3[n3][3][2], U3[n3][3][2], D3[n3][3][2];  expected: double ref3[n3], def3[n3], J3[n3]
//     double X4[n4][4][2], U4[n4][4][2], D4[n4][4][2];  expected: double ref4[n4], def4[n4], J4[n4]
// ref / def: the element's reference crossing and det F crossing; J: det F (QUAD4: the smallest corner ratio).  Exit status 0 =
// every number within 1e-12 of its expectation, relative to that number (inf must match inf, 0 must be 0).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "hfem_hyper_mesh_dev.h"

using namespace hfem;

static bool rd(FILE *f, std::vector<double> &v) { return fread(v.data(), sizeof(double), v.size(), f) == v.size(); }

static int compare(const char *what, const std::vector<double> &got, const std::vector<double> &want) {
    int bad = 0;
    for (size_t i = 0; i < want.size(); ++i) {
        const bool same = std::isfinite(want[i]) ? std::fabs(got[i] - want[i]) <= 1e-12 * std::fabs(want[i]) : got[i] == want[i];
        if (!same && bad++ < 5) std::fprintf(stderr, "%s[%zu]: got %.17g want %.17g\n", what, i, got[i], want[i]);
    }
    return bad;
}

template <int N, typename Crossings, typename Measure>
static int run(FILE *f, int64_t n, double eta, const char *kind, Crossings crossings, Measure measure) {
    std::vector<double> X(2 * N * n), U(2 * N * n), D(2 * N * n), ref(n), def(n), J(n), gref(n), gdef(n), gJ(n);
    if (!rd(f, X) || !rd(f, U) || !rd(f, D) || !rd(f, ref) || !rd(f, def) || !rd(f, J)) return -1;
    for (int64_t e = 0; e < n; ++e) {
        double2 x[N], u[N], d[N];
        for (int k = 0; k < N; ++k) {
            const size_t o = 2 * (N * (size_t)e + k);
            x[k] = make_double2(X[o], X[o + 1]);
            u[k] = make_double2(U[o], U[o + 1]);
            d[k] = make_double2(D[o], D[o + 1]);
        }
        crossings(x, u, d, eta, gref[e], gdef[e]);
        gJ[e] = measure(x, u);
        if (smaller_crossing(gref[e], gdef[e]) != std::fmin(gref[e], gdef[e])) return -1;
    }
    const std::string k(kind);
    const int bad = compare((k + " ref").c_str(), gref, ref) + compare((k + " def").c_str(), gdef, def) +
                    compare((k + " J").c_str(), gJ, J);
    std::printf("%s: %lld elements -- %s\n", kind, (long long)n, bad ? "MISMATCH" : "ok");
    return bad;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t hdr[2];
    double eta;
    if (fread(hdr, sizeof(int64_t), 2, f) != 2 || fread(&eta, sizeof(double), 1, f) != 1) return 2;
    const int b3 = run<3>(
        f, hdr[0], eta, "TRI3",
        [](const double2 (&x)[3], const double2 (&u)[3], const double2 (&d)[3], double eta, double &r, double &s) {
            tri3_hyper_crossings(x, u, d, eta, r, s);
        },
        [](const double2 (&x)[3], const double2 (&u)[3]) { return tri3_det_f(x, u); });
    if (b3 < 0) return 2;
    const int b4 = run<4>(
        f, hdr[1], eta, "QUAD4",
        [](const double2 (&x)[4], const double2 (&u)[4], const double2 (&d)[4], double eta, double &r, double &s) {
            quad4_hyper_crossings(x, u, d, eta, r, s);
        },
        [](const double2 (&x)[4], const double2 (&u)[4]) { return quad4_corner_det_f(x, u); });
    if (b4 < 0) return 2;
    std::fclose(f);
    return (b3 || b4) ? 1 : 0;
}
