// Host-only sanitizer harness for the finite-strain stress law and the per-element ZZ indicator
// (csrc/hfem_recover_hyper_dev.h: the text the kernels of csrc/recover.hip compile), one loop iteration per device thread.
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I hip_stub \
//         -I ../../hidenn_fem_amd/csrc hyper_recover_san_main.cpp -o hyper_recover_san && ./hyper_recover_san case.bin
// case.bin (tests/test_hyper_zz_reference_host.py writes it from tests/hyper_zz_reference.py), little endian:
//     int64 ne, nn, npe;  double lambda, mu;  int32 conn[ne][npe];  double X[nn][2], U[nn][2], nodal_stress[nn][3];
//     expected: double sigma[ne][nq][3] (NaN = not compared: the points of an inverted element), j[ne][nq], eta2[ne]
// with nq = 1 (npe 3) or 4 (npe 4).  Exit status 0 = every number within 1e-12 of the expectation (relative to the largest
// finite entry of its array; inf must match inf).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <vector>

#include "hfem_recover_hyper_dev.h"

using namespace hfem;

template <typename T>
static bool rd(FILE *f, T *p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

static int compare(const char *what, const std::vector<double> &got, const std::vector<double> &want) {
    double m = 0.0;
    for (double x : want)
        if (std::isfinite(x) && std::fabs(x) > m) m = std::fabs(x);
    const double tol = 1e-12 * m;
    int bad = 0;
    for (size_t i = 0; i < want.size(); ++i) {
        if (std::isnan(want[i])) continue;
        const bool same = std::isfinite(want[i]) ? std::fabs(got[i] - want[i]) <= tol : got[i] == want[i];
        if (!same && bad++ < 5) std::fprintf(stderr, "%s[%zu]: got %.17g want %.17g\n", what, i, got[i], want[i]);
    }
    for (double x : got)
        if (std::isnan(x)) { ++bad; std::fprintf(stderr, "%s: NaN computed\n", what); break; }
    return bad;
}

template <int NPE>
static int run(int64_t ne, const CauchyLaw &law, const std::vector<int32_t> &conn, const std::vector<double> &X,
               const std::vector<double> &U, const std::vector<double> &S, const std::vector<double> &sig,
               const std::vector<double> &jw, const std::vector<double> &eta2) {
    constexpr int NQ = RecPoints<NPE>::NQ;
    std::vector<double> gs(3 * NQ * ne), gj(NQ * ne), ge(ne);
    int inverted = 0;
    for (int64_t e = 0; e < ne; ++e) {
        double2 Xn[NPE], Un[NPE];
        Sig3 ss[NPE];
        for (int k = 0; k < NPE; ++k) {
            const int32_t n = conn[NPE * e + k];
            Xn[k] = make_double2(X[2 * n], X[2 * n + 1]);
            Un[k] = make_double2(U[2 * n], U[2 * n + 1]);
            ss[k] = Sig3{S[3 * n], S[3 * n + 1], S[3 * n + 2]};
        }
        Sig3 sg[NQ];
        double w[NQ], jq[NQ];
        const bool ok = element_points<NPE>(Xn, Un, law, sg, w, jq);
        for (int q = 0; q < NQ; ++q) {
            gs[3 * (NQ * e + q)] = sg[q].xx; gs[3 * (NQ * e + q) + 1] = sg[q].yy; gs[3 * (NQ * e + q) + 2] = sg[q].xy;
            gj[NQ * e + q] = jq[q];
        }
        double ve, vn, jmin;
        const bool ok2 = hyper_zz_element<NPE>(Xn, Un, ss, law, ve, vn, jmin);
        if (ok != ok2 || (!ok && vn != 0.0)) { std::fprintf(stderr, "element %lld: inconsistent inversion\n", (long long)e); return 1; }
        ge[e] = ve;
        inverted += ok ? 0 : 1;
    }
    const int bad = compare("sigma", gs, sig) + compare("j", gj, jw) + compare("eta2", ge, eta2);
    std::printf("%lld elements of %d nodes, %d inverted -- %s\n", (long long)ne, NPE, inverted, bad ? "MISMATCH" : "ok");
    return bad ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t hdr[3];
    double c[2];
    if (!rd(f, hdr, 3) || !rd(f, c, 2)) return 2;
    const int64_t ne = hdr[0], nn = hdr[1], npe = hdr[2];
    if (npe != 3 && npe != 4) return 2;
    const int64_t nq = npe == 3 ? 1 : 4;
    std::vector<int32_t> conn(npe * ne);
    std::vector<double> X(2 * nn), U(2 * nn), S(3 * nn), sig(3 * nq * ne), jw(nq * ne), eta2(ne);
    if (!rd(f, conn.data(), conn.size()) || !rd(f, X.data(), X.size()) || !rd(f, U.data(), U.size()) || !rd(f, S.data(), S.size()) ||
        !rd(f, sig.data(), sig.size()) || !rd(f, jw.data(), jw.size()) || !rd(f, eta2.data(), eta2.size()))
        return 2;
    std::fclose(f);
    const CauchyLaw law = cauchy_law(c[0], c[1]);
    return npe == 3 ? run<3>(ne, law, conn, X, U, S, sig, jw, eta2) : run<4>(ne, law, conn, X, U, S, sig, jw, eta2);
}
