// Host-only sanitizer harness for the Neo-Hookean element and its finishing reduction (csrc/hfem_hyper_dev.h: the text
// the kernels of csrc/tri3_hyper.hip compile), one loop iteration per device thread.
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I hip_stub \
//         -I ../../hidenn_fem_amd/csrc hyper_san_main.cpp -o hyper_san && ./hyper_san case.bin
// case.bin (tests/test_hyper_reference_host.py writes it from tests/hyper_reference.py), little endian:
//     int64 ne, nn, tile;  double lambda, mu, W, Bk[6];  int32 conn[ne][3];  double X[nn][2], U[nn][2];
//     expected: double e[ne], J[ne], gX[ne][3][2], gU[ne][3][2], loss, min_J, count
// `tile` consecutive elements play one tile of the plan (its three partials).  Exit status 0 = every number within 1e-12
// of the expectation (relative to the largest entry of its array; inf must match inf).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <vector>

#include "hfem_hyper_dev.h"

using namespace hfem;

template <typename T>
static bool rd(FILE *f, T *p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

static double amax(const std::vector<double> &v) {
    double m = 0.0;
    for (double x : v)
        if (std::isfinite(x) && std::fabs(x) > m) m = std::fabs(x);
    return m;
}

static int compare(const char *what, const std::vector<double> &got, const std::vector<double> &want) {
    const double tol = 1e-12 * amax(want);
    int bad = 0;
    for (size_t i = 0; i < want.size(); ++i) {
        const bool same = std::isfinite(want[i]) ? std::fabs(got[i] - want[i]) <= tol : got[i] == want[i];
        if (!same && bad++ < 5) std::fprintf(stderr, "%s[%zu]: got %.17g want %.17g\n", what, i, got[i], want[i]);
    }
    return bad;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t hdr[3];
    double c[9];
    if (!rd(f, hdr, 3) || !rd(f, c, 9)) return 2;
    const int64_t ne = hdr[0], nn = hdr[1], tile = hdr[2];
    std::vector<int32_t> conn(3 * ne);
    std::vector<double> X(2 * nn), U(2 * nn), e(ne), J(ne), gX(6 * ne), gU(6 * ne), tot(3);
    if (!rd(f, conn.data(), conn.size()) || !rd(f, X.data(), X.size()) || !rd(f, U.data(), U.size()) || !rd(f, e.data(), e.size()) ||
        !rd(f, J.data(), J.size()) || !rd(f, gX.data(), gX.size()) || !rd(f, gU.data(), gU.size()) || !rd(f, tot.data(), 3))
        return 2;
    std::fclose(f);
    HyperConsts k;
    k.lambda = c[0]; k.mu = c[1]; k.W = c[2];
    for (int i = 0; i < 6; ++i) k.Bk[i] = c[3 + i];

    // ---- the slot loop, one iteration per thread; tile partials as the kernel forms them
    const int n_tiles = (int)((ne + tile - 1) / tile);
    std::vector<double> ge(ne), gJ(ne), ggX(6 * ne), ggU(6 * ne), work(3 * (size_t)n_tiles);
    for (int t = 0; t < n_tiles; ++t) { work[t] = 0.0; work[n_tiles + t] = INFINITY; work[2 * n_tiles + t] = 0.0; }
    for (int64_t i = 0; i < ne; ++i) {
        auto row = [&](const std::vector<double> &a, int n) { return make_double2(a[2 * n], a[2 * n + 1]); };
        const int n0 = conn[3 * i], n1 = conn[3 * i + 1], n2 = conn[3 * i + 2];
        double2 gx[3], gu[3];
        double jm1;
        ge[i] = neo_hookean_element(row(X, n0), row(X, n1), row(X, n2), row(U, n0), row(U, n1), row(U, n2), k, gx, gu, jm1);
        gJ[i] = 1.0 + jm1;
        for (int a = 0; a < 3; ++a) {
            ggX[6 * i + 2 * a] = gx[a].x; ggX[6 * i + 2 * a + 1] = gx[a].y;
            ggU[6 * i + 2 * a] = gu[a].x; ggU[6 * i + 2 * a + 1] = gu[a].y;
        }
        const int t = (int)(i / tile);
        work[t] += ge[i];
        work[n_tiles + t] = std::fmin(work[n_tiles + t], gJ[i]);
        work[2 * n_tiles + t] += jm1 > -1.0 ? 0.0 : 1.0;
    }
    int bad = compare("e", ge, e) + compare("J", gJ, J) + compare("gX", ggX, gX) + compare("gU", ggU, gU);

    // ---- the finishing launch: 256 threads, then the shuffle tree of every wave and the wave order
    const int nthr = 256;
    std::vector<double> te(nthr), tj(nthr), tc(nthr);
    for (int tid = 0; tid < nthr; ++tid) hyper_finish_thread(work.data(), n_tiles, tid, nthr, te[tid], tj[tid], tc[tid]);
    double loss = 0.0, min_j = INFINITY, count = 0.0;
    for (int w = 0; w < nthr / 64; ++w) {
        for (int off = 32; off > 0; off >>= 1)
            for (int l = 0; l < off; ++l) {                       // lane l reads lane l + off (lanes >= off no longer matter)
                te[64 * w + l] += te[64 * w + l + off];
                tj[64 * w + l] = std::fmin(tj[64 * w + l], tj[64 * w + l + off]);
                tc[64 * w + l] += tc[64 * w + l + off];
            }
        loss += te[64 * w]; min_j = std::fmin(min_j, tj[64 * w]); count += tc[64 * w];
    }
    bad += compare("loss", {loss}, {tot[0]}) + compare("min_J", {min_j}, {tot[1]}) + compare("count", {count}, {tot[2]});
    std::printf("%lld elements, %d tiles: loss %.17g min J %.17g inverted %.0f -- %s\n", (long long)ne, n_tiles, loss, min_j,
                count, bad ? "MISMATCH" : "ok");
    return bad ? 1 : 0;
}
