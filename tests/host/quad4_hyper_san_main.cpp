// Host-only sanitizer harness for the Neo-Hookean QUAD4 element and its finishing reduction (csrc/hfem_quad4_hyper_dev.h and
// hfem_hyper_dev.h: the text the kernels of csrc/quad4_hyper.hip compile), one loop iteration per device thread.
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I hip_stub \
//         -I ../../hidenn_fem_amd/csrc quad4_hyper_san_main.cpp -o quad4_hyper_san && ./quad4_hyper_san case.bin
// case.bin (tests/test_quad4_hyper_reference_host.py writes it from tests/quad4_hyper_reference.py), little endian:
//     int64 ne, nn, tile;  double lambda, mu, Bq[8];  int32 conn[ne][4];  double X[nn][2], U[nn][2];
//     expected: double e[ne], J[ne][4], gX[ne][4][2], gU[ne][4][2], loss, min_J, count
// `tile` consecutive cells play one tile of the plan (its three partials).  Exit status 0 = every number within 1e-12 of the
// expectation (relative to the largest entry of its array; inf must match inf).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <vector>

#include "hfem_quad4_hyper_dev.h"

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

template <bool HASB>
static double cell(const std::vector<int32_t> &conn, const std::vector<double> &X, const std::vector<double> &U, int64_t i,
                   const Quad4HyperConsts &k, double2 (&gx)[4], double2 (&gu)[4], double &jmin, bool &inv, double *jq) {
    double2 Xn[4], Un[4];
    for (int a = 0; a < 4; ++a) {
        const int n = conn[4 * i + a];
        Xn[a] = make_double2(X[2 * n], X[2 * n + 1]);
        Un[a] = make_double2(U[2 * n], U[2 * n + 1]);
    }
    return quad4_neo_hookean_element<HASB>(Xn, Un, k, gx, gu, jmin, inv, jq);
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t hdr[3];
    double c[10];
    if (!rd(f, hdr, 3) || !rd(f, c, 10)) return 2;
    const int64_t ne = hdr[0], nn = hdr[1], tile = hdr[2];
    std::vector<int32_t> conn(4 * ne);
    std::vector<double> X(2 * nn), U(2 * nn), e(ne), J(4 * ne), gX(8 * ne), gU(8 * ne), tot(3);
    if (!rd(f, conn.data(), conn.size()) || !rd(f, X.data(), X.size()) || !rd(f, U.data(), U.size()) || !rd(f, e.data(), e.size()) ||
        !rd(f, J.data(), J.size()) || !rd(f, gX.data(), gX.size()) || !rd(f, gU.data(), gU.size()) || !rd(f, tot.data(), 3))
        return 2;
    std::fclose(f);
    Quad4HyperConsts k;
    k.lambda = c[0]; k.mu = c[1];
    bool hasb = false;
    for (int q = 0; q < 4; ++q) {
        k.b[q] = make_double2(c[2 + 2 * q], c[3 + 2 * q]);
        hasb = hasb || k.b[q].x != 0.0 || k.b[q].y != 0.0;
    }

    // ---- the slot loop, one iteration per thread; tile partials as the kernel forms them
    const int n_tiles = (int)((ne + tile - 1) / tile);
    std::vector<double> ge(ne), gJ(4 * ne), ggX(8 * ne), ggU(8 * ne), work(3 * (size_t)n_tiles);
    for (int t = 0; t < n_tiles; ++t) { work[t] = 0.0; work[n_tiles + t] = INFINITY; work[2 * n_tiles + t] = 0.0; }
    for (int64_t i = 0; i < ne; ++i) {
        double2 gx[4], gu[4];
        double jmin, jq[4];
        bool inv;
        ge[i] = hasb ? cell<true>(conn, X, U, i, k, gx, gu, jmin, inv, jq) : cell<false>(conn, X, U, i, k, gx, gu, jmin, inv, jq);
        for (int a = 0; a < 4; ++a) {
            gJ[4 * i + a] = 1.0 + jq[a];
            ggX[8 * i + 2 * a] = gx[a].x; ggX[8 * i + 2 * a + 1] = gx[a].y;
            ggU[8 * i + 2 * a] = gu[a].x; ggU[8 * i + 2 * a + 1] = gu[a].y;
        }
        const int t = (int)(i / tile);
        work[t] += ge[i];
        work[n_tiles + t] = std::fmin(work[n_tiles + t], 1.0 + jmin);
        work[2 * n_tiles + t] += inv ? 1.0 : 0.0;
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
    std::printf("%lld cells, %d tiles, body %d: loss %.17g min J %.17g inverted %.0f -- %s\n", (long long)ne, n_tiles, (int)hasb,
                loss, min_j, count, bad ? "MISMATCH" : "ok");
    return bad ? 1 : 0;
}
