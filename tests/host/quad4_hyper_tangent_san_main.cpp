// Host-only sanitizer harness for the Neo-Hookean QUAD4 element tangent (csrc/hfem_quad4_hyper_dev.h:
// quad4_hyper_tangent_apply + quad4_hyper_tangent_blocks, the text the kernels of csrc/quad4_hyper_cg.hip compile), one loop
// iteration per device thread.
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I hip_stub \
//         -I ../../hidenn_fem_amd/csrc quad4_hyper_tangent_san_main.cpp -o quad4_hyper_tangent_san && ./quad4_hyper_tangent_san case.bin
// case.bin (tests/test_quad4_newton_reference_host.py writes it from tests/quad4_newton_reference.py), little endian:
//     int64 ne, nn;  double lambda, mu;  int32 conn[ne][4];  double X[nn][2], U[nn][2], P[nn][2];
//     expected: double q[ne][4][2] (K_e p_e), pq[ne] (p_e . q_e), J[ne][4], blocks[ne][4][3] ({K_xx, K_xy, K_yy} of every
//               corner), count
// Exit status 0 = every number within 1e-12 of the expectation (relative to the largest entry of its array), the apply's and
// the blocks' min J and inversion flags agree, the apply on the c_q the blocks return equals the apply that recomputes them
// bit for bit, and an inverted cell's outputs are exactly zero.
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

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t hdr[2];
    double c[2];
    if (!rd(f, hdr, 2) || !rd(f, c, 2)) return 2;
    const int64_t ne = hdr[0], nn = hdr[1];
    std::vector<int32_t> conn(4 * ne);
    std::vector<double> X(2 * nn), U(2 * nn), P(2 * nn), q(8 * ne), pq(ne), J(4 * ne), blocks(12 * ne), cnt(1);
    if (!rd(f, conn.data(), conn.size()) || !rd(f, X.data(), X.size()) || !rd(f, U.data(), U.size()) || !rd(f, P.data(), P.size()) ||
        !rd(f, q.data(), q.size()) || !rd(f, pq.data(), pq.size()) || !rd(f, J.data(), J.size()) ||
        !rd(f, blocks.data(), blocks.size()) || !rd(f, cnt.data(), 1))
        return 2;
    std::fclose(f);
    Quad4HyperConsts k{};
    k.lambda = c[0]; k.mu = c[1];

    std::vector<double> gq(8 * ne), gpq(ne), gJ(4 * ne), gblocks(12 * ne);
    double count = 0.0;
    int bad = 0;
    for (int64_t i = 0; i < ne; ++i) {
        double2 Xn[4], Un[4], Pn[4], qe[4];
        for (int a = 0; a < 4; ++a) {
            const int n = conn[4 * i + a];
            Xn[a] = make_double2(X[2 * n], X[2 * n + 1]);
            Un[a] = make_double2(U[2 * n], U[2 * n + 1]);
            Pn[a] = make_double2(P[2 * n], P[2 * n + 1]);
        }
        // the apply kernel's slot
        double jmin, jq[4];
        bool inv;
        gpq[i] = quad4_hyper_tangent_apply(Xn, Un, Pn, k, qe, jmin, inv, jq);
        double jm = INFINITY;
        for (int a = 0; a < 4; ++a) {
            gq[8 * i + 2 * a] = qe[a].x; gq[8 * i + 2 * a + 1] = qe[a].y;
            gJ[4 * i + a] = 1.0 + jq[a];
            jm = std::fmin(jm, jq[a]);
            if (inv && (qe[a].x != 0.0 || qe[a].y != 0.0)) ++bad;
        }
        count += inv ? 1.0 : 0.0;
        if (jm != jmin || inv != !(jm > -1.0)) {
            std::fprintf(stderr, "cell %lld: jmin %.17g against min_q j_q %.17g, inverted %d\n", (long long)i, jmin, jm, (int)inv);
            ++bad;
        }
        // the diag kernel's slot
        double blk[4][3], jmin_b, cq[4];
        bool inv_b;
        quad4_hyper_tangent_blocks(Xn, Un, k, blk, jmin_b, inv_b, cq);
        if (jmin_b != jmin || inv_b != inv) {
            std::fprintf(stderr, "cell %lld: the blocks' min j / flag differ from the apply's\n", (long long)i);
            ++bad;
        }
        // the apply kernel's slot as it runs behind a diag launch: c_q read, not recomputed -- the same numbers
        double2 qs[4];
        double jmin_s;
        bool inv_s;
        const double pq_s = quad4_hyper_tangent_apply(Xn, Un, Pn, k, qs, jmin_s, inv_s, nullptr, cq);
        bool same = pq_s == gpq[i] && jmin_s == jmin && inv_s == inv;
        for (int a = 0; a < 4; ++a) same = same && qs[a].x == qe[a].x && qs[a].y == qe[a].y;
        if (!same) {
            std::fprintf(stderr, "cell %lld: the apply on stored c differs from the apply that recomputes it\n", (long long)i);
            ++bad;
        }
        for (int a = 0; a < 4; ++a)
            for (int e = 0; e < 3; ++e) {
                gblocks[12 * i + 3 * a + e] = blk[a][e];
                if (inv && blk[a][e] != 0.0) ++bad;
            }
    }
    bad += compare("q", gq, q) + compare("pq", gpq, pq) + compare("J", gJ, J) + compare("blocks", gblocks, blocks);
    if (count != cnt[0]) {
        std::fprintf(stderr, "count: got %.0f want %.0f\n", count, cnt[0]);
        ++bad;
    }
    std::printf("%lld cells: inverted %.0f -- %s\n", (long long)ne, count, bad ? "MISMATCH" : "ok");
    return bad ? 1 : 0;
}
