// Host-only sanitizer harness for the assembly of the Neo-Hookean tangent (csrc/hfem_amg_hyper_dev.h: amg_hyper_row, the
// text amg_assemble_hyper_kernel of csrc/tri3_amg.hip compiles), one loop iteration per device thread.  Every buffer has
// exactly the size the pattern gives it, so a read or write outside a row's fan or blocks is an AddressSanitizer report.
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I hip_stub \
//         -I ../../hidenn_fem_amd/csrc amg_hyper_san_main.cpp -o amg_hyper_san && ./amg_hyper_san case.bin
// case.bin (tests/test_tangent_amg_host.py writes it from the host hierarchy and tests/tangent_amg_reference.py), little endian:
//     int64 ne, npe, n_u, nnz, nfan, n_xfree, n_xfixed, n_ufixed;  double lambda, mu, W;
//     int32 conn_x[ne][npe], conn_u[ne][npe], fan_ptr[n_u + 1], fan_elem[nfan], fan_corner[nfan], fan_slot[nfan][npe],
//           a_ptr[n_u + 1];
//     double x_free[n_xfree][2], x_fixed[n_xfixed][2], u_free[n_u][2], u_fixed[n_ufixed][2];
//     expected: double a_val[nnz][2][2]
// Exit status 0 = every block entry within 1e-12 of the expectation (relative to the largest entry).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <vector>

#include "hfem_amg_hyper_dev.h"

using namespace hfem;

template <typename T>
static bool rd(FILE *f, std::vector<T> &v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

template <int NPE>
static void run(int64_t n_u, const std::vector<int32_t> &fan_ptr, const std::vector<int32_t> &fan_elem,
                const std::vector<int32_t> &fan_corner, const std::vector<int32_t> &fan_slot, const std::vector<int32_t> &conn_x,
                const std::vector<int32_t> &conn_u, const std::vector<double> &xf, const std::vector<double> &xfix,
                const std::vector<double> &uf, const std::vector<double> &ufix, const std::vector<int32_t> &a_ptr,
                std::vector<double> &a_val, const double c[3]) {
    for (int64_t r = 0; r < n_u; ++r)
        amg_hyper_row<NPE>((int32_t)r, fan_ptr.data(), fan_elem.data(), fan_corner.data(), fan_slot.data(), conn_x.data(),
                           conn_u.data(), (const double2 *)xf.data(), (const double2 *)xfix.data(), (const double2 *)uf.data(),
                           (const double2 *)ufix.data(), a_ptr.data(), a_val.data(), c[0], c[1], c[2]);
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t h[8];
    double c[3];
    if (fread(h, sizeof(int64_t), 8, f) != 8 || fread(c, sizeof(double), 3, f) != 3) return 2;
    const int64_t ne = h[0], npe = h[1], n_u = h[2], nnz = h[3], nfan = h[4];
    if (npe != 3 && npe != 4) return 2;
    std::vector<int32_t> conn_x(ne * npe), conn_u(ne * npe), fan_ptr(n_u + 1), fan_elem(nfan), fan_corner(nfan),
        fan_slot(nfan * npe), a_ptr(n_u + 1);
    std::vector<double> xf(2 * h[5]), xfix(2 * h[6]), uf(2 * n_u), ufix(2 * h[7]), want(4 * nnz);
    if (!rd(f, conn_x) || !rd(f, conn_u) || !rd(f, fan_ptr) || !rd(f, fan_elem) || !rd(f, fan_corner) || !rd(f, fan_slot) ||
        !rd(f, a_ptr) || !rd(f, xf) || !rd(f, xfix) || !rd(f, uf) || !rd(f, ufix) || !rd(f, want))
        return 2;
    std::fclose(f);
    std::vector<double> got(4 * nnz, -1.0);                  // not zero: the row loop has to clear its blocks itself
    if (npe == 3) run<3>(n_u, fan_ptr, fan_elem, fan_corner, fan_slot, conn_x, conn_u, xf, xfix, uf, ufix, a_ptr, got, c);
    else run<4>(n_u, fan_ptr, fan_elem, fan_corner, fan_slot, conn_x, conn_u, xf, xfix, uf, ufix, a_ptr, got, c);
    double top = 0.0;
    for (double v : want) top = std::fabs(v) > top ? std::fabs(v) : top;
    int bad = 0;
    int64_t dropped = 0;
    for (int32_t s : fan_slot) dropped += s < 0;
    for (size_t i = 0; i < want.size(); ++i)
        if (!(std::fabs(got[i] - want[i]) <= 1e-12 * top) && bad++ < 5)
            std::fprintf(stderr, "a_val[%zu]: got %.17g want %.17g\n", i, got[i], want[i]);
    std::printf("%lld rows, %lld blocks, %lld Dirichlet columns dropped -- %s\n", (long long)n_u, (long long)nnz, (long long)dropped,
                bad ? "MISMATCH" : "ok");
    return bad ? 1 : 0;
}
