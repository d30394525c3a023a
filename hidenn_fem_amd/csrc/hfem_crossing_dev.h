// The closed form every step bound shares: the first positive root of the quadratic a step bound solves (hfem_mesh_elem_dev.h:
// detJ(x + a d) = eta detJ(x), and at finite strain det F(a) = eta det F(0) as well).  A plain inline function, no wave
// intrinsics: a host program compiles it against tests/host/hip_stub.  Internal linkage, one instance per translation unit.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace hfem {
namespace {

// Smallest a > 0 with c + b a + a2 a^2 = 0, where c = (1 - eta) A0 > 0 after normalising by sign(A0) (+inf: none).  p(0) = c
// > 0, so a positive root exists iff b < 0 (then the smaller positive root is c / qq, qq = (-b + sqrt(disc)) / 2, stable for
// any a2 including 0 -- the linear case -c / b) or a2 < 0 (b >= 0: the positive root is qq / a2, qq = -(b + sqrt(disc)) / 2).
// disc < 0 (only with a2 > 0): p never reaches 0.  The double root (disc = 0) is returned: there detJ touches eta detJ(0).
__device__ __forceinline__ double first_crossing(double A0, double A1, double A2, double eta) {
    if (A0 == 0.0) return 0.0;                               // degenerate already: no step keeps a share of nothing
    const double sg = A0 > 0.0 ? 1.0 : -1.0;
    const double c = (1.0 - eta) * A0 * sg, b = A1 * sg, a2 = A2 * sg;
    const double disc = b * b - 4.0 * a2 * c;
    if (disc < 0.0) return INFINITY;
    const double sq = sqrt(disc);
    if (b < 0.0) return c / (0.5 * (sq - b));
    if (a2 < 0.0) return (-0.5 * (b + sq)) / a2;
    return INFINITY;
}

}  // namespace
}  // namespace hfem
