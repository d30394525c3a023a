// Host stand-in for <hip/hip_runtime.h>: just enough for csrc/hfem_hyper_dev.h to compile as plain C++
// (tests/host/hyper_san_main.cpp).
#pragma once
#include <cmath>

#define __device__
#define __host__
#define __forceinline__ inline __attribute__((always_inline))

struct double2 {
    double x, y;
};
static inline double2 make_double2(double x, double y) { return double2{x, y}; }
