// What the mesh-validity kernels of the two element kinds share (tri3_mesh.hip, quad4_mesh.hip and their finite-strain
// siblings tri3_hyper_mesh.hip, quad4_hyper_mesh.hip): coordinate rows through the x row map, the monotone keys and the
// filtered atomic min of the deterministic reductions, the closed form of the step bound's first crossing
// (hfem_crossing_dev.h), and the one-thread init / finish launches around a reduction.  Everything has internal linkage:
// each translation unit carries its own instance.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "hfem_crossing_dev.h"
#include "hfem_device.h"

namespace hfem {
namespace {

constexpr int kMeshBlock = 256;

template <typename T> struct MeshRow;
template <> struct MeshRow<double> { typedef double2 type; };
template <> struct MeshRow<float> { typedef float2 type; };

template <typename T>
__device__ __forceinline__ double2 corner(const typename MeshRow<T>::type *__restrict__ x_free,
                                          const typename MeshRow<T>::type *__restrict__ x_fixed, int32_t src) {
    const typename MeshRow<T>::type v = src >= 0 ? x_free[src] : x_fixed[-1 - src];
    return make_double2((double)v.x, (double)v.y);
}

__device__ __forceinline__ double sign_of(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0); }

// Monotone key of a double: unsigned order of the key = numeric order of the value (NaN above +inf).
__device__ __forceinline__ unsigned long long dkey(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double dkey_value(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

// Workgroup min of a u64 (result in thread 0); `red` holds kMeshBlock / 64 words of LDS.
__device__ __forceinline__ unsigned long long block_min_u64(unsigned long long v, unsigned long long *red) {
    v = wave_min_u64(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kMeshBlock / 64; ++w) v = red[w] < v ? red[w] : v;
    return v;
}

__device__ __forceinline__ void atomic_min_filtered(unsigned long long *p, unsigned long long v) {
    if (v < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// summary (as u64 words while the measure runs): {key(min q), key(min ratio), inverted count}
__global__ void mesh_measure_init_kernel(unsigned long long *summary) {
    summary[0] = ~0ull;
    summary[1] = ~0ull;
    summary[2] = 0ull;
}

__global__ void mesh_measure_finish_kernel(unsigned long long *summary) {
    double *out = reinterpret_cast<double *>(summary);
    const double q = dkey_value(summary[0]), r = dkey_value(summary[1]);
    const double n = (double)summary[2];
    out[0] = q;
    out[1] = r;
    out[2] = n;
}

// Workgroup part of the measure's summary: min of the two keys, the count of inverted elements, one filtered atomic each.
__device__ __forceinline__ void mesh_measure_reduce(unsigned long long kq, unsigned long long kr, unsigned inv,
                                                    unsigned long long *red, unsigned long long *summary) {
    const unsigned long long bq = block_min_u64(kq, red);
    __syncthreads();
    const unsigned long long br = block_min_u64(kr, red);
    __syncthreads();
    const unsigned long long binv = (unsigned long long)__syncthreads_count(inv);
    if (threadIdx.x == 0) {
        atomic_min_filtered(summary, bq);
        atomic_min_filtered(summary + 1, br);
        if (binv) __hip_atomic_fetch_add(summary + 2, binv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// summary of the deformation measure (tri3_hyper_mesh.hip, quad4_hyper_mesh.hip; u64 words while it runs): {key(min J),
// count of elements with J <= 0 or NaN}
__global__ void deformation_measure_init_kernel(unsigned long long *summary) {
    summary[0] = ~0ull;
    summary[1] = 0ull;
}

__global__ void deformation_measure_finish_kernel(unsigned long long *summary) {
    double *out = reinterpret_cast<double *>(summary);
    const double j = dkey_value(summary[0]);
    const double n = (double)summary[1];
    out[0] = j;
    out[1] = n;
}

__device__ __forceinline__ void deformation_measure_reduce(unsigned long long kj, unsigned inv, unsigned long long *red,
                                                           unsigned long long *summary) {
    const unsigned long long bj = block_min_u64(kj, red);
    const unsigned long long binv = (unsigned long long)__syncthreads_count(inv);
    if (threadIdx.x == 0) {
        atomic_min_filtered(summary, bj);
        if (binv) __hip_atomic_fetch_add(summary + 1, binv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---------------------------------------------------------------- step bound (first_crossing(): hfem_crossing_dev.h)
__global__ void step_bound_init_kernel(double *alpha) { alpha[0] = INFINITY; }

inline unsigned mesh_blocks(int64_t ne) { return (unsigned)((ne + kMeshBlock - 1) / kMeshBlock); }

}  // namespace
}  // namespace hfem
