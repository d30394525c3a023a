// The frame of the mesh-validity kernels (mesh_guard.hip): one thread per element over the int32 connectivity
// (caller numbering), every kernel an instance of mesh_element_kernel<element description, operation, row type>.
//   rows        coordinate rows come through the x row map (x_src[n] >= 0: x_free row, < 0: x_fixed row -1 - x_src[n]) and
//               displacement rows through the u row map of the same convention, so any storage row order works.  Rows are
//               fp64 or fp32 (T); all arithmetic is fp64.
//   operation   declares the gathers it needs (kRef: reference rows x_ref by node id; kU: displacement rows; kDir: direction
//               rows d by x_free row, zero for a fixed row), names its reduction and turns the gathered rows of one element
//               into that reduction's partial, through the closed forms of the element description (hfem_mesh_elem_dev.h).
//   reduction   MinBound    min of a non-negative double by a 64-bit atomic min on its bit pattern (monotone);
//               Summary<K>  min of K doubles by monotone keys + the count of flagged elements by integer atomic add, between
//                           a one-thread init and a one-thread finish launch that turns the words into doubles;
//               Sum         fp64 sum by atomic add (with the per-node atomics of node_atomic_add: not deterministic in the
//                           last bits; the other two are order-independent, hence deterministic).
// Each launch that reduces into a caller scalar is preceded by a one-thread init launch on the same stream (the sentinel).
// Atomic filters: a workgroup reads the running minimum first and only issues its atomic when it improves on it, so the
// single-address atomics do not serialise the tail of a launch.  Gather-bound; no LDS beyond the reduction words, no per-thread
// array that survives unrolling (no scratch).  Everything has internal linkage.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "hfem_device.h"
#include "hfem_mesh_elem_dev.h"

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

// ---------------------------------------------------------------- the three reductions
// Each: the LDS word type, a thread's partial with its identity, and the workgroup step `reduce(partial, red, value, acc)`.
struct MinBound {
    typedef unsigned long long Word;
    struct Partial { double a = INFINITY; };
    // a >= 0 or +inf (a NaN from non-finite rows sorts above +inf): the u64 order of the bits is the numeric order
    static __device__ __forceinline__ void reduce(const Partial &p, Word *red, double *, unsigned long long *alpha) {
        const unsigned long long k = block_min_u64((unsigned long long)__double_as_longlong(p.a), red);
        if (threadIdx.x == 0) atomic_min_filtered(alpha, k);
    }
};

// summary (as u64 words while the launch runs): {key(min) x K, count}
template <int K> struct Summary {
    static constexpr int kKeys = K;
    typedef unsigned long long Word;
    struct Partial {
        unsigned long long key[K];
        unsigned flagged = 0;
        __device__ __forceinline__ Partial() {
#pragma unroll
            for (int k = 0; k < K; ++k) key[k] = ~0ull;
        }
    };
    static __device__ __forceinline__ void reduce(const Partial &p, Word *red, double *, unsigned long long *summary) {
        unsigned long long b[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (k) __syncthreads();                              // thread 0 may still be reading the previous key's words
            b[k] = block_min_u64(p.key[k], red);
        }
        const unsigned long long n = (unsigned long long)__syncthreads_count(p.flagged);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) atomic_min_filtered(summary + k, b[k]);
            if (n) __hip_atomic_fetch_add(summary + K, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
};

struct Sum {
    typedef double Word;
    struct Partial { double v = 0.0; };
    static __device__ __forceinline__ void reduce(const Partial &p, Word *red, double *value, unsigned long long *) {
        const double tot = block_sum(p.v, red);
        if (threadIdx.x == 0 && value) __hip_atomic_fetch_add(value, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// The per-node part of Sum: g[k] onto row src[k] of grad [n_x][2], free rows only.
template <int N>
__device__ __forceinline__ void node_atomic_add(double *grad, const int32_t (&src)[N], const double2 (&g)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k)
        if (src[k] >= 0) {
            __hip_atomic_fetch_add(grad + 2 * (int64_t)src[k], g[k].x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(grad + 2 * (int64_t)src[k] + 1, g[k].y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
}

__global__ void step_bound_init_kernel(double *alpha) { alpha[0] = INFINITY; }

template <int K> __global__ void summary_init_kernel(unsigned long long *summary) {
#pragma unroll
    for (int k = 0; k < K; ++k) summary[k] = ~0ull;
    summary[K] = 0ull;
}

template <int K> __global__ void summary_finish_kernel(unsigned long long *summary) {
    double *out = reinterpret_cast<double *>(summary);
    double v[K + 1];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = dkey_value(summary[k]);
    v[K] = (double)summary[K];
#pragma unroll
    for (int k = 0; k <= K; ++k) out[k] = v[k];
}

// ---------------------------------------------------------------- the five operations
// The rows of one element; an operation reads only what it declared.  src: the x row map entries of its nodes.
template <int N> struct ElemRows {
    int32_t src[N];
    double2 X[N], R[N], U[N], D[N];
};

// element<E>(rows, param, e, out0, out1, partial): param = eta or the barrier's scale; out0 / out1 = the call's optional
// outputs (measure: q, ratio per element; deformation: J per element; barrier: the value and the gradient accumulators).
struct MeasureOp {                                               // q, ratio, inverted
    static constexpr bool kRef = true, kU = false, kDir = false;
    typedef Summary<2> Reduce;
    template <typename E>
    static __device__ __forceinline__ void element(const ElemRows<E::kNodes> &r, double, int64_t e, double *q_out,
                                                   double *ratio_out, Reduce::Partial &p) {
        double q, ratio;
        p.flagged = E::measure(r.X, r.R, q, ratio);
        if (q_out) q_out[e] = q;
        if (ratio_out) ratio_out[e] = ratio;
        p.key[0] = dkey(q);
        p.key[1] = dkey(ratio);
    }
};

struct StepBoundOp {                                             // the first a with detJ(x + a d) = eta detJ(x)
    static constexpr bool kRef = false, kU = false, kDir = true;
    typedef MinBound Reduce;
    template <typename E>
    static __device__ __forceinline__ void element(const ElemRows<E::kNodes> &r, double eta, int64_t, double *, double *,
                                                   Reduce::Partial &p) {
        p.a = E::reference_crossing(r.X, r.D, eta);
    }
};

struct BarrierOp {                                               // scale (1/q - 1) and its gradient
    static constexpr bool kRef = true, kU = false, kDir = false;
    typedef Sum Reduce;
    template <typename E>
    static __device__ __forceinline__ void element(const ElemRows<E::kNodes> &r, double scale, int64_t, double *, double *grad,
                                                   Reduce::Partial &p) {
        double2 g[E::kNodes];
        p.v = E::barrier(r.X, r.R, scale, grad != nullptr, g);
        if (grad) node_atomic_add(grad, r.src, g);
    }
};

struct HyperStepBoundOp {                                        // the smaller of the reference and the det F crossing
    static constexpr bool kRef = false, kU = true, kDir = true;
    typedef MinBound Reduce;
    template <typename E>
    static __device__ __forceinline__ void element(const ElemRows<E::kNodes> &r, double eta, int64_t, double *, double *,
                                                   Reduce::Partial &p) {
        double a_ref, a_def;
        E::hyper_crossings(r.X, r.U, r.D, eta, a_ref, a_def);
        p.a = smaller_crossing(a_ref, a_def);
    }
};

struct DeformationOp {                                           // J = det F, flagged: J <= 0 or NaN
    static constexpr bool kRef = false, kU = true, kDir = false;
    typedef Summary<1> Reduce;
    template <typename E>
    static __device__ __forceinline__ void element(const ElemRows<E::kNodes> &r, double, int64_t e, double *j_out, double *,
                                                   Reduce::Partial &p) {
        const double j = E::det_f(r.X, r.U);
        if (j_out) j_out[e] = j;
        p.key[0] = dkey(j);
        p.flagged = !(j > 0.0);
    }
};

// ---------------------------------------------------------------- the frame
// acc: the words the reduction's atomics land on (MinBound: alpha; Summary: the summary); Sum adds onto out0.
template <typename E, typename Op, typename T>
__global__ __launch_bounds__(kMeshBlock) void mesh_element_kernel(
    int64_t ne, const int32_t *__restrict__ conn, const int32_t *__restrict__ x_src,
    const typename MeshRow<T>::type *__restrict__ x_free, const typename MeshRow<T>::type *__restrict__ x_fixed,
    const typename MeshRow<T>::type *__restrict__ x_ref, const int32_t *__restrict__ u_src,
    const typename MeshRow<T>::type *__restrict__ u_free, const typename MeshRow<T>::type *__restrict__ u_fixed,
    const double2 *__restrict__ d, double param, double *out0, double *out1, unsigned long long *acc) {
    constexpr int N = E::kNodes;
    __shared__ typename Op::Reduce::Word red[kMeshBlock / 64];
    const int64_t e = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    typename Op::Reduce::Partial part;
    if (e < ne) {
        int32_t n[N];
        ElemRows<N> r;
#pragma unroll
        for (int k = 0; k < N; ++k) n[k] = conn[N * e + k];      // dword loads: the caller's pointer need not be 16-byte aligned
#pragma unroll
        for (int k = 0; k < N; ++k) r.src[k] = x_src[n[k]];
#pragma unroll
        for (int k = 0; k < N; ++k) r.X[k] = corner<T>(x_free, x_fixed, r.src[k]);
        if constexpr (Op::kRef) {
#pragma unroll
            for (int k = 0; k < N; ++k) {
                const typename MeshRow<T>::type v = x_ref[n[k]];
                r.R[k] = make_double2((double)v.x, (double)v.y);
            }
        }
        if constexpr (Op::kU) {
#pragma unroll
            for (int k = 0; k < N; ++k) r.U[k] = corner<T>(u_free, u_fixed, u_src[n[k]]);
        }
        if constexpr (Op::kDir) {
#pragma unroll
            for (int k = 0; k < N; ++k) r.D[k] = r.src[k] >= 0 ? d[r.src[k]] : make_double2(0.0, 0.0);
        }
        Op::template element<E>(r, param, e, out0, out1, part);
    }
    Op::Reduce::reduce(part, red, out0, acc);
}

inline unsigned mesh_blocks(int64_t ne) { return (unsigned)((ne + kMeshBlock - 1) / kMeshBlock); }

}  // namespace
}  // namespace hfem
