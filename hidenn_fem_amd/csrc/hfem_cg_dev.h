// Device-side pieces the frozen-mesh solve's element kernels share (tri3_cg.hip, quad4_cg.hip): the status publication, the
// last-workgroup hand-off and the fixed-order partial sum; and the launchers of the QUAD4 kernels, which the one PCG driver
// (tri3_cg.hip) and the AMG numeric setup (tri3_amg.hip) call for npe == 4.
#pragma once
#include <hip/hip_runtime.h>

#include "hfem_amg.h"
#include "hfem_device.h"
#include "hfem_plan_dev.h"

namespace hfem {

__device__ __forceinline__ void publish(const double *st, double *host) {
    if (host)
        for (int i = 0; i < kStatusN; ++i) host[i] = st[i];
}

// The last-workgroup hand-off (cdna_hip_programming.md section 6, Guideline 16, write-through form): every partial is stored
// with put_partial (agent-scope relaxed store: write-through, no release fence -- a release in every workgroup writes back its
// XCD's L2 under the running tiles), every wave drains its stores, lane 0 takes a relaxed agent-scope ticket; the workgroup
// that draws n - 1 is the reducer and reads the partials with agent-scope loads (get_partial).  `flag` is one word of the
// block's own LDS array.  Returns true in every thread of the last block.
__device__ __forceinline__ void put_partial(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double get_partial(const double *p) {
    return __hip_atomic_load(const_cast<double *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ bool last_block(unsigned *ticket, unsigned n, int *flag) {
    __builtin_amdgcn_s_waitcnt(0x0F70);                     // vmcnt(0): this wave's stores have been acknowledged
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = t == n - 1;
        if (last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
        *flag = last;
    }
    __syncthreads();
    return *flag != 0;
}

// Fixed-order sum of the n partials by one block (strided lanes, then block_sum's wave order).  Result in thread 0.
template <int BLOCK>
__device__ __forceinline__ double ordered_sum(const double *v, int n, double *red) {
    double a = 0.0;
    for (int i = threadIdx.x; i < n; i += BLOCK) a += get_partial(v + i);
    __syncthreads();                                        // red[] may still be read by the caller's earlier reduction
    return block_sum(a, red);
}

// ---------------------------------------------------------------- QUAD4 launchers (quad4_cg.hip)
// What the driver binds of a solve, by value: the model's own QUAD4 tile plan (one element per slot, no pairing).
struct Quad4CgArgs {
    const hfem_plan *plan = nullptr;
    int n_tiles = 0;
    bool phys = false;
    const double2 *x_free = nullptr, *x_fixed = nullptr;
    Tri3Consts k{};
    size_t lds = 0;
    hipStream_t s = nullptr;
};
// q = K p (the contract of tri3_cg_apply_kernel: st != NULL an iteration, st == NULL the standalone apply)
void launch_quad4_cg_apply(const Quad4CgArgs &A, const double2 *z, double2 *pbuf0, double2 *pbuf1, double2 *q, double *partials,
                           unsigned *ticket, double *st, double *host, double *pq_out);
// 2x2 diagonal blocks of K and their inverses (the layout and the identity fallback of tri3_cg_diag_kernel)
void launch_quad4_cg_diag(const Quad4CgArgs &A, double *diag, double *dinv, int precond);
// fine-level K_ff of the AMG hierarchy over a QUAD4 fan (four fan_slot entries per record)
void launch_quad4_amg_assemble(int32_t n, const int32_t *fan_ptr, const int32_t *fan_elem, const int32_t *fan_corner,
                               const int32_t *fan_slot, const int32_t *conn_x, const double2 *x_free, const double2 *x_fixed,
                               const int32_t *a_ptr, double *a_val, const Tri3Consts &k, bool phys, hipStream_t s);

}  // namespace hfem
