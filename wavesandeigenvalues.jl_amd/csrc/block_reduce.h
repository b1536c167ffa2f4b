// The first stage of every reduction over the rows of an interleaved multivector: the sum inside one workgroup.  Shared by vec.hip (the
// Krylov reductions), forced.hip (the observation functionals of a frequency sweep) and kernels.hip (the column norms of a prolonged
// result); nothing else belongs here.
#pragma once
#include "kernel_helpers.h"

__device__ __forceinline__ cplx vadd(cplx a, cplx b) { return cplx{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ double vadd(double a, double b) { return a + b; }
__device__ __forceinline__ cplx vshfl_xor(cplx a, int m) { return cplx{__shfl_xor(a.x, m), __shfl_xor(a.y, m)}; }
__device__ __forceinline__ double vshfl_xor(double a, int m) { return __shfl_xor(a, m); }
// First stage, inside a workgroup of NT threads in which thread t owns column t % nb: the sum of v over the threads of a column, returned
// to the threads tid < nb (the others get a value that means nothing).  EVERY thread of the workgroup calls it: idle threads (beyond
// R*nb, R = NT / nb) and threads of a masked chunk with v = 0.  sm: NT values of LDS scratch, free again on return (the closing barrier).
// POW2 (nb a power of two <= 64): the lanes of a wavefront that own the same column are reduced with xor shuffles, m = 32 ... nb, and only
// one value per wavefront and column goes through LDS; the NT/64 of them are added in index order.  Otherwise the R LDS entries of a
// column are added serially in index order (at nb = 1 that was 256 serial reads per vector: 168 us per launch in the narrow-batch
// solves of the Newton-type iterations).  The two orders give different bits: a kernel keeps the arm it has.
template <bool POW2, int NT, class T>
__device__ __forceinline__ T block_colsum(T v, int nb, T *sm) {
    const int tid = threadIdx.x;
    if (POW2) {
        for (int m = 32; m >= nb; m >>= 1) v = vadd(v, vshfl_xor(v, m));
        if ((tid & 63) < nb) sm[(tid >> 6) * nb + (tid & 63)] = v;
    } else {
        sm[tid] = v;
    }
    __syncthreads();
    if (tid < nb) {
        const int terms = POW2 ? NT / 64 : NT / nb;
        v = sm[tid];
        for (int k = 1; k < terms; ++k) v = vadd(v, sm[k * nb + tid]);
    }
    __syncthreads();
    return v;
}
