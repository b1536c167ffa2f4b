// One-line device helpers and launch arithmetic shared by kernels.hip (operator, transfer, dense level), vec.hip (vector kernels) and
// tall.hip (tall matrices).  Private to those files; nothing else belongs here.
#pragma once
#include <algorithm>
#include <mutex>
#include "wae_internal.h"

// ---------------------------------------------------------------------------------------------------
// complex helpers
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ cplx cmul(cplx a, cplx b) { return cplx{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ cplx cconj(cplx a) { return cplx{a.x, -a.y}; }
__device__ __forceinline__ void cfma(cplx &acc, cplx a, cplx b) {
    acc.x = fma(a.x, b.x, acc.x); acc.x = fma(-a.y, b.y, acc.x);
    acc.y = fma(a.x, b.y, acc.y); acc.y = fma(a.y, b.x, acc.y);
}
// streaming (non-temporal) read of a vector entry: the Krylov basis is read once per kernel and is far larger than any cache
// (1.1 % of a 1M-DoF pass, paired runs; the same hint on w and on the store of the update: nothing measurable)
typedef double dbl2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ cplx stream_load(const cplx *p) {
#ifndef WAE_NO_NT_GS
    const dbl2v v = __builtin_nontemporal_load((const dbl2v *)p);
    return cplx{v.x, v.y};
#else
    return *p;
#endif
}
__device__ __forceinline__ cplx cdiv(cplx a, cplx b) {
    double s = 1.0 / (b.x * b.x + b.y * b.y);
    return cplx{(a.x * b.x + a.y * b.y) * s, (a.y * b.x - a.x * b.y) * s};
}
// first chunk >= c of the batch's nch 8-column chunks that the mask keeps (no mask: c itself)
__device__ __forceinline__ int next_chunk(const unsigned char *cmask, int c, int nch) { while (c < nch && cmask && !cmask[c]) ++c; return c; }

// ---------------------------------------------------------------------------------------------------
// launch arithmetic
// ---------------------------------------------------------------------------------------------------
static inline unsigned grid_for(size_t total, unsigned cap = 4096) {
    size_t g = (total + 255) / 256;
    if (g < 1) g = 1;
    return (unsigned)(g > cap ? cap : g);
}
// Geometry of a row-streaming kernel on an interleaved multivector: thread t of nt owns column t % nb and every R-th row, R = nt / nb
// rows per workgroup (threads beyond R*nb idle), rpt rows per thread and step.  steps = ceil(n / (R * rpt)) grid strides cover the
// n rows; grid = min(steps, cap) workgroups.
struct RowGrid { int R; int64_t steps; unsigned grid; };
static inline RowGrid row_grid(int64_t n, int nb, int nt, int rpt, int64_t cap) {
    const int R = nt / nb;
    const int64_t per = (int64_t)R * rpt, steps = (n + per - 1) / per;
    return RowGrid{R, steps, (unsigned)std::min(steps, cap)};
}
// f(device) once per device, under a lock.  Opting a kernel in to more dynamic LDS than the default is a property of the function ON A
// DEVICE, and one process may drive several devices with a host thread each (mgpu.hip), so the "done" flags are kept per device and
// what f fills in (launch_spmv_tile: the CU count) is visible to every later caller on that device.  Returns the current device.
struct OncePerDevice { std::mutex mu; bool done[64] = {false}; };
template <class F> static inline int once_per_device(OncePerDevice &s, F &&f) {
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(s.mu);
    if (!s.done[dev & 63]) { f(dev); s.done[dev & 63] = true; }
    return dev;
}
