// Host-side helpers of the mesh entries (assemble.hip, assemble_p2.hip, assemble_herm.hip, bloch.hip, octosplit.hip, locate.hip): the range check of an index
// list, the launch grid, and the hipCUB calls with their temporary storage.  wae_guarded and the copies of Dev / DevBuf are in wae_internal.h.
#pragma once
#include <hipcub/hipcub.hpp>

#include <iterator>

#include "wae_internal.h"

// every entry of list[0..count) must lie in 0..bound-1
inline void check_indices(const int32_t *list, int64_t count, int64_t bound, const char *message) {
    for (int64_t i = 0; i < count; ++i)
        if (list[i] < 0 || list[i] >= bound) throw WaeError(WAE_ERR_INVALID, message);
}

inline void check_tets(const int32_t *tets, int64_t ntets, int64_t npoints) {
    check_indices(tets, ntets * 4, npoints, "tetrahedron refers to a point outside 0..npoints-1");
}
inline void check_tris(const int32_t *tris, int64_t ntris, int64_t npoints) {
    check_indices(tris, ntris * 3, npoints, "triangle refers to a point outside 0..npoints-1");
}

// blocks of 256 threads over n items, one item per thread, or at most `cap` blocks for a kernel that strides; never an empty grid
constexpr size_t GRID_STRIDE_CAP = 8192;
inline dim3 grid_for(size_t n, size_t cap = 0xffffffffu) { return dim3((unsigned)std::max<size_t>(1, std::min((n + 255) / 256, cap))); }

// key bits a radix sort has to look at: every value up to x fits them
inline int key_bits(unsigned long long x) {
    int b = 1;
    while (b < 64 && (x >> b)) ++b;
    return b;
}

// A hipCUB device call as call(void *tmp, size_t &bytes) -> hipError_t: with tmp == nullptr it only reports the temporary storage it needs.
// cub_run asks, makes `tmp` large enough and runs the call.  Calls that share one buffer: cub_reserve(tmp, a, b) first, one allocation for both.
template <class Call> size_t cub_bytes(Call &&call) {
    size_t bytes = 0;
    HIP_CHECK(call(nullptr, bytes));
    return std::max<size_t>(bytes, 1);
}
template <class... Calls> void cub_reserve(DevBuf<char> &tmp, Calls &&...calls) {
    size_t need = 1;
    ((need = std::max(need, cub_bytes(calls))), ...);
    tmp.reserve(need);
}
template <class Call> void cub_run(Call &&call, DevBuf<char> &tmp) {
    size_t bytes = cub_bytes(call);
    tmp.reserve(bytes);
    HIP_CHECK(call(tmp.p, bytes));
}
template <class Call> void cub_run(Call &&call) {
    DevBuf<char> tmp;
    cub_run(call, tmp);
}

template <class In, class Out> void exclusive_sum(In in, Out out, int n, DevBuf<char> &tmp) {
    cub_run([&](void *t, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(t, b, in, out, n); }, tmp);
}
// the sum of n device values, in hipCUB's fixed tree order, on the host
template <class In> typename std::iterator_traits<In>::value_type device_sum(In d, int n) {
    typedef typename std::iterator_traits<In>::value_type T;
    Dev<T> out(1);
    cub_run([&](void *t, size_t &b) { return hipcub::DeviceReduce::Sum(t, b, d, out.p, n); });
    T h = T();
    out.to_host(&h, 1);
    return h;
}

// flame volume = sum |det J| / 6 over the flame tetrahedra (Meshutils.jl:757-767), from their |det J| on the device; WaeError if it is not
// positive  (assemble.hip)
double flame_volume(const Dev<double> &adet, int64_t nflame);
// the distinct values of the nk keys in k0 (`bits` key bits), ascending, in ek (room for nk); returns how many, WaeError if hipCUB reports a
// count outside 1..nk.  k0 is left as it was.  (assemble_p2.hip)
int sorted_unique_keys(Dev<unsigned long long> &k0, int nk, int bits, Dev<unsigned long long> &ek);
