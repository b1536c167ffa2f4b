// Vector kernels of libwaehip.so on interleaved multivectors X[row][b] (layout: kernels.hip) -- gfx950 (MI355X, CDNA4; wave64) only:
// the Krylov streams and their reductions, the snapshot-basis helpers, the GMRES bookkeeping and the perturbation recurrence.
#include <type_traits>

#include "block_reduce.h"
#include "kernel_helpers.h"

// ---------------------------------------------------------------------------------------------------
// streaming vector kernels on interleaved multivectors
// ---------------------------------------------------------------------------------------------------
__global__ void fill_zero_kernel(cplx *X, size_t count) {
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < count; e += (size_t)gridDim.x * 256) X[e] = cplx{0.0, 0.0};
}
void launch_fill_zero(cplx *X, size_t count, hipStream_t st) {
    if (!count) return;
    hipLaunchKernelGGL(fill_zero_kernel, dim3(grid_for(count)), dim3(256), 0, st, X, count);
    HIP_CHECK(hipGetLastError());
}
void launch_copy(const cplx *X, cplx *Y, size_t count, hipStream_t st) {
    if (!count) return;
    HIP_CHECK(hipMemcpyAsync(Y, X, count * sizeof(cplx), hipMemcpyDeviceToDevice, st));
}
__global__ void add_kernel(const cplx *__restrict__ X, cplx *__restrict__ Y, size_t count) {
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < count; e += (size_t)gridDim.x * 256) {
        cplx a = X[e], b = Y[e];
        Y[e] = cplx{a.x + b.x, a.y + b.y};
    }
}
void launch_add(const cplx *X, cplx *Y, size_t count, hipStream_t st) {
    if (!count) return;
    hipLaunchKernelGGL(add_kernel, dim3(grid_for(count)), dim3(256), 0, st, X, Y, count);
    HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------------
// the two stages of every reduction over the rows (the first, block_colsum, is in block_reduce.h)
// ---------------------------------------------------------------------------------------------------
// Second stage: the sum over the nblk first-stage partials of output e = blockIdx.x * EPB + threadIdx.x % EPB, returned to the threads
// threadIdx.x < EPB (meaningful where e < count).  EPB outputs per workgroup, 256/EPB slices of the partials each, LDS tree over the
// slices: with 32 outputs per workgroup the norms of one batch (64 outputs, 768-1024 partials) ran on 2 workgroups, ~100
// dependent-latency loads per lane (31 us per call, 3.7 % of a pass).
template <int EPB>
__device__ __forceinline__ cplx sum_partials(const cplx *__restrict__ partial, int nblk, int count) {
    __shared__ cplx sm[256];
    constexpr int NS = 256 / EPB;
    const int slice = threadIdx.x / EPB;
    const int e = blockIdx.x * EPB + threadIdx.x % EPB;
    cplx acc = {0.0, 0.0};
    if (e < count)
        for (int k = slice; k < nblk; k += NS) { const cplx p = partial[(size_t)k * count + e]; acc.x += p.x; acc.y += p.y; }
    sm[threadIdx.x] = acc;
    __syncthreads();
#pragma unroll
    for (int s = NS / 2; s >= 1; s >>= 1) {
        if (slice < s) { sm[threadIdx.x].x += sm[threadIdx.x + s * EPB].x; sm[threadIdx.x].y += sm[threadIdx.x + s * EPB].y; }
        __syncthreads();
    }
    return sm[threadIdx.x];
}

// partial[blk][i][b] = sum over this block's rows of conj(V_i[row][b]) W[row][b];  any nb <= 256
// (thread t owns column t % nb and every R-th row, R = 256 / nb; threads beyond R*nb idle)
constexpr int DOT_BLOCKS = 1024;
template <int MAXV, bool POW2>
__global__ __launch_bounds__(256) void dots_kernel(const cplx *__restrict__ V, size_t stride, int nv, const cplx *__restrict__ W,
                                                   int64_t n, int nb, cplx *__restrict__ partial,
                                                   const unsigned char *__restrict__ cmask) {
    __shared__ cplx sm[256];
    const int tid = threadIdx.x;
    const int R = 256 / nb;
    const int b = tid % nb, rl = tid / nb;
    const bool live = rl < R && (!cmask || cmask[b >> 3]);
    cplx acc[MAXV];
#pragma unroll
    for (int i = 0; i < MAXV; ++i) acc[i] = cplx{0.0, 0.0};
    if (live) {
        for (int64_t row = (int64_t)blockIdx.x * R + rl; row < n; row += (int64_t)gridDim.x * R) {
            const size_t e = (size_t)row * nb + b;
            const cplx w = W[e];
#pragma unroll
            for (int i = 0; i < MAXV; ++i) {
                if (i < nv) {
                    const cplx v = stream_load(V + (size_t)i * stride + e);
                    acc[i].x += v.x * w.x + v.y * w.y;
                    acc[i].y += v.x * w.y - v.y * w.x;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        if (i < nv) {
            const cplx s = block_colsum<POW2, 256>(acc[i], nb, sm);
            if (tid < nb) partial[((size_t)blockIdx.x * nv + i) * nb + tid] = s;
        }
    }
}
// out[e] = sum_k partial[k][e], then scale, square root and inverse as asked for
template <int EPB>
__global__ __launch_bounds__(256) void reduce_partials_kernel(const cplx *__restrict__ partial, int nblk, int count, cplx *__restrict__ out, int do_sqrt,
                                                              const cplx *__restrict__ scale, cplx *__restrict__ inv_out) {
    cplx acc = sum_partials<EPB>(partial, nblk, count);
    const int e = blockIdx.x * EPB + threadIdx.x;
    if (threadIdx.x < EPB && e < count) {
        if (scale) { const double sc = scale[e].x; acc.x *= sc; acc.y *= sc; }        // dots against unnormalised vectors (lazy GMRES basis)
        if (do_sqrt) {
            if (inv_out) inv_out[e] = cplx{acc.x > 0.0 ? 1.0 / acc.x : 0.0, 0.0};     // 1/||.||^2 of the vector just measured
            acc = cplx{sqrt(acc.x), 0.0};
        }
        out[e] = acc;
    }
}
void launch_reduce_partials(const cplx *partial, int nblk, int count, cplx *out, int do_sqrt, hipStream_t st, const cplx *scale, cplx *inv_out) {
    if (count <= 256) hipLaunchKernelGGL(reduce_partials_kernel<2>, dim3((count + 1) / 2), dim3(256), 0, st, partial, nblk, count, out, do_sqrt, scale, inv_out);
    else hipLaunchKernelGGL(reduce_partials_kernel<8>, dim3((count + 7) / 8), dim3(256), 0, st, partial, nblk, count, out, do_sqrt, scale, inv_out);
    HIP_CHECK(hipGetLastError());
}

static void dots_impl(const cplx *V, size_t stride, int nv, const cplx *W, int64_t n, int nb, cplx *partial, cplx *out, int do_sqrt, hipStream_t st,
                      const unsigned char *cmask, const cplx *scale = nullptr) {
    if (nb < 1 || nb > 256) throw WaeError(WAE_ERR_INVALID, "dots: nb must be in 1..256");
    int done = 0;
    while (done < nv) {
        int chunk = nv - done > 32 ? 32 : nv - done;
        const cplx *Vc = V + (size_t)done * stride;
        // one resident round only: dots_kernel<32> holds 3 waves/SIMD (768 workgroups on 256 CUs); a 1024-block grid ran a
        // second, one-third-full round
        // small problems (narrow batches): fewer, fuller workgroups -- the second-stage reduction reads nblk partials per output
        // (four rows per thread: ceil(ceil(n / R) / 4) = ceil(n / 4R))
        const int nblk = (int)std::max(32u, row_grid(n, nb, 256, 4, chunk <= 16 ? DOT_BLOCKS : 768).grid);
        const bool pow2 = nb <= 64 && (nb & (nb - 1)) == 0;     // wavefront-shuffle reduction needs the columns to tile a wavefront
#define WAE_DOTS(MV) do { if (pow2) hipLaunchKernelGGL((dots_kernel<MV, true>), dim3(nblk), dim3(256), 0, st, Vc, stride, chunk, W, n, nb, partial, cmask); \
                          else hipLaunchKernelGGL((dots_kernel<MV, false>), dim3(nblk), dim3(256), 0, st, Vc, stride, chunk, W, n, nb, partial, cmask); } while (0)
        if (chunk <= 8) WAE_DOTS(8);
        else if (chunk <= 16) WAE_DOTS(16);
        else WAE_DOTS(32);
#undef WAE_DOTS
        HIP_CHECK(hipGetLastError());
        int count = chunk * nb;
        launch_reduce_partials(partial, nblk, count, out + (size_t)done * nb, do_sqrt, st, scale ? scale + (size_t)done * nb : nullptr);
        done += chunk;
    }
}
// block version: partial[blk][i*nw + j][b] = sum over this block's rows of conj(V_i[row][b]) W_j[row][b], j < nw <= NW.
// Reads V once for NW right-hand vectors (the projected-operator build of the snapshot basis, beyn.hip rb_append, is a
// tall-skinny Gram product: with one w per launch it re-read the whole basis for every new column).
template <int MAXV, int NW>
__global__ __launch_bounds__(256) void dots_multi_kernel(const cplx *__restrict__ V, size_t sv, int nv, const cplx *__restrict__ W, size_t sw, int nw,
                                                         int64_t n, int nb, cplx *__restrict__ partial) {
    __shared__ cplx sm[256];
    const int tid = threadIdx.x;
    const int R = 256 / nb;
    const int b = tid % nb, rl = tid / nb;
    cplx acc[MAXV][NW];
#pragma unroll
    for (int i = 0; i < MAXV; ++i)
#pragma unroll
        for (int j = 0; j < NW; ++j) acc[i][j] = cplx{0.0, 0.0};
    if (rl < R) {
        for (int64_t row = (int64_t)blockIdx.x * R + rl; row < n; row += (int64_t)gridDim.x * R) {
            const size_t e = (size_t)row * nb + b;
            cplx w[NW];
#pragma unroll
            for (int j = 0; j < NW; ++j) w[j] = j < nw ? W[(size_t)j * sw + e] : cplx{0.0, 0.0};
#pragma unroll
            for (int i = 0; i < MAXV; ++i) {
                if (i < nv) {
                    const cplx v = V[(size_t)i * sv + e];
#pragma unroll
                    for (int j = 0; j < NW; ++j) {
                        acc[i][j].x += v.x * w[j].x + v.y * w[j].y;
                        acc[i][j].y += v.x * w[j].y - v.y * w[j].x;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            if (i < nv && j < nw) {                          // (the serial arm at every nb: the bits this kernel has always given)
                const cplx s = block_colsum<false, 256>(acc[i][j], nb, sm);
                if (tid < nb) partial[((size_t)blockIdx.x * nv * nw + (size_t)i * nw + j) * nb + tid] = s;
            }
        }
    }
}
// out[(i*nw + j)*nb + b] = V_i[:,b]^H W_j[:,b]   (nv arbitrary, nw <= 4)
void launch_dots_multi(const cplx *V, size_t sv, int nv, const cplx *W, size_t sw, int nw, int64_t n, int nb, cplx *partial, cplx *out,
                       hipStream_t st) {
    if (nb < 1 || nb > 256 || nw < 1 || nw > 4) throw WaeError(WAE_ERR_INVALID, "dots_multi: nb in 1..256, nw in 1..4");
    int done = 0;
    while (done < nv) {
        const int chunk = std::min(8, nv - done);
        const int nblk = 768;
        hipLaunchKernelGGL((dots_multi_kernel<8, 4>), dim3(nblk), dim3(256), 0, st, V + (size_t)done * sv, sv, chunk, W, sw, nw, n, nb, partial);
        HIP_CHECK(hipGetLastError());
        const int count = chunk * nw * nb;
        launch_reduce_partials(partial, nblk, count, out + (size_t)done * nw * nb, 0, st);
        done += chunk;
    }
}
void launch_dots(const cplx *V, size_t stride, int nv, const cplx *W, int64_t n, int nb, cplx *partial, cplx *out, hipStream_t st,
                 const unsigned char *cmask) {
    dots_impl(V, stride, nv, W, n, nb, partial, out, 0, st, cmask);
}
void launch_dots_scaled(const cplx *V, size_t stride, int nv, const cplx *W, int64_t n, int nb, cplx *partial, cplx *out, const cplx *scale,
                        hipStream_t st, const unsigned char *cmask) {
    dots_impl(V, stride, nv, W, n, nb, partial, out, 0, st, cmask, scale);
}
void launch_norms(const cplx *X, int64_t n, int nb, cplx *partial, cplx *out, hipStream_t st, const unsigned char *cmask) {
    dots_impl(X, 0, 1, X, n, nb, partial, out, 1, st, cmask);
}

// W[row][b] = base[row][b] + sign * sum_i c[i][b] V_i[row][b].  The nv x nb coefficients are staged in LDS once per
// workgroup (reading them per element through the vector cache doubled the L1 traffic of this streaming kernel), and
// the basis vectors are fetched AXU at a time so that up to AXU 16-B loads are in flight per lane.
// Thread t owns column t % nb and every R-th row, R = 256 / nb (as in dots_kernel).
// A lane whose coefficient for V_i is exactly (0, 0) neither loads its entry of V_i nor adds to its sum: the update x += V y at the end
// of a lock-step cycle has zeros for every step beyond a column's own (gmres_solve_y_kernel), about half of all (vector, column) pairs
// of a contour pass, and what a converged column's chunk of a basis slot holds is stale (any bits, a NaN included: 0 * NaN would poison
// the sum).  The choice is per lane: the other lanes of the wavefront still have AXU loads in flight.
constexpr int AXU = 8;
constexpr int AX_MAXC = 4096;      // coefficients per launch (64 KB of LDS)
__device__ __forceinline__ bool nonzero(const cplx &c) { return c.x != 0.0 || c.y != 0.0; }
// NORM: additionally partial[blk][b] = sum over this workgroup's rows of |W[row][b]|^2 (the Gram-Schmidt step needs the norm
// of the vector it has just written: one pass over it less)
template <bool NORM>
__global__ __launch_bounds__(256) void axpy_neg_kernel(const cplx *__restrict__ V, size_t stride, int nv, const cplx *__restrict__ h,
                                                       cplx *W, int64_t n, int nb, double sign, const cplx *base,
                                                       const unsigned char *__restrict__ cmask, cplx *__restrict__ partial) {
    extern __shared__ cplx hs[];
    const int tid = threadIdx.x;
    for (int k = tid; k < nv * nb; k += 256) {
        const cplx c = h[k];
        hs[k] = cplx{sign * c.x, sign * c.y};
    }
    __syncthreads();
    const int R = 256 / nb;
    const int b = tid % nb, rl = tid / nb;
    const bool live = rl < R && !(cmask && !cmask[b >> 3]);
    if (!NORM && !live) return;
    double nrm2 = 0.0;
    // bit u: vector i0 + u exists and this lane's coefficient of it is not (0, 0).  The bits of a group of AXU vectors are taken one group
    // ahead, while the loads of the group before are in flight, so that no load waits for LDS; they do not depend on the row, and those
    // of the first group are taken once.  The last group may be short: its missing vectors have no bit, and their LDS reads go to the last
    // vector's coefficient.  group_coefs reads the AXU coefficients in a row and pins them in registers: left to itself the compiler puts
    // every read behind a branch of its own, with a wait each.
    const cplx *const hb = hs + b;
    auto group_coefs = [&](int i0, cplx (&c)[AXU]) {
#pragma unroll
        for (int u = 0; u < AXU; ++u) c[u] = hb[(i0 + u < nv ? i0 + u : nv - 1) * nb];
#pragma unroll
        for (int u = 0; u < AXU; ++u) asm volatile("" : "+v"(c[u].x), "+v"(c[u].y));      // no instruction
    };
    auto group_bits = [&](int i0) {
        cplx c[AXU];
        group_coefs(i0, c);
        unsigned m = 0;
#pragma unroll
        for (int u = 0; u < AXU; ++u) m |= (unsigned)(i0 + u < nv) & (unsigned)nonzero(c[u]) ? 1u << u : 0u;
        return m;
    };
    const unsigned nz0 = (live && nv > 0) ? group_bits(0) : 0u;
    if (live)
    for (int64_t row = (int64_t)blockIdx.x * R + rl; row < n; row += (int64_t)gridDim.x * R) {
        const size_t e = (size_t)row * nb + b;
        cplx acc = base ? base[e] : cplx{0.0, 0.0};
        // one group: the loads its bits ask for, the bits of the next group, the sums; returns those bits.  The products are written out
        // with fma: these are the roundings this kernel has always had -- a full group and the short last one (`full`) differ in which
        // product of the imaginary part is rounded first -- and no compiler choice can move them.
        auto group = [&](int i, unsigned nz, auto full) {
            cplx v[AXU], c[AXU];
#pragma unroll
            for (int u = 0; u < AXU; ++u) v[u] = (nz >> u & 1u) ? stream_load(V + (size_t)(i + u) * stride + e) : cplx{0.0, 0.0};
            const unsigned nz_next = i + AXU < nv ? group_bits(i + AXU) : 0u;
            group_coefs(i, c);
#pragma unroll
            for (int u = 0; u < AXU; ++u) {
                cplx t = acc;
                t.x += fma(c[u].x, v[u].x, -(c[u].y * v[u].y));
                t.y += decltype(full)::value ? fma(c[u].y, v[u].x, c[u].x * v[u].y) : fma(c[u].x, v[u].y, c[u].y * v[u].x);
                if (nz >> u & 1u) acc = t;
            }
            return nz_next;
        };
        int i = 0;
        unsigned nz = nz0;
        for (; i + AXU <= nv; i += AXU) nz = group(i, nz, std::true_type{});
        if (i < nv) group(i, nz, std::false_type{});
        W[e] = acc;
        if (NORM) nrm2 += fma(acc.x, acc.x, acc.y * acc.y);      // (written out for the same reason)
    }
    if (NORM) {
        __syncthreads();                        // hs is re-used for the reduction
        double *sm = (double *)hs;
        nrm2 = nb <= 64 && (nb & (nb - 1)) == 0 ? block_colsum<true, 256>(nrm2, nb, sm) : block_colsum<false, 256>(nrm2, nb, sm);
        if (tid < nb) partial[(size_t)blockIdx.x * nb + tid] = cplx{nrm2, 0.0};
    }
}
// launch(done, chunk, shm) for the coefficient groups of nv vectors: chunk vectors from vector done on, at most AX_MAXC coefficients
// and shm bytes of them per launch.  nv == 0 is one launch with chunk = 0 (the kernels still write W = base, or 0).
template <class F> static void for_coef_groups(int nv, int nb, F &&launch) {
    const int maxv = std::max(1, AX_MAXC / nb);
    int done = 0;
    do {
        const int chunk = std::min(nv - done, maxv);
        launch(done, chunk, (size_t)std::max(chunk, 1) * nb * sizeof(cplx));
        HIP_CHECK(hipGetLastError());
        done += chunk;
    } while (done < nv);
}
static void axpy_impl(const cplx *V, size_t stride, int nv, const cplx *c, cplx *W, int64_t n, int nb, double sign, const cplx *base,
                      hipStream_t st, const unsigned char *cmask) {
    if (!n || nb < 1) return;
    if (nb > 256) throw WaeError(WAE_ERR_INVALID, "axpy: nb must be in 1..256");
    const unsigned grid = row_grid(n, nb, 256, 1, 2048).grid;
    for_coef_groups(nv, nb, [&](int done, int chunk, size_t shm) {
        hipLaunchKernelGGL(axpy_neg_kernel<false>, dim3(grid), dim3(256), shm, st, V + (size_t)done * stride, stride, chunk, c + (size_t)done * nb, W,
                           n, nb, sign, done ? (const cplx *)W : base, cmask, (cplx *)nullptr);
    });
}
void launch_axpy_neg(const cplx *V, size_t stride, int nv, const cplx *h, cplx *W, int64_t n, int nb, hipStream_t st, const unsigned char *cmask) {
    axpy_impl(V, stride, nv, h, W, n, nb, -1.0, W, st, cmask);
}
// W_j -= sum_i h[i][j] V_i for CNT vectors W_j (stride wstride) in ONE reading of V_0..nv-1: the block Gram-Schmidt update of the
// snapshot basis (beyn.hip rb_append_block), whose four new vectors used to read the basis once each.  h[(i*CNT + j)*nb + b], the
// layout dots_multi writes.
template <int CNT>
__global__ __launch_bounds__(256) void axpy_neg_multi_kernel(const cplx *__restrict__ V, size_t stride, int nv, const cplx *__restrict__ h, cplx *W,
                                                             size_t wstride, int64_t n, int nb) {
    extern __shared__ cplx hs[];
    const int tid = threadIdx.x;
    for (int k = tid; k < nv * CNT * nb; k += 256) {
        const cplx c = h[k];
        hs[k] = cplx{-c.x, -c.y};
    }
    __syncthreads();
    const int R = 256 / nb;
    const int b = tid % nb, rl = tid / nb;
    if (rl >= R) return;
    for (int64_t row = (int64_t)blockIdx.x * R + rl; row < n; row += (int64_t)gridDim.x * R) {
        const size_t e = (size_t)row * nb + b;
        cplx acc[CNT];
#pragma unroll
        for (int j = 0; j < CNT; ++j) acc[j] = W[(size_t)j * wstride + e];
        for (int i = 0; i < nv; ++i) {
            const cplx v = stream_load(V + (size_t)i * stride + e);
#pragma unroll
            for (int j = 0; j < CNT; ++j) {
                const cplx c = hs[(i * CNT + j) * nb + b];
                acc[j].x += c.x * v.x - c.y * v.y;
                acc[j].y += c.x * v.y + c.y * v.x;
            }
        }
#pragma unroll
        for (int j = 0; j < CNT; ++j) W[(size_t)j * wstride + e] = acc[j];
    }
}
void launch_axpy_neg_multi(const cplx *V, size_t stride, int nv, const cplx *h, cplx *W, size_t wstride, int cnt, int64_t n, int nb, hipStream_t st) {
    if (!n || nb < 1 || nv < 1 || cnt < 1) return;
    const size_t shm = (size_t)nv * cnt * nb * sizeof(cplx);
    if (nb > 256 || cnt > 4 || shm > 60 * 1024) throw WaeError(WAE_ERR_INVALID, "axpy_neg_multi: coefficients do not fit one launch");
    const unsigned grid = row_grid(n, nb, 256, 1, 2048).grid;
    switch (cnt) {
    case 1: hipLaunchKernelGGL(axpy_neg_multi_kernel<1>, dim3(grid), dim3(256), shm, st, V, stride, nv, h, W, wstride, n, nb); break;
    case 2: hipLaunchKernelGGL(axpy_neg_multi_kernel<2>, dim3(grid), dim3(256), shm, st, V, stride, nv, h, W, wstride, n, nb); break;
    case 3: hipLaunchKernelGGL(axpy_neg_multi_kernel<3>, dim3(grid), dim3(256), shm, st, V, stride, nv, h, W, wstride, n, nb); break;
    default: hipLaunchKernelGGL(axpy_neg_multi_kernel<4>, dim3(grid), dim3(256), shm, st, V, stride, nv, h, W, wstride, n, nb); break;
    }
    HIP_CHECK(hipGetLastError());
}
// w -= V h and norms[b] = ||w[:,b]|| in one pass over w (falls back to two kernels when the coefficients do not fit one launch)
// base (optional): W = base - V h instead of the in-place update; inv_out (optional): 1/||W[:,b]||^2 beside the norms.  Both are
// what a Krylov basis kept UNNORMALISED needs (gmres.hip gmres): the new vector goes straight into its basis slot.
void launch_axpy_neg_norm(const cplx *V, size_t stride, int nv, const cplx *h, cplx *W, int64_t n, int nb, cplx *partial, cplx *norms,
                          hipStream_t st, const unsigned char *cmask, const cplx *base, cplx *inv_out) {
    if (!n || nb < 1) return;
    if (nb > 256) throw WaeError(WAE_ERR_INVALID, "axpy: nb must be in 1..256");
    if (!base) base = W;
    if (nv < 1 || nv > AX_MAXC / nb) {
        if (inv_out) throw WaeError(WAE_ERR_INVALID, "axpy_neg_norm: inverse norms need the single-launch form");
        axpy_impl(V, stride, nv, h, W, n, nb, -1.0, base, st, cmask);
        launch_norms(W, n, nb, partial, norms, st, cmask);
        return;
    }
    const unsigned grid = row_grid(n, nb, 256, 1, 1024).grid;
    const size_t shm = std::max((size_t)nv * nb * sizeof(cplx), (size_t)256 * sizeof(double));
    hipLaunchKernelGGL(axpy_neg_kernel<true>, dim3(grid), dim3(256), shm, st, V, stride, nv, h, W, n, nb, -1.0, base, cmask, partial);
    HIP_CHECK(hipGetLastError());
    launch_reduce_partials(partial, (int)grid, nb, norms, 1, st, nullptr, inv_out);
}
// ---------------------------------------------------------------------------------------------------
// Two Arnoldi steps per pass over the basis (gmres.hip Gmres::run_device, "pair" steps).  With w1 = Op v_j and w2 = Op w1 -- the operator
// applied to the vector BEFORE it is orthogonalised -- both new basis vectors come out of ONE reading of V_0..j for the inner
// products and ONE for the update, where two single steps read it four times: the Gram-Schmidt traffic of a long recurrence, the
// largest stream of a from-zero solve, halves.
//   dots2:  c1 = V^H w1, c2 = V^H w2 (each scaled by 1/||v_i||^2: coefficients against the unnormalised basis) and the Gram
//           entries w1^H w1, w1^H w2, w2^H w2;
//   axpy2:  v_{j+1} = w1 - V c1,   v_{j+2} = w2 - alpha w1 - V (c2 - alpha c1)   in place, with their squared norms.
// ---------------------------------------------------------------------------------------------------
template <int MAXV, bool POW2>
__global__ __launch_bounds__(256) void dots2_kernel(const cplx *__restrict__ V, size_t stride, int nv, const cplx *__restrict__ W1,
                                                    const cplx *__restrict__ W2, int64_t n, int nb, cplx *__restrict__ partial,
                                                    const unsigned char *__restrict__ cmask, int gram) {
    __shared__ cplx sm[256];
    const int tid = threadIdx.x;
    const int R = 256 / nb;
    const int b = tid % nb, rl = tid / nb;
    const bool live = rl < R && (!cmask || cmask[b >> 3]);
    cplx a1[MAXV], a2[MAXV];
    cplx g[3];
#pragma unroll
    for (int i = 0; i < MAXV; ++i) { a1[i] = cplx{0.0, 0.0}; a2[i] = cplx{0.0, 0.0}; }
    g[0] = g[1] = g[2] = cplx{0.0, 0.0};
    if (live) {
        for (int64_t row = (int64_t)blockIdx.x * R + rl; row < n; row += (int64_t)gridDim.x * R) {
            const size_t e = (size_t)row * nb + b;
            const cplx w1 = W1[e], w2 = W2[e];
            if (gram) {
                g[0].x += w1.x * w1.x + w1.y * w1.y;
                g[1].x += w1.x * w2.x + w1.y * w2.y; g[1].y += w1.x * w2.y - w1.y * w2.x;
                g[2].x += w2.x * w2.x + w2.y * w2.y;
            }
#pragma unroll
            for (int i = 0; i < MAXV; ++i) {
                if (i < nv) {
                    const cplx v = stream_load(V + (size_t)i * stride + e);
                    a1[i].x += v.x * w1.x + v.y * w1.y; a1[i].y += v.x * w1.y - v.y * w1.x;
                    a2[i].x += v.x * w2.x + v.y * w2.y; a2[i].y += v.x * w2.y - v.y * w2.x;
                }
            }
        }
    }
    // block reduction (as dots_kernel); output order [k][i][b], k = 0, 1, then the three Gram entries
    const int nout = 2 * nv + (gram ? 3 : 0);
    auto reduce_store = [&](cplx v, int slot) {
        const cplx s = block_colsum<POW2, 256>(v, nb, sm);
        if (tid < nb) partial[((size_t)blockIdx.x * nout + slot) * nb + tid] = s;
    };
#pragma unroll
    for (int i = 0; i < MAXV; ++i)
        if (i < nv) { reduce_store(a1[i], i); reduce_store(a2[i], nv + i); }
    if (gram)
        for (int q = 0; q < 3; ++q) reduce_store(g[q], 2 * nv + q);
}
// second stage: out1[i][b], out2[i][b] (scaled by scale[i][b].x) and gram[q][b] from partial[blk][2 nv + 3][nb]
__global__ __launch_bounds__(256) void reduce_partials2_kernel(const cplx *__restrict__ partial, int nblk, int nv, int nb, int gram, cplx *__restrict__ out1,
                                                               cplx *__restrict__ out2, const cplx *__restrict__ scale, cplx *__restrict__ gram_out) {
    constexpr int EPB = 2;
    const int count = (2 * nv + (gram ? 3 : 0)) * nb;
    const cplx acc = sum_partials<EPB>(partial, nblk, count);
    const int e = blockIdx.x * EPB + threadIdx.x;
    if (threadIdx.x < EPB && e < count) {
        const int slot = e / nb, b = e - slot * nb;
        if (slot < 2 * nv) {
            const int i = slot < nv ? slot : slot - nv;
            const double sc = scale[(size_t)i * nb + b].x;
            (slot < nv ? out1 : out2)[(size_t)i * nb + b] = cplx{acc.x * sc, acc.y * sc};
        } else {
            gram_out[(size_t)(slot - 2 * nv) * nb + b] = acc;
        }
    }
}
void launch_dots2_scaled(const cplx *V, size_t stride, int nv, const cplx *W1, const cplx *W2, int64_t n, int nb, cplx *partial, cplx *out1,
                         cplx *out2, cplx *gram_out, const cplx *scale, hipStream_t st, const unsigned char *cmask) {
    if (nb < 1 || nb > 256) throw WaeError(WAE_ERR_INVALID, "dots2: nb must be in 1..256");
    const bool pow2 = nb <= 64 && (nb & (nb - 1)) == 0;
    const int nblk = (int)std::max(32u, row_grid(n, nb, 256, 4, 768).grid);      // (as dots_impl)
    int done = 0;
    do {
        const int chunk = std::min(16, nv - done);
        const int gram = done == 0 ? 1 : 0;
        const cplx *Vc = V + (size_t)done * stride;
        if (pow2) hipLaunchKernelGGL((dots2_kernel<16, true>), dim3(nblk), dim3(256), 0, st, Vc, stride, chunk, W1, W2, n, nb, partial, cmask, gram);
        else hipLaunchKernelGGL((dots2_kernel<16, false>), dim3(nblk), dim3(256), 0, st, Vc, stride, chunk, W1, W2, n, nb, partial, cmask, gram);
        HIP_CHECK(hipGetLastError());
        const int count = (2 * chunk + (gram ? 3 : 0)) * nb;
        hipLaunchKernelGGL(reduce_partials2_kernel, dim3((count + 1) / 2), dim3(256), 0, st, partial, nblk, chunk, nb, gram, out1 + (size_t)done * nb,
                           out2 + (size_t)done * nb, scale + (size_t)done * nb, gram_out);
        HIP_CHECK(hipGetLastError());
        done += chunk;
    } while (done < nv);
}

// v1 = w1 - V c1,  v2 = w2 - alpha w1 - V c2m  (c2m = c2 - alpha c1), in place of w1 / w2; partial[blk][k][b] = this workgroup's part
// of ||v_k||^2.  Coefficients staged in LDS ([2][nv][nb]); 512 threads so that one workgroup per CU keeps ~64 KB of loads in flight.
template <int NT>
__global__ __launch_bounds__(NT) void axpy2_kernel(const cplx *__restrict__ V, size_t stride, int nv, const cplx *__restrict__ c1, const cplx *__restrict__ c2m,
                                                   const cplx *__restrict__ alpha, cplx *W1, cplx *W2, int64_t n, int nb,
                                                   const unsigned char *__restrict__ cmask, cplx *__restrict__ partial) {
    extern __shared__ cplx hs[];
    const int tid = threadIdx.x;
    for (int k = tid; k < nv * nb; k += NT) { hs[k] = c1[k]; hs[nv * nb + k] = c2m[k]; }
    __syncthreads();
    const int R = NT / nb;
    const int b = tid % nb, rl = tid / nb;
    const bool live = rl < R && !(cmask && !cmask[b >> 3]);
    double n1 = 0.0, n2 = 0.0;
    if (live) {
        const cplx al = alpha[b];
        const cplx *h1 = hs + b, *h2 = hs + (size_t)nv * nb + b;
        for (int64_t row = (int64_t)blockIdx.x * R + rl; row < n; row += (int64_t)gridDim.x * R) {
            const size_t e = (size_t)row * nb + b;
            const cplx w1 = W1[e], w2 = W2[e];
            cplx o1 = w1;
            cplx o2 = {w2.x - (al.x * w1.x - al.y * w1.y), w2.y - (al.x * w1.y + al.y * w1.x)};
            int i = 0;
            for (; i + AXU <= nv; i += AXU) {
                cplx v[AXU];
#pragma unroll
                for (int u = 0; u < AXU; ++u) v[u] = stream_load(V + (size_t)(i + u) * stride + e);
#pragma unroll
                for (int u = 0; u < AXU; ++u) {
                    const cplx p = h1[(size_t)(i + u) * nb], q = h2[(size_t)(i + u) * nb];
                    o1.x -= p.x * v[u].x - p.y * v[u].y; o1.y -= p.x * v[u].y + p.y * v[u].x;
                    o2.x -= q.x * v[u].x - q.y * v[u].y; o2.y -= q.x * v[u].y + q.y * v[u].x;
                }
            }
            for (; i < nv; ++i) {
                const cplx p = h1[(size_t)i * nb], q = h2[(size_t)i * nb];
                const cplx v = stream_load(V + (size_t)i * stride + e);
                o1.x -= p.x * v.x - p.y * v.y; o1.y -= p.x * v.y + p.y * v.x;
                o2.x -= q.x * v.x - q.y * v.y; o2.y -= q.x * v.y + q.y * v.x;
            }
            W1[e] = o1;
            W2[e] = o2;
            n1 += o1.x * o1.x + o1.y * o1.y;
            n2 += o2.x * o2.x + o2.y * o2.y;
        }
    }
    __syncthreads();                            // hs is re-used for the reduction
    // (the serial arm at every nb: the bits this kernel has always given.  Its sums used to start from 0.0 and add the entries
    // k = 0 ..., block_colsum starts from entry 0: the same bits, because a sum of squares is never -0.0 and 0.0 + x = x otherwise)
    double *sm = (double *)hs;
    n1 = block_colsum<false, NT>(n1, nb, sm);
    n2 = block_colsum<false, NT>(n2, nb, sm);
    if (tid < nb) {
        partial[((size_t)blockIdx.x * 2 + 0) * nb + tid] = cplx{n1, 0.0};
        partial[((size_t)blockIdx.x * 2 + 1) * nb + tid] = cplx{n2, 0.0};
    }
}
// norms[k][b] = ||v_k[:,b]|| and inv[k][b] = 1/||v_k||^2, k = 0, 1 (norms, inv: 2 x nb each)
void launch_axpy2_norm(const cplx *V, size_t stride, int nv, const cplx *c1, const cplx *c2m, const cplx *alpha, cplx *W1, cplx *W2, int64_t n, int nb,
                       cplx *partial, cplx *norms, cplx *inv_out, hipStream_t st, const unsigned char *cmask) {
    if (!n || nb < 1) return;
    if (nb > 256 || nv < 1 || (size_t)2 * nv * nb * sizeof(cplx) > 150 * 1024) throw WaeError(WAE_ERR_INVALID, "axpy2: coefficients do not fit LDS");
    static OncePerDevice lds_opt_in;
    once_per_device(lds_opt_in, [](int) {
        HIP_CHECK(hipFuncSetAttribute((const void *)axpy2_kernel<512>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
        HIP_CHECK(hipFuncSetAttribute((const void *)axpy2_kernel<256>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
    });
    const size_t shm = std::max((size_t)2 * nv * nb * sizeof(cplx), (size_t)2 * 512 * sizeof(double));
    const bool big = shm > 40 * 1024;              // few workgroups fit a CU: make them large
    const unsigned grid = row_grid(n, nb, big ? 512 : 256, 1, big ? 512 : 1024).grid;
    if (big) hipLaunchKernelGGL(axpy2_kernel<512>, dim3(grid), dim3(512), shm, st, V, stride, nv, c1, c2m, alpha, W1, W2, n, nb, cmask, partial);
    else hipLaunchKernelGGL(axpy2_kernel<256>, dim3(grid), dim3(256), shm, st, V, stride, nv, c1, c2m, alpha, W1, W2, n, nb, cmask, partial);
    HIP_CHECK(hipGetLastError());
    launch_reduce_partials(partial, (int)grid, 2 * nb, norms, 1, st, nullptr, inv_out);
}

void launch_lincomb(const cplx *V, size_t stride, int nv, const cplx *y, cplx *Y, int64_t n, int nb, hipStream_t st) {
    axpy_impl(V, stride, nv, y, Y, n, nb, 1.0, nullptr, st, nullptr);
}
void launch_lincomb_add(const cplx *V, size_t stride, int nv, const cplx *y, cplx *X, int64_t n, int nb, hipStream_t st) {
    axpy_impl(V, stride, nv, y, X, n, nb, 1.0, X, st, nullptr);      // X += sum_i y_i V_i
}

// ---------------------------------------------------------------------------------------------------
// snapshot-basis helpers (Galerkin initial guesses for the shifted systems of a contour, beyn.hip: beyn_moments_rb)
// ---------------------------------------------------------------------------------------------------
// out[row][c] = X[row][off + c], c < l   (one system's l columns out of a lock-step batch of nb columns)
__global__ __launch_bounds__(256) void extract_cols_kernel(const cplx *__restrict__ X, int nb, int off, int l, cplx *__restrict__ out, size_t total) {
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t row = e / l;
        const int c = (int)(e - row * l);
        out[e] = X[row * nb + off + c];
    }
}
void launch_extract_cols(const cplx *X, int nb, int off, int l, cplx *out, int64_t n, hipStream_t st) {
    const size_t total = (size_t)n * l;
    if (!total) return;
    hipLaunchKernelGGL(extract_cols_kernel, dim3(grid_for(total)), dim3(256), 0, st, X, nb, off, l, out, total);
    HIP_CHECK(hipGetLastError());
}
// X[row][b] = sum_i y[i][b] Q_i[row][b % l]: the basis multivectors have l columns (one per probe column), the batch
// has nb = nsys*l columns (every system re-uses the same l bases with its own coefficients).  Coefficients in LDS.
__global__ __launch_bounds__(256) void lincomb_rep_kernel(const cplx *__restrict__ Q, size_t stride, int nv, const cplx *__restrict__ y,
                                                          cplx *__restrict__ X, int64_t n, int nb, int l, int accumulate) {
    extern __shared__ cplx hs[];
    const int tid = threadIdx.x;
    for (int k = tid; k < nv * nb; k += 256) hs[k] = y[k];
    __syncthreads();
    const int R = 256 / nb;
    const int b = tid % nb, rl = tid / nb;
    if (rl >= R) return;
    const int c = b % l;
    for (int64_t row = (int64_t)blockIdx.x * R + rl; row < n; row += (int64_t)gridDim.x * R) {
        const size_t eq = (size_t)row * l + c;
        cplx acc = accumulate ? X[(size_t)row * nb + b] : cplx{0.0, 0.0};
        int i = 0;
        for (; i + AXU <= nv; i += AXU) {
            cplx v[AXU];
#pragma unroll
            for (int u = 0; u < AXU; ++u) v[u] = Q[(size_t)(i + u) * stride + eq];
#pragma unroll
            for (int u = 0; u < AXU; ++u) {
                const cplx cf = hs[(i + u) * nb + b];
                acc.x += cf.x * v[u].x - cf.y * v[u].y;
                acc.y += cf.x * v[u].y + cf.y * v[u].x;
            }
        }
        for (; i < nv; ++i) {
            const cplx cf = hs[i * nb + b];
            const cplx v = Q[(size_t)i * stride + eq];
            acc.x += cf.x * v.x - cf.y * v.y;
            acc.y += cf.x * v.y + cf.y * v.x;
        }
        X[(size_t)row * nb + b] = acc;
    }
}
// The same for batches of at most 8 systems (l >= 8 probe columns at the default width): one thread per (row, probe column)
// loads every basis entry ONCE and feeds the accumulators of all systems -- in the kernel above the lanes of the nsys systems
// load the same 16 bytes each (8 x the L1 requests: 2.55 TB/s of unique reads at 1M DoF).
constexpr int LRS = 8;
__global__ __launch_bounds__(256) void lincomb_rep8_kernel(const cplx *__restrict__ Q, size_t stride, int nv, const cplx *__restrict__ y,
                                                           cplx *__restrict__ X, int64_t n, int nb, int l, int nsys, int accumulate) {
    extern __shared__ cplx hs[];
    const int tid = threadIdx.x;
    for (int k = tid; k < nv * nb; k += 256) hs[k] = y[k];
    __syncthreads();
    const int R = 256 / l;
    const int c = tid % l, rl = tid / l;
    if (rl >= R) return;
    // TWO rows per thread and step (round 4): every coefficient read from LDS serves both, and eight basis entries are in flight per
    // thread instead of four (1 214 -> ~900 us for the 40 x 8 x 1M basis of the benchmark: the kernel was bound by its LDS reads, one
    // 16-byte coefficient per basis entry and system)
    for (int64_t row0 = ((int64_t)blockIdx.x * R + rl) * 2; row0 < n; row0 += (int64_t)gridDim.x * R * 2) {
        const bool two = row0 + 1 < n;
        const size_t eq0 = (size_t)row0 * l + c, eq1 = two ? eq0 + l : eq0;
        cplx acc[2][LRS];
#pragma unroll
        for (int s = 0; s < LRS; ++s) {
            acc[0][s] = (accumulate && s < nsys) ? X[(size_t)row0 * nb + s * l + c] : cplx{0.0, 0.0};
            acc[1][s] = (accumulate && s < nsys && two) ? X[(size_t)(row0 + 1) * nb + s * l + c] : cplx{0.0, 0.0};
        }
        int i = 0;
        for (; i + 4 <= nv; i += 4) {
            cplx v0[4], v1[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { v0[u] = Q[(size_t)(i + u) * stride + eq0]; v1[u] = Q[(size_t)(i + u) * stride + eq1]; }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int s = 0; s < LRS; ++s)
                    if (s < nsys) {
                        const cplx cf = hs[(i + u) * nb + s * l + c];
                        acc[0][s].x += cf.x * v0[u].x - cf.y * v0[u].y;
                        acc[0][s].y += cf.x * v0[u].y + cf.y * v0[u].x;
                        acc[1][s].x += cf.x * v1[u].x - cf.y * v1[u].y;
                        acc[1][s].y += cf.x * v1[u].y + cf.y * v1[u].x;
                    }
        }
        for (; i < nv; ++i) {
            const cplx v0 = Q[(size_t)i * stride + eq0], v1 = Q[(size_t)i * stride + eq1];
#pragma unroll
            for (int s = 0; s < LRS; ++s)
                if (s < nsys) {
                    const cplx cf = hs[i * nb + s * l + c];
                    acc[0][s].x += cf.x * v0.x - cf.y * v0.y;
                    acc[0][s].y += cf.x * v0.y + cf.y * v0.x;
                    acc[1][s].x += cf.x * v1.x - cf.y * v1.y;
                    acc[1][s].y += cf.x * v1.y + cf.y * v1.x;
                }
        }
#pragma unroll
        for (int s = 0; s < LRS; ++s)
            if (s < nsys) {
                X[(size_t)row0 * nb + s * l + c] = acc[0][s];
                if (two) X[(size_t)(row0 + 1) * nb + s * l + c] = acc[1][s];
            }
    }
}
void launch_lincomb_rep(const cplx *Q, size_t stride, int nv, const cplx *y, cplx *X, int64_t n, int nb, int l, hipStream_t st) {
    if (!n || nb < 1) return;
    if (nb > 256) throw WaeError(WAE_ERR_INVALID, "lincomb_rep: nb must be in 1..256");
    if (l >= 4 && l <= 256 && nb % l == 0 && nb / l <= LRS) {
        const int nsys = nb / l;
        const unsigned grid = row_grid(n, l, 256, 2, 4096).grid;       // a thread per (row, probe column), two rows per thread
        for_coef_groups(nv, nb, [&](int done, int chunk, size_t shm) {
            hipLaunchKernelGGL(lincomb_rep8_kernel, dim3(grid), dim3(256), shm, st, Q + (size_t)done * stride, stride, chunk, y + (size_t)done * nb, X,
                               n, nb, l, nsys, done ? 1 : 0);
        });
        return;
    }
    const unsigned grid = row_grid(n, nb, 256, 1, 2048).grid;
    for_coef_groups(nv, nb, [&](int done, int chunk, size_t shm) {
        hipLaunchKernelGGL(lincomb_rep_kernel, dim3(grid), dim3(256), shm, st, Q + (size_t)done * stride, stride, chunk, y + (size_t)done * nb, X, n,
                           nb, l, done ? 1 : 0);
    });
}
// X[row][b] *= keep[b] (keep = 0 or 1, real part of a complex table): drop the guesses of selected columns
__global__ __launch_bounds__(256) void mask_cols_kernel(cplx *__restrict__ X, const cplx *__restrict__ keep, size_t total, int nb) {
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        if (keep[e % nb].x == 0.0) X[e] = cplx{0.0, 0.0};
    }
}
void launch_mask_cols(cplx *X, const cplx *keep, int64_t n, int nb, hipStream_t st) {
    const size_t total = (size_t)n * nb;
    if (!total) return;
    hipLaunchKernelGGL(mask_cols_kernel, dim3(grid_for(total)), dim3(256), 0, st, X, keep, total, nb);
    HIP_CHECK(hipGetLastError());
}

__global__ __launch_bounds__(256) void scale_inv_kernel(const cplx *__restrict__ X, const cplx *__restrict__ alpha, cplx *__restrict__ Y, size_t total, int nb,
                                                        const unsigned char *__restrict__ cmask) {
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        if (cmask && !cmask[(e % nb) >> 3]) continue;
        const double a = alpha[e % nb].x;
        const double s = (a > 1e-300) ? 1.0 / a : 0.0;
        const cplx x = X[e];
        Y[e] = cplx{x.x * s, x.y * s};
    }
}
void launch_scale_inv(const cplx *X, const cplx *alpha, cplx *Y, int64_t n, int nb, hipStream_t st, const unsigned char *cmask) {
    size_t total = (size_t)n * nb;
    if (!total) return;
    hipLaunchKernelGGL(scale_inv_kernel, dim3(grid_for(total)), dim3(256), 0, st, X, alpha, Y, total, nb, cmask);
    HIP_CHECK(hipGetLastError());
}

// The column-major side of these three is in the CALLER's row numbering, the interleaved side in the library's (tiles.h):
// perm[i] = caller's row of internal row i (null: same numbering).
// out = a x + b y (or a conj(x) + b y) for one vector (out may alias x or y): the column updates of the device-resident multivectors (wae_slot_axpby).
// b == 0 follows the BLAS convention: y is not read and out = a x, whatever y holds (a NaN or Inf left in a slot column does not survive
// an overwrite; 0 * NaN would)
__global__ __launch_bounds__(256) void axpby1_kernel(cplx a, const cplx *x, cplx b, const cplx *y, cplx *out, size_t n, int conj_x) {
    const bool use_y = b.x != 0.0 || b.y != 0.0;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        cplx r = cmul(a, conj_x ? cconj(x[e]) : x[e]);
        if (use_y) cfma(r, b, y[e]);
        out[e] = r;
    }
}
void launch_axpby1(cplx a, const cplx *x, cplx b, const cplx *y, cplx *out, size_t n, hipStream_t st, int conj_x) {
    if (!n) return;
    hipLaunchKernelGGL(axpby1_kernel, dim3(grid_for(n)), dim3(256), 0, st, a, x, b, y, out, n, conj_x);
    HIP_CHECK(hipGetLastError());
}
__global__ __launch_bounds__(256) void colmajor_to_inter_kernel(const cplx *__restrict__ Xc, int64_t d, int r, cplx *__restrict__ Xi, int nb,
                                                                const int *__restrict__ perm) {
    const size_t total = (size_t)d * nb;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t row = e / nb;
        const int b = (int)(e - row * nb);
        const size_t src = perm ? (size_t)perm[row] : row;
        Xi[e] = (b < r) ? Xc[(size_t)b * d + src] : cplx{0.0, 0.0};
    }
}
void launch_colmajor_to_inter(const cplx *Xc, int64_t d, int r, cplx *Xi, int nb, hipStream_t st, const int *perm) {
    hipLaunchKernelGGL(colmajor_to_inter_kernel, dim3(grid_for((size_t)d * nb)), dim3(256), 0, st, Xc, d, r, Xi, nb, perm);
    HIP_CHECK(hipGetLastError());
}
__global__ __launch_bounds__(256) void inter_to_colmajor_kernel(const cplx *__restrict__ Xi, int nb, int64_t d, int r, cplx *__restrict__ Xc,
                                                                const int *__restrict__ perm) {
    const size_t total = (size_t)d * r;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t b = e / d, row = e - b * d;
        const size_t dst = perm ? (size_t)perm[row] : row;
        Xc[b * d + dst] = Xi[row * nb + b];
    }
}
void launch_inter_to_colmajor(const cplx *Xi, int nb, int64_t d, int r, cplx *Xc, hipStream_t st, const int *perm) {
    if (!d || !r) return;
    hipLaunchKernelGGL(inter_to_colmajor_kernel, dim3(grid_for((size_t)d * r)), dim3(256), 0, st, Xi, nb, d, r, Xc, perm);
    HIP_CHECK(hipGetLastError());
}
__global__ __launch_bounds__(256) void replicate_kernel(const cplx *__restrict__ Vc, int64_t d, int l, cplx *__restrict__ Xi, int nb,
                                                        const int *__restrict__ perm) {
    const size_t total = (size_t)d * nb;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const size_t row = e / nb;
        const int b = (int)(e - row * nb);
        const size_t src = perm ? (size_t)perm[row] : row;
        Xi[e] = Vc[(size_t)(b % l) * d + src];
    }
}
void launch_replicate(const cplx *Vc, int64_t d, int l, cplx *Xi, int nb, hipStream_t st, const int *perm) {
    hipLaunchKernelGGL(replicate_kernel, dim3(grid_for((size_t)d * nb)), dim3(256), 0, st, Vc, d, l, Xi, nb, perm);
    HIP_CHECK(hipGetLastError());
}

// A[(p*lA + c0 + c)*d + row] += sum_s w[s] z[s]^p X[row][s*l+c]
// X is interleaved [row][nb] and A column-major [row fastest]: a workgroup stages TR rows of X in LDS (coalesced 16-B reads),
// then every thread owns one (row, c) of the tile, sums over the systems in registers and touches each moment entry once
// (coalesced along the rows).  The first version read X with a 1-KB lane stride and re-read/re-wrote A once per system:
// 1.5 ms per chunk at 1M DoF against 0.4 ms of traffic.
constexpr int ACC_MAXP = 8;         // moments (2K) accumulated in registers per pass over the systems
__global__ __launch_bounds__(256) void beyn_accum_kernel(const cplx *__restrict__ Xi, int nb, int64_t d, int l, int nsys,
                                                         const cplx *__restrict__ w, const cplx *__restrict__ z, int npow, cplx *__restrict__ A,
                                                         int lA, int c0, int TR, const int *__restrict__ perm) {
    extern __shared__ cplx tile[];                           // TR x (nb + 1): the pad keeps the column reads off one bank
    const int ld = nb + 1;
    const int tid = threadIdx.x;
    for (int64_t row0 = (int64_t)blockIdx.x * TR; row0 < d; row0 += (int64_t)gridDim.x * TR) {
        for (int e = tid; e < TR * nb; e += 256) {
            const int r = e / nb, col = e - r * nb;
            tile[r * ld + col] = (row0 + r < d) ? Xi[(size_t)(row0 + r) * nb + col] : cplx{0.0, 0.0};
        }
        __syncthreads();
        for (int idx = tid; idx < TR * l; idx += 256) {
            const int c = idx / TR, r = idx - c * TR;
            const int64_t row = row0 + r;
            if (row >= d) continue;
            for (int p0 = 0; p0 < npow; p0 += ACC_MAXP) {
                const int np = npow - p0 < ACC_MAXP ? npow - p0 : ACC_MAXP;
                cplx acc[ACC_MAXP];
#pragma unroll
                for (int p = 0; p < ACC_MAXP; ++p) acc[p] = cplx{0.0, 0.0};
                for (int s = 0; s < nsys; ++s) {
                    cplx t = cmul(w[s], tile[r * ld + s * l + c]);
                    const cplx zs = z[s];
                    for (int q = 0; q < p0; ++q) t = cmul(t, zs);
#pragma unroll
                    for (int p = 0; p < ACC_MAXP; ++p) {
                        if (p < np) { acc[p].x += t.x; acc[p].y += t.y; t = cmul(t, zs); }
                    }
                }
#pragma unroll
                for (int p = 0; p < ACC_MAXP; ++p) {
                    if (p < np) {
                        cplx *dst = A + ((size_t)(p0 + p) * lA + c0 + c) * d + (perm ? (int64_t)perm[row] : row);   // the moments are the caller's
                        const cplx a = *dst;
                        *dst = cplx{a.x + acc[p].x, a.y + acc[p].y};
                    }
                }
            }
        }
        __syncthreads();
    }
}
void launch_beyn_accum(const cplx *Xi, int nb, int64_t d, int l, int nsys, const cplx *w, const cplx *z, int npow, cplx *A, hipStream_t st,
                       int lA, int c0, const int *perm) {
    if (lA <= 0) lA = l;
    if (!d || nb < 1) return;
    if (nb > 256) throw WaeError(WAE_ERR_INVALID, "beyn_accum: nb must be in 1..256");
    int TR = 2048 / (nb + 1);                                // <= 32 KB of LDS
    if (TR > 32) TR = 32;
    if (TR < 1) TR = 1;
    const int64_t tiles = (d + TR - 1) / TR;
    const unsigned grid = (unsigned)std::min<int64_t>(tiles, 4096);
    hipLaunchKernelGGL(beyn_accum_kernel, dim3(grid), dim3(256), (size_t)TR * (nb + 1) * sizeof(cplx), st, Xi, nb, d, l, nsys, w, z, npow, A, lA, c0, TR, perm);
    HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------------
// The small-matrix half of the lock-step GMRES on the device (gmres.hip Gmres::run_device): one thread per column keeps that column's
// Hessenberg column, Givens rotations, residual estimate and convergence flags in HBM, so that no iteration ends in a
// device-to-host copy + stream synchronisation (round 1: 51 us of host turnaround per lock-step iteration).  The arithmetic is
// the host loop's, statement for statement (same rotations, same tests), hence the same iterates.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gmres_init_kernel(GmresDev S, const cplx *__restrict__ beta, const unsigned char *__restrict__ done, int use_mask) {
    __shared__ int act[256];
    const int b = threadIdx.x;
    int a = 0;
    if (b < S.nb) {
        S.g[b] = cplx{beta[b].x, 0.0};
        S.sv[b] = 1.0;
        S.vsq[b] = cplx{1.0, 0.0};
        S.conv[b] = done[b] ? 1 : 0;
        S.steps[b] = 0;
        a = done[b] ? 0 : 1;
    }
    act[b] = a;
    __syncthreads();
    if (b < (S.nb + 7) / 8) {
        int any = 0;
        for (int k = 0; k < 8; ++k) any |= act[b * 8 + k];
        S.cmask[b] = use_mask ? (unsigned char)any : (unsigned char)1;
    }
    if (b == 0) {
        int n = 0;
        for (int k = 0; k < S.nb; ++k) n += act[k];
        S.status[0] = n; S.status[1] = 0; S.status[2] = 0;
    }
}

// after Arnoldi step j: hd[i][b], i <= j: s_i^2-scaled dots of the new vector against the unnormalised basis; hd[j+1][b].x: norm of
// the orthogonalised vector (gmres.hip: "lazy" basis).  Produces the Hessenberg column of the normalised recurrence, rotates it,
// updates g, the residual estimate and the flags; marks vectors whose running scale left [1/lim, lim] for renormalisation.
__global__ __launch_bounds__(256) void gmres_step_kernel(GmresDev S, const cplx *__restrict__ hd, int j, double tol, double lim, int use_mask,
                                                         const cplx *__restrict__ rn) {
    __shared__ int act[256];
    const int b = threadIdx.x;
    const int nb = S.nb, m = S.m;
    int a = 0;
    if (b < nb) {
        const int nvj = j + 1;
        const double sj = S.sv[(size_t)j * nb + b];
        const double r = rn ? rn[b].x : hd[(size_t)nvj * nb + b].x;        // norm of the new (unnormalised) vector
        if (S.Hraw) {                                         // the unnormalised recurrence itself (read by the pair steps):
            cplx *Hr = S.Hraw + (size_t)j * (m + 1) * nb;     // Op v_j = sum_{i<=j} Hraw[j][i] v_i + sub[j] v_{j+1}
            for (int i = 0; i <= j; ++i) Hr[(size_t)i * nb + b] = hd[(size_t)i * nb + b];
        }
        double svn = r > 0.0 ? 1.0 / r : 0.0;
        const bool resc = svn > lim || (svn > 0.0 && svn < 1.0 / lim);
        S.rescale[b] = resc ? cplx{r, 0.0} : cplx{0.0, 0.0};
        if (S.sub) S.sub[(size_t)j * nb + b] = resc ? r : 1.0;
        if (resc) {                                          // the vector is normalised in place by gmres_rescale_kernel
            S.vsq[(size_t)nvj * nb + b] = cplx{svn > 0.0 ? 1.0 : 0.0, 0.0};
            svn = svn > 0.0 ? 1.0 : 0.0;
            atomicOr(&S.status[2], 1);
        }
        S.sv[(size_t)nvj * nb + b] = svn;
        if (!S.conv[b]) {
            cplx *Hc = S.R + (size_t)j * (m + 1) * nb;       // column j: entries i = 0..j+1 at Hc[i*nb + b]
            for (int i = 0; i <= j; ++i) {
                const double si = S.sv[(size_t)i * nb + b];
                const double f = si > 0.0 ? sj / si : 0.0;
                const cplx c = hd[(size_t)i * nb + b];
                Hc[(size_t)i * nb + b] = cplx{c.x * f, c.y * f};
            }
            Hc[(size_t)(j + 1) * nb + b] = cplx{sj * r, 0.0};
            for (int i = 0; i < j; ++i) {
                const cplx aa = Hc[(size_t)i * nb + b], bb = Hc[(size_t)(i + 1) * nb + b];
                const double c = S.cs[(size_t)i * nb + b];
                const cplx sn = S.sn[(size_t)i * nb + b];
                const cplx sb = cmul(sn, bb), ca = cmul(cconj(sn), aa);
                Hc[(size_t)i * nb + b] = cplx{c * aa.x + sb.x, c * aa.y + sb.y};
                Hc[(size_t)(i + 1) * nb + b] = cplx{-ca.x + c * bb.x, -ca.y + c * bb.y};
            }
            const cplx av = Hc[(size_t)j * nb + b];
            const double bv = Hc[(size_t)(j + 1) * nb + b].x;
            const double aabs = hypot(av.x, av.y);
            const double t = sqrt(aabs * aabs + bv * bv);
            if (!(t > 0.0) || isnan(t)) {
                S.conv[b] = 1;
                if (isnan(t)) atomicOr(&S.status[1], 1);
            } else {
                double c;
                cplx sn;
                if (aabs == 0.0) { c = 0.0; sn = cplx{1.0, 0.0}; }
                else { c = aabs / t; const double q = bv / t; sn = cplx{av.x / aabs * q, av.y / aabs * q}; }
                S.cs[(size_t)j * nb + b] = c;
                S.sn[(size_t)j * nb + b] = sn;
                Hc[(size_t)j * nb + b] = cplx{c * av.x + sn.x * bv, c * av.y + sn.y * bv};
                Hc[(size_t)(j + 1) * nb + b] = cplx{0.0, 0.0};
                const cplx gj = S.g[(size_t)j * nb + b];
                const cplx gn = cmul(cconj(sn), gj);
                S.g[(size_t)(j + 1) * nb + b] = cplx{-gn.x, -gn.y};
                S.g[(size_t)j * nb + b] = cplx{c * gj.x, c * gj.y};
                S.steps[b] = j + 1;
                S.iters[b] += 1;
                const double rr = hypot(gn.x, gn.y) / S.bnorm[b];
                S.relres[b] = rr;
                if (isnan(rr)) atomicOr(&S.status[1], 1);
                const int hs = S.histlen[b];
                if (hs < S.histcap) { S.hist[(size_t)hs * nb + b] = rr; S.histlen[b] = hs + 1; }
                const int hn = hs + 1;
                if (rr <= 0.7 * tol) S.conv[b] = 1;
                else if (hn > 60 && hs < S.histcap && rr > 0.9 * S.hist[(size_t)(hn - 31) * nb + b]) { S.conv[b] = 1; S.stalled[b] = 1; }   // attainable accuracy reached
                else a = 1;
            }
        }
    }
    act[b] = a;
    __syncthreads();
    if (b < (nb + 7) / 8 && use_mask) {
        int any = 0;
        for (int k = 0; k < 8; ++k) any |= act[b * 8 + k];
        S.cmask[b] = (unsigned char)any;
    }
    if (b == 0) {
        int n = 0;
        for (int k = 0; k < nb; ++k) n += act[k];
        S.status[0] = n;
    }
}

// y = R^-1 g per column over that column's steps; out[i][b] = s_i y_i (coefficients against the unnormalised basis), 0 beyond
__global__ __launch_bounds__(256) void gmres_solve_y_kernel(GmresDev S, int ju, cplx *__restrict__ out) {
    const int b = threadIdx.x;
    const int nb = S.nb, m = S.m;
    if (b >= nb) return;
    const int k = S.steps[b];
    for (int i = k; i < ju; ++i) out[(size_t)i * nb + b] = cplx{0.0, 0.0};
    for (int i = k - 1; i >= 0; --i) {
        cplx sacc = S.g[(size_t)i * nb + b];
        for (int q = i + 1; q < k; ++q) {
            const cplx hq = S.R[((size_t)q * (m + 1) + i) * nb + b];
            const cplx yq = out[(size_t)q * nb + b];
            sacc.x -= hq.x * yq.x - hq.y * yq.y;
            sacc.y -= hq.x * yq.y + hq.y * yq.x;
        }
        const cplx dg = S.R[((size_t)i * (m + 1) + i) * nb + b];
        out[(size_t)i * nb + b] = (dg.x != 0.0 || dg.y != 0.0) ? cdiv(sacc, dg) : cplx{0.0, 0.0};
    }
    for (int i = 0; i < k; ++i) {
        const double f = S.sv[(size_t)i * nb + b];
        cplx y = out[(size_t)i * nb + b];
        out[(size_t)i * nb + b] = cplx{f * y.x, f * y.y};
    }
}

// columns flagged by gmres_step_kernel: V[row][b] /= factor[b]  (every workgroup leaves at once when no column is flagged)
__global__ __launch_bounds__(256) void gmres_rescale_kernel(cplx *__restrict__ V, const cplx *__restrict__ factor, const int *__restrict__ status, size_t total, int nb) {
    if (!status[2]) return;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const double f = factor[e % nb].x;
        if (f > 0.0) { const cplx x = V[e]; V[e] = cplx{x.x / f, x.y / f}; }
    }
}
__global__ void gmres_clear_rescale_kernel(int *status) { status[2] = 0; }

void launch_gmres_init(const GmresDev &S, const cplx *beta, const unsigned char *done, int use_mask, hipStream_t st) {
    hipLaunchKernelGGL(gmres_init_kernel, dim3(1), dim3(256), 0, st, S, beta, done, use_mask);
    HIP_CHECK(hipGetLastError());
}
// One thread per column, ahead of the update pass of a pair step (after dots2): alpha = u1^H u2 / u1^H u1 from the Gram entries and
// the coefficients (u_k = w_k - V c_k), c2m = c2 - alpha c1, and the coefficients hd2 of Op v_{j+1} against the unnormalised basis
// v_0..v_{j+1}:  Op v_{j+1} = Op (w1 - V c1) = w2 - sum_k c1_k Op v_k,  w2 = V c2 + alpha v_{j+1} + v_{j+2}  and
// Op v_k = sum_{i<=k} Hraw[k][i] v_i + sub[k] v_{k+1} (column j of it being c1 itself, with sub[j] = 1).
__global__ __launch_bounds__(256) void gmres_pair_coef_kernel(GmresDev S, int j, const cplx *__restrict__ c1, const cplx *__restrict__ c2,
                                                              const cplx *__restrict__ gram, cplx *__restrict__ alpha, cplx *__restrict__ c2m,
                                                              cplx *__restrict__ hd2) {
    const int b = threadIdx.x;
    const int nb = S.nb, m = S.m;
    if (b >= nb) return;
    double uu = gram[b].x;
    cplx u12 = gram[(size_t)nb + b];
    for (int i = 0; i <= j; ++i) {
        const double q = S.vsq[(size_t)i * nb + b].x;
        const double w = q > 0.0 ? 1.0 / q : 0.0;             // ||v_i||^2
        const cplx a = c1[(size_t)i * nb + b], c = c2[(size_t)i * nb + b];
        uu -= (a.x * a.x + a.y * a.y) * w;
        u12.x -= (a.x * c.x + a.y * c.y) * w;                 // conj(a) c
        u12.y -= (a.x * c.y - a.y * c.x) * w;
    }
    cplx al = {0.0, 0.0};
    if (uu > 0.0 && uu > 1e-28 * gram[b].x) al = cplx{u12.x / uu, u12.y / uu};
    alpha[b] = al;
    cplx *Hj = S.Hraw + (size_t)j * (m + 1) * nb;
    for (int i = 0; i <= j; ++i) {
        const cplx a = c1[(size_t)i * nb + b], c = c2[(size_t)i * nb + b];
        Hj[(size_t)i * nb + b] = a;
        c2m[(size_t)i * nb + b] = cplx{c.x - (al.x * a.x - al.y * a.y), c.y - (al.x * a.y + al.y * a.x)};
    }
    S.sub[(size_t)j * nb + b] = 1.0;
    for (int i = 0; i <= j + 1; ++i) {
        cplx t = i <= j ? c2[(size_t)i * nb + b] : al;
        for (int k = i; k <= j; ++k) {
            const cplx hk = S.Hraw[((size_t)k * (m + 1) + i) * nb + b], ck = c1[(size_t)k * nb + b];
            t.x -= hk.x * ck.x - hk.y * ck.y;
            t.y -= hk.x * ck.y + hk.y * ck.x;
        }
        if (i >= 1) {
            const double sb = S.sub[(size_t)(i - 1) * nb + b];
            const cplx ck = c1[(size_t)(i - 1) * nb + b];
            t.x -= sb * ck.x;
            t.y -= sb * ck.y;
        }
        hd2[(size_t)i * nb + b] = t;
    }
}
void launch_gmres_pair_coef(const GmresDev &S, int j, const cplx *c1, const cplx *c2, const cplx *gram, cplx *alpha, cplx *c2m, cplx *hd2, hipStream_t st) {
    hipLaunchKernelGGL(gmres_pair_coef_kernel, dim3(1), dim3(256), 0, st, S, j, c1, c2, gram, alpha, c2m, hd2);
    HIP_CHECK(hipGetLastError());
}
void launch_gmres_step(const GmresDev &S, const cplx *hd, int j, double tol, double lim, int use_mask, cplx *Vnew, int64_t n, hipStream_t st,
                       const cplx *rn) {
    hipLaunchKernelGGL(gmres_step_kernel, dim3(1), dim3(256), 0, st, S, hd, j, tol, lim, use_mask, rn);
    hipLaunchKernelGGL(gmres_rescale_kernel, dim3(512), dim3(256), 0, st, Vnew, S.rescale, S.status, (size_t)n * S.nb, S.nb);
    hipLaunchKernelGGL(gmres_clear_rescale_kernel, dim3(1), dim3(1), 0, st, S.status);
    HIP_CHECK(hipGetLastError());
}
void launch_gmres_solve_y(const GmresDev &S, int ju, cplx *out, hipStream_t st) {
    hipLaunchKernelGGL(gmres_solve_y_kernel, dim3(1), dim3(256), 0, st, S, ju, out);
    HIP_CHECK(hipGetLastError());
}

__global__ __launch_bounds__(256) void triad_kernel(double2 *__restrict__ a, const double2 *__restrict__ b, const double2 *__restrict__ c, double s, size_t n2) {
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n2; e += (size_t)gridDim.x * 256) {
        double2 x = b[e], y = c[e];
        a[e] = double2{x.x + s * y.x, x.y + s * y.y};
    }
}
void launch_triad(double *a, const double *b, const double *c, double s_, int64_t n, hipStream_t st, unsigned grid_cap) {
    size_t n2 = (size_t)n / 2;
    hipLaunchKernelGGL(triad_kernel, dim3(grid_for(n2, grid_cap)), dim3(256), 0, st, (double2 *)a, (const double2 *)b, (const double2 *)c, s_, n2);
    HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------------
// Batched adjoint perturbation (perturb.hip perturb_batch_core): nb eigenpairs expanded in lock-step.  Every vector of the batch is
// interleaved [row][system] like the solver's multivectors; the input columns of the regrouped recurrence are U[row][t][system].
// ---------------------------------------------------------------------------------------------------
// U[row][t0 + t][b] (+)= sum_{i<k} G[i][t0 + t][b] * V_i[row][b],  t < tn <= TMAX;  V_i = V + i*stride, G: [k][T][nb].
// A stream over the series: thread t owns column t % nb and every R-th row (R = 256 / nb, as in dots_kernel), holds the tn outputs of
// its (row, column) in registers and reads V_i[row][b] ONCE for all of them; the k x tn x nb weights sit in LDS (the launcher cuts k so
// that they fit).  Four 16-B loads of the series in flight per lane.
constexpr int PTG_MAXW = 3072;      // weights per launch (48 KB of LDS)
template <int TMAX>
__global__ __launch_bounds__(256) void pt_gemm_batch_kernel(const cplx *__restrict__ V, size_t stride, int k, const cplx *__restrict__ G, int T, int t0,
                                                            int tn, cplx *__restrict__ U, int64_t d, int nb, int accumulate) {
    extern __shared__ cplx ptg_w[];                          // [k][tn][nb]
    const int tid = threadIdx.x;
    for (int e = tid; e < k * tn * nb; e += 256) {
        const int b = e % nb, it = e / nb, t = it % tn, i = it / tn;
        ptg_w[e] = G[((size_t)i * T + t0 + t) * nb + b];
    }
    __syncthreads();
    const int R = 256 / nb;
    const int b = tid % nb, rl = tid / nb;
    if (rl >= R) return;
    for (int64_t row = (int64_t)blockIdx.x * R + rl; row < d; row += (int64_t)gridDim.x * R) {
        const size_t e = (size_t)row * nb + b;
        cplx acc[TMAX];
#pragma unroll
        for (int t = 0; t < TMAX; ++t) acc[t] = cplx{0.0, 0.0};
        int i = 0;
        for (; i + 4 <= k; i += 4) {
            cplx v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = stream_load(V + (size_t)(i + u) * stride + e);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int t = 0; t < TMAX; ++t)
                    if (t < tn) cfma(acc[t], ptg_w[((i + u) * tn + t) * nb + b], v[u]);
        }
        for (; i < k; ++i) {
            const cplx v = stream_load(V + (size_t)i * stride + e);
#pragma unroll
            for (int t = 0; t < TMAX; ++t)
                if (t < tn) cfma(acc[t], ptg_w[(i * tn + t) * nb + b], v);
        }
        cplx *out = U + ((size_t)row * T + t0) * nb + b;
#pragma unroll
        for (int t = 0; t < TMAX; ++t)
            if (t < tn) {
                cplx a = acc[t];
                if (accumulate) { const cplx o = out[(size_t)t * nb]; a.x += o.x; a.y += o.y; }
                out[(size_t)t * nb] = a;
            }
    }
}
void launch_pt_gemm_batch(const cplx *V, size_t stride, int k, const cplx *G, cplx *U, int64_t d, int T, int nb, hipStream_t st) {
    if (nb < 1 || nb > 256 || k < 1 || T < 1) throw WaeError(WAE_ERR_INVALID, "pt_gemm_batch: nb in 1..256, k >= 1, T >= 1");
    const int R = 256 / nb;
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(2048, (d + R - 1) / R));
    for (int t0 = 0; t0 < T; t0 += 16) {
        const int tn = std::min(16, T - t0);
        const int kc = std::max(1, PTG_MAXW / (tn * nb));                  // series vectors per launch: their weights fill LDS
        for (int i0 = 0; i0 < k; i0 += kc) {
            const int kk = std::min(kc, k - i0);
            const size_t shm = (size_t)kk * tn * nb * sizeof(cplx);
            const cplx *Vc = V + (size_t)i0 * stride, *Gc = G + (size_t)i0 * T * nb;
            const int acc = i0 > 0;
            if (tn <= 4) hipLaunchKernelGGL(pt_gemm_batch_kernel<4>, dim3(grid), dim3(256), shm, st, Vc, stride, kk, Gc, T, t0, tn, U, d, nb, acc);
            else if (tn <= 8) hipLaunchKernelGGL(pt_gemm_batch_kernel<8>, dim3(grid), dim3(256), shm, st, Vc, stride, kk, Gc, T, t0, tn, U, d, nb, acc);
            else hipLaunchKernelGGL(pt_gemm_batch_kernel<16>, dim3(grid), dim3(256), shm, st, Vc, stride, kk, Gc, T, t0, tn, U, d, nb, acc);
            HIP_CHECK(hipGetLastError());
        }
    }
}

// out[row][b] = a[b] x[row][b] + c[b] y[row][b]  (coef = a[0..nb), c[0..nb) on the device; out may alias x or y).  A column whose two
// coefficients are both zero is WRITTEN as zero whatever x and y hold: a system that has been given up leaves no NaN behind.
__global__ __launch_bounds__(256) void pt_axpby_cols_kernel(const cplx *__restrict__ coef, const cplx *x, const cplx *y, cplx *out, int64_t d, int nb) {
    const int tid = threadIdx.x;
    const int R = 256 / nb;
    const int b = tid % nb, rl = tid / nb;
    if (rl >= R) return;
    const cplx a = coef[b], c = coef[nb + b];
    const bool dead = a.x == 0.0 && a.y == 0.0 && c.x == 0.0 && c.y == 0.0;
    for (int64_t row = (int64_t)blockIdx.x * R + rl; row < d; row += (int64_t)gridDim.x * R) {
        const size_t e = (size_t)row * nb + b;
        cplx r = {0.0, 0.0};
        if (!dead) { r = cmul(a, x[e]); cfma(r, c, y[e]); }
        out[e] = r;
    }
}
void launch_pt_axpby_cols(const cplx *coef, const cplx *x, const cplx *y, cplx *out, int64_t d, int nb, hipStream_t st) {
    if (nb < 1 || nb > 256) throw WaeError(WAE_ERR_INVALID, "pt_axpby_cols: nb in 1..256");
    const int R = 256 / nb;
    hipLaunchKernelGGL(pt_axpby_cols_kernel, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(4096, (d + R - 1) / R))), dim3(256), 0, st, coef, x, y,
                       out, d, nb);
    HIP_CHECK(hipGetLastError());
}

// The two projections of an order in one pass: vk[row][b] += (-dots[0][b] - 1/2 sum_{1<=j<nd} dots[j][b]) * v0[row][b]
// (dots[0] = v0^H [Y] v_k: perturbation.jl:425; dots[j] = v_j^H [Y] v_{k-j}: the normalisation sum of perturbation.jl:427-432; both
// corrections are multiples of v0, and the second does not involve v_k).  The coefficients never visit the host.
__global__ __launch_bounds__(256) void pt_project_kernel(cplx *__restrict__ vk, const cplx *__restrict__ v0, const cplx *__restrict__ dots, int nd,
                                                         int64_t d, int nb) {
    const int tid = threadIdx.x;
    const int R = 256 / nb;
    const int b = tid % nb, rl = tid / nb;
    if (rl >= R) return;
    cplx c = dots[b];
    c.x = -c.x; c.y = -c.y;
    for (int j = 1; j < nd; ++j) { const cplx t = dots[(size_t)j * nb + b]; c.x -= 0.5 * t.x; c.y -= 0.5 * t.y; }
    for (int64_t row = (int64_t)blockIdx.x * R + rl; row < d; row += (int64_t)gridDim.x * R) {
        const size_t e = (size_t)row * nb + b;
        cplx v = vk[e];
        cfma(v, c, v0[e]);
        vk[e] = v;
    }
}
void launch_pt_project(cplx *vk, const cplx *v0, const cplx *dots, int nd, int64_t d, int nb, hipStream_t st) {
    if (nb < 1 || nb > 256 || nd < 1) throw WaeError(WAE_ERR_INVALID, "pt_project: nb in 1..256, nd >= 1");
    const int R = 256 / nb;
    hipLaunchKernelGGL(pt_project_kernel, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(4096, (d + R - 1) / R))), dim3(256), 0, st, vk, v0, dots, nd,
                       d, nb);
    HIP_CHECK(hipGetLastError());
}
