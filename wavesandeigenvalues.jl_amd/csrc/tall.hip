// libwaehip.so -- wae_tall_* (include/waehip.h, "tall matrices"): the tall-skinny half of the step that turns Beyn's moments into
// eigenpairs (beyn.jl:76-107, moments2eigs at beyn.jl:289-323).  A wae_tall is a column-major rows x ncols complex matrix in HBM, in
// the caller's row numbering, independent of any family; the three kernels below are all the device work of that step:
//   tall_gram_kernel    G = X^H Y     (rows 1e5..1e7, 1..64 columns per side): per-workgroup partials, then a fixed-order sum
//   tall_mul_kernel     dst = beta dst + alpha src C   (C small, read through the scalar cache)
//   tall_hankel_kernel  the block Hankel matrices B0 / B1 of beyn.jl:76-90, a gather copy
// The small (lK x lK) eigen / singular value problems stay with the host language's LAPACK, as the Arnoldi entries leave theirs.
// Every entry returns with its result complete: the work runs on one stream per device, synchronised before the return.
#include <memory>
#include <mutex>

#include "family.h"
#include "kernel_helpers.h"

struct wae_tall {
    int device = 0;
    int64_t rows = 0;
    int32_t ncols = 0;
    DevBuf<cplx> buf;                       // rows x ncols, leading dimension rows
    mutable DevBuf<cplx> partial, small;    // scratch of wae_tall_gram (first-stage partials, G; in its FIRST operand) and of wae_tall_mul (C; in
                                            // dst), grow-only: why a handle, also a const one, takes one call at a time (include/waehip.h)
};

namespace {
constexpr int GT = 16;          // a workgroup of tall_gram_kernel owns a GT x GT block of G ...
constexpr int GR = 64;          // ... and stages GR rows of its 2 GT columns in LDS per step (2 x 16 KB)
constexpr int GBLOCKS = 768;    // workgroups over the rows, summed over the blocks of G, while every block keeps at least 64 of them: the
                                // kernel takes 156 registers = 3 workgroups per CU, so up to 16 x 16 columns (768) and at 32 x 32 (4 x 192)
                                // the grid is one resident round; a 64 x 64 Gram runs 16 x 64 = 1024 workgroups, a round and a third

// G block (ti, tj) = X[:, ti*GT ..]^H Y[:, tj*GT ..]: partial[((ti * ntj + tj) * nblk + blk) * GT*GT + i * GT + j] = the sum over the rows
// of this workgroup's tiles.  Thread t: lane r = t % 16 takes every 16th row of the staged tile, group g = t / 16 the 4 x 4 outputs
// i = 4 (g % 4) .., j = 4 (g / 4) .. in registers: 8 LDS reads of 16 bytes for 16 complex multiply-adds.  The 16 lanes of a group read
// consecutive entries of one staged column; the four groups of a wavefront read columns that lie 4 KB apart, i.e. the same banks --
// whether the 16-byte reads of different groups collide there has not been measured (no LDS counters taken).  The next tile's global
// loads are issued before the current tile is consumed.  X and Y blocks that are the same columns of the same matrix (the diagonal
// blocks of X^H X) are staged once.  Rows and columns beyond the matrix are staged as zeros.
__global__ __launch_bounds__(256) void tall_gram_kernel(const cplx *__restrict__ A, size_t lda, int na, const cplx *__restrict__ B, size_t ldb,
                                                        int nb, int64_t rows, cplx *__restrict__ partial) {
    __shared__ cplx sX[GT][GR], sY[GT][GR];
    const int tid = threadIdx.x, rl = tid & 15, og = tid >> 4;
    const int i0 = (og & 3) * 4, j0 = (og >> 2) * 4;
    const int ti = blockIdx.y, tj = blockIdx.z;
    const int wi = min(GT, na - ti * GT), wj = min(GT, nb - tj * GT);
    const cplx *Ab = A + (size_t)ti * GT * lda, *Bb = B + (size_t)tj * GT * ldb;
    const bool alias = Ab == Bb && wi == wj;
    cplx acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = cplx{0.0, 0.0};
    const int64_t ntiles = (rows + GR - 1) / GR;
    const int sr = tid & (GR - 1), sc = tid >> 6;           // staging: entry k of this thread is row sr of column sc + 4k
    cplx px[4], py[4];
    auto fetch = [&](int64_t t) {
        const int64_t r = t * GR + sr;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = sc + 4 * k;
            px[k] = (r < rows && c < wi) ? Ab[(size_t)c * lda + (size_t)r] : cplx{0.0, 0.0};
            if (!alias) py[k] = (r < rows && c < wj) ? Bb[(size_t)c * ldb + (size_t)r] : cplx{0.0, 0.0};
        }
    };
    int64_t t = blockIdx.x;
    if (t < ntiles) fetch(t);
    for (; t < ntiles; t += gridDim.x) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            sX[sc + 4 * k][sr] = px[k];
            if (!alias) sY[sc + 4 * k][sr] = py[k];
        }
        __syncthreads();
        if (t + gridDim.x < ntiles) fetch(t + gridDim.x);
        const cplx(*Y)[GR] = alias ? sX : sY;
#pragma unroll 1
        for (int rr = 0; rr < GR; rr += 16) {        // (unrolled, the operands of all four steps are live at once: 184 registers)
            cplx x[4], y[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) x[a] = sX[i0 + a][rr + rl];
#pragma unroll
            for (int b = 0; b < 4; ++b) y[b] = Y[j0 + b][rr + rl];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {                 // acc += conj(x) y
                    acc[a][b].x = fma(x[a].x, y[b].x, acc[a][b].x); acc[a][b].x = fma(x[a].y, y[b].y, acc[a][b].x);
                    acc[a][b].y = fma(x[a].x, y[b].y, acc[a][b].y); acc[a][b].y = fma(-x[a].y, y[b].x, acc[a][b].y);
                }
        }
        __syncthreads();
    }
    // the 16 lanes of a group: xor butterfly (the same tree in every launch), lane 0 writes the group's 16 sums
    cplx *out = partial + ((size_t)(ti * gridDim.z + tj) * gridDim.x + blockIdx.x) * (GT * GT);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            cplx v = acc[a][b];
#pragma unroll
            for (int m = 8; m >= 1; m >>= 1) { v.x += __shfl_xor(v.x, m); v.y += __shfl_xor(v.y, m); }
            if (rl == 0) out[(i0 + a) * GT + j0 + b] = v;
        }
}

// second stage: G[ci + i, cj + j] = sum over the nblk partials of block (ti, tj), 16 slices of the partials per output added in index
// order, then an LDS tree over the slices: one fixed order.  Workgroup (i, ti * ntj + tj) sums row i of the block.
__global__ __launch_bounds__(256) void tall_gram_reduce_kernel(const cplx *__restrict__ partial, int nblk, int ntj, int na, int nb,
                                                               cplx *__restrict__ G) {
    __shared__ cplx sm[256];
    const int j = threadIdx.x & 15, slice = threadIdx.x >> 4, i = blockIdx.x, sub = blockIdx.y;
    const cplx *p = partial + (size_t)sub * nblk * (GT * GT) + i * GT + j;
    cplx acc = {0.0, 0.0};
    for (int k = slice; k < nblk; k += 16) { const cplx v = p[(size_t)k * (GT * GT)]; acc.x += v.x; acc.y += v.y; }
    sm[threadIdx.x] = acc;
    __syncthreads();
#pragma unroll
    for (int s = 8; s >= 1; s >>= 1) {
        if (slice < s) { sm[threadIdx.x].x += sm[threadIdx.x + s * 16].x; sm[threadIdx.x].y += sm[threadIdx.x + s * 16].y; }
        __syncthreads();
    }
    const int gi = (sub / ntj) * GT + i, gj = (sub % ntj) * GT + j;
    if (slice == 0 && gi < na && gj < nb) G[(size_t)gj * na + gi] = sm[threadIdx.x];
}

// dst[r, jb + j] = beta dst[r, jb + j] + sum_i src[r, i] C[i][jb + j], jb = JT blockIdx.y: one thread per row (16-byte accesses,
// consecutive rows over the lanes), JT accumulators in registers, one pass over the ns source columns and one over the JT destination
// columns.  C: [ns][ncp] with alpha folded in and the columns padded with zeros to ncp = a multiple of JT; its address is the same in
// every lane, so it is read through the scalar cache.  use_beta = 0: dst is not read.
template <int JT>
__global__ __launch_bounds__(256) void tall_mul_kernel(const cplx *__restrict__ src, size_t lds, int ns, const cplx *__restrict__ C, int ncp,
                                                       cplx *__restrict__ dst, size_t ldd, int nc, int64_t rows, cplx beta, int use_beta) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const int jb = blockIdx.y * JT;
    cplx acc[JT];
#pragma unroll
    for (int j = 0; j < JT; ++j) acc[j] = cplx{0.0, 0.0};
    const cplx *s = src + (size_t)r, *c = C + jb;
#pragma unroll 4
    for (int i = 0; i < ns; ++i) {
        const cplx x = s[(size_t)i * lds];
#pragma unroll
        for (int j = 0; j < JT; ++j) cfma(acc[j], x, c[(size_t)i * ncp + j]);
    }
#pragma unroll
    for (int j = 0; j < JT; ++j)
        if (jb + j < nc) {
            cplx *p = dst + (size_t)(jb + j) * ldd + (size_t)r;
            cplx v = acc[j];
            if (use_beta) cfma(v, beta, *p);
            *p = v;
        }
}

// dst[i d + r, j l + c] = mom[r, (i + j + shift) l + c]: workgroup (x, j l + c, i) copies 256 rows of one column block
__global__ __launch_bounds__(256) void tall_hankel_kernel(const cplx *__restrict__ mom, int64_t d, int l, int shift, cplx *__restrict__ dst,
                                                          size_t ldd) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= d) return;
    const int col = blockIdx.y, i = blockIdx.z, j = col / l, c = col % l;
    dst[(size_t)col * ldd + (size_t)i * (size_t)d + (size_t)r] = mom[((size_t)(i + j + shift) * l + c) * (size_t)d + (size_t)r];
}

// one stream per device for all tall matrices (created at first use, kept for the life of the process)
hipStream_t tall_stream(int device) {
    static std::mutex mu;
    static hipStream_t streams[64] = {nullptr};
    std::lock_guard<std::mutex> lock(mu);
    if (!streams[device]) HIP_CHECK(hipStreamCreateWithFlags(&streams[device], hipStreamNonBlocking));
    return streams[device];
}
bool cols_ok(const wae_tall *m, int32_t c0, int32_t n) { return c0 >= 0 && n >= 0 && (int64_t)c0 + n <= m->ncols; }
}   // namespace

extern "C" int wae_tall_create(wae_tall **out, int32_t device, int64_t rows, int32_t ncols) {
    return guarded([&]() {
        WAE_REQUIRE(out, "wae_tall_create: null output pointer");
        *out = nullptr;
        WAE_REQUIRE(rows >= 1 && rows <= ((int64_t)1 << 38) && ncols >= 1 && ncols <= (1 << 20), "wae_tall_create: rows in 1..2^38, ncols in 1..2^20");
        int ndev = 0;
        HIP_CHECK(hipGetDeviceCount(&ndev));
        WAE_REQUIRE(device >= 0 && device < ndev && device < 64, "wae_tall_create: no such device");
        HIP_CHECK(hipSetDevice(device));
        std::unique_ptr<wae_tall> m(new wae_tall);
        m->device = device; m->rows = rows; m->ncols = ncols;
        const size_t count = (size_t)rows * (size_t)ncols;
        m->buf.alloc(count);
        hipStream_t st = tall_stream(device);
        HIP_CHECK(hipMemsetAsync(m->buf.p, 0, count * sizeof(cplx), st));
        HIP_CHECK(hipStreamSynchronize(st));
        *out = m.release();
        return WAE_OK;
    });
}

extern "C" int wae_tall_destroy(wae_tall *m) {
    return guarded([&]() {
        if (m) { (void)hipSetDevice(m->device); delete m; }
        return WAE_OK;
    });
}

extern "C" int wae_tall_info(const wae_tall *m, int64_t *rows, int32_t *ncols, uint64_t *dev_ptr) {
    return guarded([&]() {
        WAE_REQUIRE(m, "wae_tall_info: null handle");
        if (rows) *rows = m->rows;
        if (ncols) *ncols = m->ncols;
        if (dev_ptr) *dev_ptr = (uint64_t)(uintptr_t)m->buf.p;
        return WAE_OK;
    });
}

// host <-> device copies of a sub-block: whole columns in one copy, otherwise one copy per column
static int tall_copy(const wae_tall *m, int64_t row0, int64_t nrows, int32_t col0, int32_t ncols, double *X, bool to_device, const char *what) {
    return guarded([&]() {
        WAE_REQUIRE(m, std::string(what) + ": null handle");
        WAE_REQUIRE(row0 >= 0 && nrows >= 0 && nrows <= m->rows && row0 <= m->rows - nrows && cols_ok(m, col0, ncols),
                    std::string(what) + ": the block lies outside the matrix");
        if (nrows == 0 || ncols == 0) return WAE_OK;
        WAE_REQUIRE(X, std::string(what) + ": null host array");
        HIP_CHECK(hipSetDevice(m->device));
        hipStream_t st = tall_stream(m->device);
        cplx *h = (cplx *)X;
        const bool whole = nrows == m->rows;
        const int ncopies = whole ? 1 : ncols;
        const size_t per = (whole ? (size_t)nrows * ncols : (size_t)nrows) * sizeof(cplx);
        for (int c = 0; c < ncopies; ++c) {
            cplx *dp = m->buf.p + (size_t)(col0 + c) * (size_t)m->rows + (size_t)row0, *hp = h + (size_t)c * (size_t)nrows;
            if (to_device) HIP_CHECK(hipMemcpyAsync(dp, hp, per, hipMemcpyHostToDevice, st));
            else HIP_CHECK(hipMemcpyAsync(hp, dp, per, hipMemcpyDeviceToHost, st));
        }
        HIP_CHECK(hipStreamSynchronize(st));
        return WAE_OK;
    });
}
extern "C" int wae_tall_write(wae_tall *m, int64_t row0, int64_t nrows, int32_t col0, int32_t ncols, const double *X) {
    return tall_copy(m, row0, nrows, col0, ncols, const_cast<double *>(X), true, "wae_tall_write");
}
extern "C" int wae_tall_read(const wae_tall *m, int64_t row0, int64_t nrows, int32_t col0, int32_t ncols, double *X) {
    return tall_copy(m, row0, nrows, col0, ncols, X, false, "wae_tall_read");
}

extern "C" int wae_tall_gram(const wae_tall *a, int32_t a_col0, int32_t na, const wae_tall *b, int32_t b_col0, int32_t nb, double *G_out) {
    return guarded([&]() {
        WAE_REQUIRE(a && b, "wae_tall_gram: null handle");
        WAE_REQUIRE(na >= 0 && na <= WAE_TALL_MAXCOLS && nb >= 0 && nb <= WAE_TALL_MAXCOLS, "wae_tall_gram: widths must lie in 0..WAE_TALL_MAXCOLS");
        WAE_REQUIRE(cols_ok(a, a_col0, na) && cols_ok(b, b_col0, nb), "wae_tall_gram: a column range lies outside its matrix");
        WAE_REQUIRE(a->rows == b->rows && a->device == b->device, "wae_tall_gram: the matrices differ in rows or device");
        if (na == 0 || nb == 0) return WAE_OK;
        WAE_REQUIRE(G_out, "wae_tall_gram: null output array");
        HIP_CHECK(hipSetDevice(a->device));
        hipStream_t st = tall_stream(a->device);
        const int nti = (na + GT - 1) / GT, ntj = (nb + GT - 1) / GT;
        const int64_t ntiles = (a->rows + GR - 1) / GR;
        const int nblk = (int)std::min<int64_t>(ntiles, std::max(64, GBLOCKS / (nti * ntj)));
        const size_t npart = (size_t)nti * ntj * nblk * (GT * GT);
        if (a->partial.n < npart) a->partial.alloc(npart);
        if (a->small.n < (size_t)WAE_TALL_MAXCOLS * WAE_TALL_MAXCOLS) a->small.alloc((size_t)WAE_TALL_MAXCOLS * WAE_TALL_MAXCOLS);
        hipLaunchKernelGGL(tall_gram_kernel, dim3(nblk, nti, ntj), dim3(256), 0, st, a->buf.p + (size_t)a_col0 * (size_t)a->rows, (size_t)a->rows, na,
                           b->buf.p + (size_t)b_col0 * (size_t)b->rows, (size_t)b->rows, nb, a->rows, a->partial.p);
        HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(tall_gram_reduce_kernel, dim3(GT, nti * ntj), dim3(256), 0, st, a->partial.p, nblk, ntj, na, nb, a->small.p);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(G_out, a->small.p, (size_t)na * nb * sizeof(cplx), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        return WAE_OK;
    });
}

extern "C" int wae_tall_mul(wae_tall *dst, int32_t dst_col0, const wae_tall *src, int64_t src_row0, int32_t src_col0, int32_t ns, const double *C,
                            int32_t nc, const double *alpha, const double *beta) {
    return guarded([&]() {
        WAE_REQUIRE(dst && src, "wae_tall_mul: null handle");
        WAE_REQUIRE(ns >= 0 && ns <= WAE_TALL_MAXCOLS && nc >= 0 && nc <= WAE_TALL_MAXCOLS, "wae_tall_mul: widths must lie in 0..WAE_TALL_MAXCOLS");
        WAE_REQUIRE(cols_ok(dst, dst_col0, nc) && cols_ok(src, src_col0, ns), "wae_tall_mul: a column range lies outside its matrix");
        WAE_REQUIRE(src_row0 >= 0 && dst->rows <= src->rows && src_row0 <= src->rows - dst->rows, "wae_tall_mul: the source rows lie outside the source");
        WAE_REQUIRE(dst->device == src->device, "wae_tall_mul: the matrices are on different devices");
        WAE_REQUIRE(dst != src || dst_col0 + nc <= src_col0 || src_col0 + ns <= dst_col0, "wae_tall_mul: source and destination columns overlap");
        if (ns == 0 || nc == 0) return WAE_OK;
        WAE_REQUIRE(C && alpha && beta, "wae_tall_mul: null coefficient array");
        HIP_CHECK(hipSetDevice(dst->device));
        hipStream_t st = tall_stream(dst->device);
        const int JT = nc <= 4 ? 4 : nc <= 8 ? 8 : 16;
        const int ncp = (nc + JT - 1) / JT * JT;
        const zc al(alpha[0], alpha[1]);
        std::vector<cplx> Cp((size_t)ns * ncp, cplx{0.0, 0.0});         // [i][j], alpha folded in
        for (int j = 0; j < nc; ++j)
            for (int i = 0; i < ns; ++i) {
                const zc v = al * zc(C[2 * ((size_t)j * ns + i)], C[2 * ((size_t)j * ns + i) + 1]);
                Cp[(size_t)i * ncp + j] = cplx{v.real(), v.imag()};
            }
        if (dst->small.n < (size_t)WAE_TALL_MAXCOLS * WAE_TALL_MAXCOLS) dst->small.alloc((size_t)WAE_TALL_MAXCOLS * WAE_TALL_MAXCOLS);
        HIP_CHECK(hipMemcpyAsync(dst->small.p, Cp.data(), Cp.size() * sizeof(cplx), hipMemcpyHostToDevice, st));
        const cplx be{beta[0], beta[1]};
        const int use_beta = (beta[0] != 0.0 || beta[1] != 0.0) ? 1 : 0;
        const cplx *sp = src->buf.p + (size_t)src_col0 * (size_t)src->rows + (size_t)src_row0;
        cplx *dp = dst->buf.p + (size_t)dst_col0 * (size_t)dst->rows;
        const dim3 grid((unsigned)((dst->rows + 255) / 256), ncp / JT);
#define WAE_TALL_MUL(J) hipLaunchKernelGGL(tall_mul_kernel<J>, grid, dim3(256), 0, st, sp, (size_t)src->rows, ns, dst->small.p, ncp, dp, (size_t)dst->rows, \
                                           nc, dst->rows, be, use_beta)
        if (JT == 4) WAE_TALL_MUL(4);
        else if (JT == 8) WAE_TALL_MUL(8);
        else WAE_TALL_MUL(16);
#undef WAE_TALL_MUL
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(st));                            // (Cp is a stack vector)
        return WAE_OK;
    });
}

extern "C" int wae_tall_hankel(wae_tall *dst, const wae_tall *moments, int32_t l, int32_t K, int32_t shift) {
    return guarded([&]() {
        WAE_REQUIRE(dst && moments, "wae_tall_hankel: null handle");
        WAE_REQUIRE(dst != moments && dst->device == moments->device, "wae_tall_hankel: the matrices must be two matrices on one device");
        WAE_REQUIRE(l >= 1 && K >= 1 && (shift == 0 || shift == 1) && (int64_t)l * K <= 65535 && K <= 65535, "wae_tall_hankel: bad l, K or shift");
        WAE_REQUIRE(moments->ncols == (int64_t)l * 2 * K && dst->ncols == (int64_t)l * K && dst->rows == moments->rows * K,
                    "wae_tall_hankel: moments must be d x (l*2K) and dst (d*K) x (l*K)");
        HIP_CHECK(hipSetDevice(dst->device));
        hipStream_t st = tall_stream(dst->device);
        const int64_t d = moments->rows;
        hipLaunchKernelGGL(tall_hankel_kernel, dim3((unsigned)((d + 255) / 256), l * K, K), dim3(256), 0, st, moments->buf.p, d, l, shift, dst->buf.p,
                           (size_t)dst->rows);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(st));
        return WAE_OK;
    });
}
