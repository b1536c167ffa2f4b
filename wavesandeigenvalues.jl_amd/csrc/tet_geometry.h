// Geometry of the straight-sided tetrahedron that every element order shares (assemble.hip, assemble_p2.hip, assemble_herm.hip): the
// coordinate transformation x = p3 + J xi (CooTrafo, src/FEM/FEM.jl:9-21) with its inverse and determinant, |det J| of a list of
// tetrahedra, and what the flame entries do before they form their own g.  The expressions and their order fix the bits of every
// element matrix: change them only with dev/mesh_entries_digest.py at hand.  Indexed by literals and unrolled counters only, so that
// J, Ji and G stay in registers.
#pragma once
#include "mesh_host.h"

// X[a] = the point of corner a, the first four entries of a connectivity row (of 4, 10 or 20 nodes)
__host__ __device__ inline void tet_corners(const double *__restrict__ pts, const int *__restrict__ nodes, double X[4][3]) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int k = 0; k < 3; ++k) X[a][k] = pts[(size_t)nodes[a] * 3 + k];
}

// J[i][j] = X[j][i] - X[3][i], Ji = J^-1 (cofactors over det J); returns det J
__host__ __device__ inline double tet_jacobian(const double X[4][3], double J[3][3], double Ji[3][3]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) J[i][j] = X[j][i] - X[3][i];
    const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
    const double c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2];
    const double c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
    const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
    const double id = 1.0 / det;
    Ji[0][0] = c00 * id; Ji[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) * id; Ji[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) * id;
    Ji[1][0] = c01 * id; Ji[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) * id; Ji[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) * id;
    Ji[2][0] = c02 * id; Ji[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) * id; Ji[2][2] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) * id;
    return det;
}

// G[a] = grad l_a of the barycentric coordinates (l_4 = 1 - l_1 - l_2 - l_3, corner 4 is the origin): G[0..2] the rows of J^-1,
// G[3] = -(G[0] + G[1] + G[2]); returns det J
__host__ __device__ inline double tet_gradients(const double X[4][3], double G[4][3]) {
    double J[3][3];
    const double det = tet_jacobian(X, J, G);
    for (int k = 0; k < 3; ++k) G[3][k] = -(G[0][k] + G[1][k] + G[2][k]);
    return det;
}

// |det J| of the listed tetrahedra, conn holding STRIDE nodes per tetrahedron (volume source S_a = |det J|/24 per node, FEM.jl:2429-2431;
// flame volume = sum |det J| / 6)
template <int STRIDE>
__global__ __launch_bounds__(256) void tet_det_kernel(const double *__restrict__ pts, const int *__restrict__ conn, const int *__restrict__ list, int64_t n,
                                                      double *__restrict__ adet) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double X[4][3], J[3][3], Ji[3][3];
    tet_corners(pts, conn + (int64_t)list[i] * STRIDE, X);
    adet[i] = fabs(tet_jacobian(X, J, Ji));
}

// What the flame entries share between their argument checks and their own g (Helmholtz.jl:19-33,325,477-483), in this order: the list
// of flame tetrahedra goes up, adet = their |det J|, the flame volume (WaeError if it is not positive) goes to *volume_out (may be NULL),
// nlocal = nglobal_scaled / volume, X = the corners of the reference tetrahedron from the host arrays.
// dpts, dconn: the points and the connectivity (STRIDE nodes per tetrahedron) on the device.
template <int STRIDE> struct FlameSetup {
    Dev<int> list;
    Dev<double> adet;
    double nlocal = 0.0, X[4][3];
    FlameSetup(const double *dpts, const int *dconn, int64_t nflame, const int32_t *flame_tets, double nglobal_scaled, double *volume_out,
               const double *points, const int32_t *tets, int32_t ref_tet)
        : list(flame_tets, (size_t)nflame), adet((size_t)nflame) {
        hipLaunchKernelGGL(tet_det_kernel<STRIDE>, grid_for(nflame), dim3(256), 0, 0, dpts, dconn, list.p, nflame, adet.p);
        HIP_CHECK(hipGetLastError());
        const double volume = flame_volume(adet, nflame);
        if (volume_out) *volume_out = volume;
        nlocal = nglobal_scaled / volume;
        tet_corners(points, tets + (size_t)ref_tet * 4, X);
    }
};
