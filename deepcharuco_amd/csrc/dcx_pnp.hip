// dcx_pnp.hip -- solve_pnp (/root/reference/src/inference.py:15-29, cv2.solvePnP with default flags) on the device, read straight
// from the corner pool dcx_infer_batch writes.  The steps (all fp64) are restated readably in deepcharuco_amd/pnp.py
// (solve_pnp_host), which is the pin of this kernel:
//   undistortPoints (5 fixed-point rounds) -> planar DLT homography on Hartley-normalised points (9x9 normal matrix, smallest
//   eigenvector by cyclic Jacobi) -> OpenCV's homography decomposition, orthonormalised by the polar factor (3x3 Jacobi) ->
//   Levenberg-Marquardt on the pixel reprojection error (6 parameters, analytic Jacobian, Marquardt damping, OpenCV's CvLevMarq
//   acceptance and stopping rule: 20 accepted steps, |dp| / |p| < FLT_EPSILON).
//
// One 64-lane wavefront per frame.  Lanes stride over the frame's points (no cap on their number); every per-point sum (centroids,
// the 45 entries of the DLT normal matrix, the 21 + 6 + 1 of JtJ / Jtr / cost) is reduced by a __shfl_xor butterfly, after which
// every lane holds the same bits (each pairwise add is commutative), so every lane runs the small dense solves (Jacobi, Cholesky)
// redundantly and takes the same branches: no LDS, no barrier.  The exception is the 9x9 Jacobi's eigenvector matrix: lane j keeps
// row j of V (a rotation mixes two entries of every row, so no lane needs another's data), which keeps it out of 81 registers.
// K and the distortion coefficients are kernel arguments (captured by value in a hipGraph); no allocation, no synchronisation.
// The solver itself is dcx_pnp_dev.h (solve and what it calls) on dcx_camera_dev.h (camera model, rotations) and dcx_mat_dev.h
// (Jacobi, Cholesky, the butterfly).  The entry's pool arguments pass that header's host check corner_pool(); the kernel reads the
// pool as the header's CornerPool.
#include "dcx_pnp_dev.h"

namespace {

// The pool arrives as loose __restrict__ parameters and becomes a CornerPool here: passed as the struct, the kernels of this unit and
// of dcx_pnp_ransac.hip measured 1 - 3 % slower.
__global__ __launch_bounds__(kLanes) void dcx_solve_pnp_kernel(
    const int32_t* __restrict__ counts, const int32_t* __restrict__ starts, const int32_t* __restrict__ rows,
    const float* __restrict__ xy, int pool, int n_ids, int rm1, double square_len, PnpCamera cam, int32_t* __restrict__ status,
    double* __restrict__ pose) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const CornerPool pl{counts, starts, rows, xy, pool, n_ids, rm1, square_len};
    const int n = pl.counts[b], s0 = pl.starts[b];
    double out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // The header's frame_status(), spelt out: through the call this kernel's code generation moves (the compiler shares one large-
    // argument sine reduction less, four registers and eight SGPR spills more).  A change there is a change here.
    int st;
    if (n <= 0) {
        st = DCX_PNP_TOO_FEW;
    } else if (s0 < 0 || (long long)s0 + n > (long long)pl.pool) {
        st = DCX_PNP_TRUNCATED;               // (its slots are not read)
    } else if (n < 4) {
        st = DCX_PNP_TOO_FEW;
    } else {
        bool bad = false;
        for (int i = lane; i < n; i += kLanes) {
            const int id = pl.rows[4 * ((long long)s0 + i) + 2];
            bad |= id < 0 || id >= pl.n_ids;
        }
        if (__any(bad)) {
            st = DCX_PNP_BAD_ID;
        } else {
            st = solve(pl.frame(n, s0), cam, out);
            if (st != DCX_PNP_OK) {
#pragma unroll
                for (int i = 0; i < 8; ++i) out[i] = 0.0;
            }
        }
    }
    if (lane == 0) {
        status[b] = st;
#pragma unroll
        for (int i = 0; i < 8; ++i) pose[8 * (long long)b + i] = out[i];
    }
}

}  // namespace

extern "C" int dcx_solve_pnp_pool(const int32_t* d_counts, const int32_t* d_starts, const int32_t* d_rows, const float* d_xy, int batch,
                                  int pool, int col_count, int row_count, double square_len, const double* h_camera9,
                                  const double* h_dist, int n_dist, int32_t* d_status, double* d_pose, void* stream) {
    CornerPool pl;
    PnpCamera cam;
    if (!corner_pool(d_counts, d_starts, d_rows, d_xy, batch, pool, col_count, row_count, square_len, pl)) return DCX_E_ARG;
    if (!h_camera9 || !d_status || !d_pose || !pnp_camera(h_camera9, h_dist, n_dist, cam)) return DCX_E_ARG;
    hipLaunchKernelGGL(dcx_solve_pnp_kernel, dim3((unsigned)batch), dim3(kLanes), 0, (hipStream_t)stream, pl.counts, pl.starts, pl.rows,
                       pl.xy, pl.pool, pl.n_ids, pl.rm1, pl.square_len, cam, d_status, d_pose);
    return (int)hipGetLastError();
}
