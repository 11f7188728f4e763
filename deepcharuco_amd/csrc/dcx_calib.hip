// dcx_calib.hip -- cv2.calibrateCamera (default flags) for a planar board, on the device, read straight from the corner pool
// dcx_infer_batch writes (the views of a ChArUco board: id-labelled corners).  The steps (all fp64) are restated readably in
// deepcharuco_amd/calib.py (calibrate_camera_host_full), which is the pin of these kernels:
//   per-view checks -> initIntrinsicParams2D (principal point at the centre, per-view DLT homography, two rows per view in
//   (1/fx^2, 1/fy^2), least squares) -> every view's pose by the PnP solver (solve(), K0, no distortion) -> joint
//   Levenberg-Marquardt over theta = (fx, fy, cx, cy, k1, k2, p1, p2, k3) and every used view's (rvec, tvec), CvLevMarq's rules,
//   at most 30 accepted steps, stop at |dp| / |p| < DBL_EPSILON.
//
// This unit holds the start (Zhang's), one 64-lane wave per view unless noted; grid = batch:
//   init_views      per-view checks, the view's homography, its two init rows
//   init_reduce     (one workgroup) the rows reduced, the 2x2 least squares -> K0
//   init_poses      solve() with K0 and zero distortion
// and the C entries.  The joint solve behind it (evaluate, schur, reduce_solve, trial, decide, the host loop, the workspace) is
// dcx_calib_dev.h's, instantiated on PinholeCalib; what it shares with the other solvers, its fixed summation orders and why the
// call synchronises its stream are said there.  cv2's flags and the rational model are dcx_calib_flags.hip's entry, which shares the
// start below (dcx_calib_zhang_start).
#include "dcx_calib_dev.h"

namespace {

using Model = PinholeCalib;
using CalibState = Model::State;
using CalibWs = Ws<Model>;
constexpr int kRows = Model::kRows;

// ---------------------------------------------------------------------------------------------------------------- init

__global__ __launch_bounds__(kLanes) void calib_init_views_kernel(CornerPool pl, double cx, double cy, int32_t* __restrict__ status,
                                                                  double* __restrict__ pose, CalibWs ws) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int n, s0;
    int st = frame_status(pl, b, n, s0);
    double r[6] = {0, 0, 0, 0, 0, 0};
    if (st == DCX_PNP_OK) {
        // the DLT on the pixels themselves: undistort() through the identity camera leaves them as they are
        const PnpCamera ident = identity_camera();
        double H[9], mcx, mcy;
        st = homography(pl.frame(b), ident, false, H, mcx, mcy);
        if (st == DCX_PNP_OK) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {        // the principal point subtracted
                H[j] -= H[6 + j] * cx;
                H[3 + j] -= H[6 + j] * cy;
            }
            double h[3], v[3], d1[3], d2[3], nn[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                h[j] = H[3 * j];
                v[j] = H[3 * j + 1];
                d1[j] = (h[j] + v[j]) * 0.5;
                d2[j] = (h[j] - v[j]) * 0.5;
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                nn[0] += h[j] * h[j]; nn[1] += v[j] * v[j]; nn[2] += d1[j] * d1[j]; nn[3] += d2[j] * d2[j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) nn[j] = 1.0 / sqrt(nn[j]);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                h[j] *= nn[0]; v[j] *= nn[1]; d1[j] *= nn[2]; d2[j] *= nn[3];
            }
            r[0] = h[0] * v[0]; r[1] = h[1] * v[1]; r[2] = -h[2] * v[2];
            r[3] = d1[0] * d2[0]; r[4] = d1[1] * d2[1]; r[5] = -d1[2] * d2[2];
#pragma unroll
            for (int j = 0; j < 6; ++j)
                if (!isfinite(r[j])) st = DCX_PNP_NONFINITE;
            if (st != DCX_PNP_OK) {
#pragma unroll
                for (int j = 0; j < 6; ++j) r[j] = 0.0;
            }
        }
    }
    if (lane == 0) {
        status[b] = st;
#pragma unroll
        for (int i = 0; i < 7; ++i) pose[8 * (long long)b + i] = 0.0;
        pose[8 * (long long)b + 7] = (double)n;
#pragma unroll
        for (int i = 0; i < 6; ++i) ws.rows[(long long)b * kRows + i] = r[i];
    }
}

__global__ __launch_bounds__(kRedThreads) void calib_init_reduce_kernel(int batch, double cx, double cy,
                                                                        const int32_t* __restrict__ status,
                                                                        const double* __restrict__ pose, CalibWs ws) {
    __shared__ double s[kRedThreads][7];    // a00 a01 a11 b0 b1, views, points
    const int t = threadIdx.x;
    double a[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int b = t; b < batch; b += kRedThreads) {
        if (status[b] != DCX_PNP_OK) continue;
        const double* r = ws.rows + (long long)b * kRows;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const double a0 = r[3 * k], a1 = r[3 * k + 1], bb = r[3 * k + 2];
            a[0] += a0 * a0; a[1] += a0 * a1; a[2] += a1 * a1; a[3] += a0 * bb; a[4] += a1 * bb;
        }
        a[5] += 1.0;
        a[6] += pose[8 * (long long)b + 7];
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) s[t][j] = a[j];
    block_tree<kRedThreads, 7>(s);
    if (t != 0) return;
    CalibState* st = ws.st;
    const double a00 = s[0][0], a01 = s[0][1], a11 = s[0][2], b0 = s[0][3], b1 = s[0][4];
    lm_reset(st);
    st->result[12] = s[0][5];
    st->result[13] = s[0][6];
    if (s[0][5] == 0.0) {
        st->result[14] = DCX_CALIB_NO_VIEWS;
        st->code = kFinished;
        return;
    }
    const double det = a00 * a11 - a01 * a01;
    const double f0 = (a11 * b0 - a01 * b1) / det, f1 = (a00 * b1 - a01 * b0) / det;
    const double fx = f0 != 0.0 ? sqrt(fabs(1.0 / f0)) : INFINITY, fy = f1 != 0.0 ? sqrt(fabs(1.0 / f1)) : INFINITY;
    if (!(det > 1e-12 * a00 * a11) || !(isfinite(fx) && isfinite(fy) && fx > 0 && fy > 0)) {
        st->result[14] = DCX_CALIB_DEGENERATE;
        st->code = kFinished;
        return;
    }
    const double th[9] = {fx, fy, cx, cy, 0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 9; ++i) st->g[i] = th[i];
    st->code = kNextEvaluate;
}

__global__ __launch_bounds__(kLanes) void calib_init_poses_kernel(CornerPool pl, int32_t* __restrict__ status, CalibWs ws) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (ws.st->code == kFinished || status[b] != DCX_PNP_OK) return;
    const PnpCamera cam = camera_of(ws.st->g);       // K0, zero distortion
    double out[8];
    const int st = solve(pl.frame(b), cam, out);
    if (lane == 0) {
        if (st != DCX_PNP_OK) status[b] = st;
#pragma unroll
        for (int i = 0; i < 6; ++i) ws.pose[(long long)b * 6 + i] = st == DCX_PNP_OK ? out[i] : 0.0;
    }
}

}  // namespace

// Zhang's start up to K0 (init_views, init_reduce), queued on s: the state at d_state (kNextEvaluate with g = fx fy cx cy 0 .. 0,
// or kFinished with the status in result[14]), the views' rows at d_rows [B][6], every view's status and zeroed pose words with its
// point count.  For this unit's entry and for dcx_calib_flags.hip, which has its own poses kernel; not part of the C ABI.
void dcx_calib_zhang_start(const int32_t* d_counts, const int32_t* d_starts, const int32_t* d_rows, const float* d_xy, int batch, int pool,
                           int col_count, int row_count, double square_len, int image_width, int image_height, void* d_state,
                           double* d_init_rows, int32_t* d_view_status, double* d_pose, void* stream) {
    CornerPool pl;
    if (!corner_pool(d_counts, d_starts, d_rows, d_xy, batch, pool, col_count, row_count, square_len, pl)) return;   // (checked by the caller)
    CalibWs ws{};
    ws.st = (CalibState*)d_state;
    ws.rows = d_init_rows;
    const double cx = (image_width - 1) * 0.5, cy = (image_height - 1) * 0.5;
    hipLaunchKernelGGL(calib_init_views_kernel, dim3((unsigned)batch), dim3(kLanes), 0, (hipStream_t)stream, pl, cx, cy, d_view_status,
                       d_pose, ws);
    hipLaunchKernelGGL(calib_init_reduce_kernel, dim3(1), dim3(kRedThreads), 0, (hipStream_t)stream, batch, cx, cy, d_view_status, d_pose,
                       ws);
}

extern "C" size_t dcx_calibrate_workspace_bytes(int batch) { return batch > 0 ? ws_layout<Model>(nullptr, batch, nullptr) : 0; }

extern "C" int dcx_calibrate_pool(const int32_t* d_counts, const int32_t* d_starts, const int32_t* d_rows, const float* d_xy,
                                  int batch, int pool, int col_count, int row_count, double square_len, int image_width,
                                  int image_height, void* d_workspace, size_t workspace_bytes, int32_t* d_view_status,
                                  double* d_pose, double* h_result, void* stream) {
    CornerPool pl;
    CalibWs ws;
    if (const int e = calib_args(d_counts, d_starts, d_rows, d_xy, batch, pool, col_count, row_count, square_len, image_width,
                                 image_height, d_workspace, workspace_bytes, d_view_status, d_pose, h_result, pl, ws))
        return e;
    hipStream_t s = (hipStream_t)stream;
    dcx_calib_zhang_start(d_counts, d_starts, d_rows, d_xy, batch, pool, col_count, row_count, square_len, image_width, image_height,
                          ws.st, ws.rows, d_view_status, d_pose, stream);
    hipLaunchKernelGGL(calib_init_poses_kernel, dim3((unsigned)batch), dim3(kLanes), 0, s, pl, d_view_status, ws);
    DCX_CHECK_HIP(calib_lm(s, pl, batch, d_view_status, d_pose, ws));
    DCX_CHECK_HIP(hipMemcpyAsync(h_result, ws.st->result, 16 * sizeof(double), hipMemcpyDeviceToHost, s));
    DCX_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
}
