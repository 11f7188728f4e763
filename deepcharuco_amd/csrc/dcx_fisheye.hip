// dcx_fisheye.hip -- the fisheye camera model on the device (cv2.fisheye's documented model, skew 0, field of view under 180
// degrees; dcx_fisheye_dev.h): the pose of every frame of a corner pool (cv2.solvePnP on a fisheye camera), the calibration of such
// a camera from the views of a pool (cv2.fisheye.calibrate's role), the undistort + rectify map (cv2.fisheye.initUndistortRectifyMap
// in the 1/32 px fixed point that dcx_remap_u8 reads) and the corner pool in rectified coordinates (cv2.fisheye.undistortPoints with
// R and P).  deepcharuco_amd/fisheye.py restates every step (solve_pnp_fisheye_host_full, calibrate_fisheye_host_full,
// undistort_rectify_map_fisheye_host, rectify_points_fisheye_host) and is the pin of these kernels.  All fp64.
//
// Pose: dcx_pnp.hip's kernel with the other camera: one 64-lane wave per frame, the solver of dcx_pnp_dev.h (a template on the
// camera class) through FisheyeCamera's undistort / project; a frame with a pixel outside the model is DCX_PNP_DEGENERATE.
//
// Calibration: joint Levenberg-Marquardt over theta = (fx, fy, cx, cy, k1, k2, k3, k4) and every used view's (rvec, tvec):
// dcx_calib_dev.h's kernels, host loop and fixed summation orders, the text dcx_calib.hip runs, instantiated on FisheyeCalib
// (NG = 8: a row of [J_theta | J_pose | r] has 15 columns, a view's packed symmetric 15 x 15 has 120 entries).  This unit holds the
// start.  There is no closed-form one for this model: the principal point starts at the image centre, fx = fy = focal0 (or
// max(w, h) / 2, at which every in-frame pixel undistorts: sqrt(2) < pi / 2), k = 0, and every view's pose is the fisheye PnP
// solve at that camera; the start being cruder than Zhang's, the cap is 100 accepted steps, not 30.  Launches: init_state (one
// thread), init_poses (one wave per view), then the shared solve.  The call synchronises its stream.  No atomics, nothing
// allocated: two calls on the same input give the same bits.
//
// Map and points: dcx_rectify_dev.h's two kernels, the text dcx_rectify.hip runs, with the ray through the fisheye model; a
// rectified ray with q_z <= 0 is outside.
#include "dcx_calib_dev.h"
#include "dcx_rectify_dev.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------- pose

__global__ __launch_bounds__(kLanes) void dcx_fisheye_solve_pnp_kernel(CornerPool pl, FisheyeCamera cam, int32_t* __restrict__ status,
                                                                       double* __restrict__ pose) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int n, s0;
    int st = frame_status(pl, b, n, s0);
    double out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (st == DCX_PNP_OK) {
        st = solve(pl.frame(n, s0), cam, out);
        if (st != DCX_PNP_OK) {
#pragma unroll
            for (int i = 0; i < 8; ++i) out[i] = 0.0;
        }
    }
    if (lane == 0) {
        status[b] = st;
#pragma unroll
        for (int i = 0; i < 8; ++i) pose[8 * (long long)b + i] = out[i];
    }
}

// ---------------------------------------------------------------------------------------------------------------- calibration

using Model = FisheyeCalib;
using FcalWs = Ws<Model>;
constexpr int kNG = Model::NG;

struct Theta0 {
    double th[kNG];
};

__global__ void fcal_init_state_kernel(Theta0 t0, FcalWs ws) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    Model::State* st = ws.st;
    lm_reset(st);
    for (int i = 0; i < kNG; ++i) st->g[i] = st->g_trial[i] = t0.th[i];
    for (int i = 0; i < kNG; ++i) st->dg[i] = 0.0;
    st->prev_cost = 0.0;
    st->code = kNextEvaluate;
}

// the per-view checks and the view's pose at the start camera
__global__ __launch_bounds__(kLanes) void fcal_init_poses_kernel(CornerPool pl, Theta0 t0, int32_t* __restrict__ status,
                                                                 double* __restrict__ pose, FcalWs ws) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int n, s0;
    int st = frame_status(pl, b, n, s0);
    double out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (st == DCX_PNP_OK) st = solve(pl.frame(n, s0), fisheye_camera_of(t0.th), out);
    if (lane == 0) {
        status[b] = st;
#pragma unroll
        for (int i = 0; i < 7; ++i) pose[8 * (long long)b + i] = 0.0;
        pose[8 * (long long)b + 7] = (double)n;
#pragma unroll
        for (int i = 0; i < 6; ++i) ws.pose[(long long)b * 6 + i] = st == DCX_PNP_OK ? out[i] : 0.0;
    }
}

}  // namespace

extern "C" int dcx_fisheye_solve_pnp_pool(const int32_t* d_counts, const int32_t* d_starts, const int32_t* d_rows, const float* d_xy,
                                          int batch, int pool, int col_count, int row_count, double square_len,
                                          const double* h_camera9, const double* h_dist4, int32_t* d_status, double* d_pose,
                                          void* stream) {
    CornerPool pl;
    FisheyeCamera cam;
    if (!corner_pool(d_counts, d_starts, d_rows, d_xy, batch, pool, col_count, row_count, square_len, pl)) return DCX_E_ARG;
    if (!d_status || !d_pose || !fisheye_camera(h_camera9, h_dist4, cam)) return DCX_E_ARG;
    hipLaunchKernelGGL(dcx_fisheye_solve_pnp_kernel, dim3((unsigned)batch), dim3(kLanes), 0, (hipStream_t)stream, pl, cam, d_status,
                       d_pose);
    return (int)hipGetLastError();
}

extern "C" size_t dcx_fisheye_calibrate_workspace_bytes(int batch) { return batch > 0 ? ws_layout<Model>(nullptr, batch, nullptr) : 0; }

extern "C" int dcx_fisheye_calibrate_pool(const int32_t* d_counts, const int32_t* d_starts, const int32_t* d_rows, const float* d_xy,
                                          int batch, int pool, int col_count, int row_count, double square_len, int image_width,
                                          int image_height, double focal0, void* d_workspace, size_t workspace_bytes,
                                          int32_t* d_view_status, double* d_pose, double* h_result, void* stream) {
    CornerPool pl;
    FcalWs ws;
    if (focal0 > 0 && isinf(focal0)) return DCX_E_ARG;
    if (const int e = calib_args(d_counts, d_starts, d_rows, d_xy, batch, pool, col_count, row_count, square_len, image_width,
                                 image_height, d_workspace, workspace_bytes, d_view_status, d_pose, h_result, pl, ws))
        return e;
    hipStream_t s = (hipStream_t)stream;
    const double f0 = focal0 > 0 ? focal0 : 0.5 * (double)(image_width > image_height ? image_width : image_height);
    const Theta0 t0{{f0, f0, (image_width - 1) * 0.5, (image_height - 1) * 0.5, 0.0, 0.0, 0.0, 0.0}};
    hipLaunchKernelGGL(fcal_init_state_kernel, dim3(1), dim3(1), 0, s, t0, ws);
    hipLaunchKernelGGL(fcal_init_poses_kernel, dim3((unsigned)batch), dim3(kLanes), 0, s, pl, t0, d_view_status, d_pose, ws);
    DCX_CHECK_HIP(calib_lm(s, pl, batch, d_view_status, d_pose, ws));
    // the state's result is g (8), rms, steps, attempts, views, points, status; h_result keeps dcx_calibrate_pool's places
    double r[16];
    DCX_CHECK_HIP(hipMemcpyAsync(r, ws.st->result, 16 * sizeof(double), hipMemcpyDeviceToHost, s));
    DCX_CHECK_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < 8; ++i) h_result[i] = r[i];
    h_result[8] = 0.0;
    for (int i = 0; i < 6; ++i) h_result[9 + i] = r[8 + i];
    h_result[15] = 0.0;
    return 0;
}

extern "C" int dcx_fisheye_undistort_rectify_map(const double* h_camera9, const double* h_dist4, const double* h_R9,
                                                 const double* h_P12, int width, int height, int32_t* d_map, void* stream) {
    if (!d_map || ((uintptr_t)d_map & 7) || width <= 0 || height <= 0 || (long long)width * height > 0x7fffffffLL / 2) return DCX_E_ARG;
    FisheyeCamera cam;
    RectXform xf;
    if (!fisheye_camera(h_camera9, h_dist4, cam) || !rect_xform(h_R9, h_P12, cam, xf)) return DCX_E_ARG;
    const dim3 grid((unsigned)((width + 63) / 64), (unsigned)((height + 3) / 4));
    if (grid.y > 65535u) return DCX_E_ARG;
    hipLaunchKernelGGL(dcx_rectify_map_kernel<FisheyeCamera>, grid, dim3(256), 0, (hipStream_t)stream, cam, xf, width, height, d_map);
    return (int)hipGetLastError();
}

extern "C" int dcx_fisheye_rectify_points_pool(const int32_t* d_rows, const float* d_xy, int pool, const double* h_camera9,
                                               const double* h_dist4, const double* h_R9, const double* h_P12, double* d_out,
                                               void* stream) {
    if (pool < 0 || (pool > 0 && (!d_out || (!d_rows && !d_xy)))) return DCX_E_ARG;
    FisheyeCamera cam;
    RectXform xf;
    if (!fisheye_camera(h_camera9, h_dist4, cam) || !rect_xform(h_R9, h_P12, cam, xf)) return DCX_E_ARG;
    if (pool == 0) return 0;
    hipLaunchKernelGGL(dcx_rectify_points_kernel<FisheyeCamera>, dim3((unsigned)((pool + kLanes - 1) / kLanes)), dim3(kLanes), 0,
                       (hipStream_t)stream, d_rows, d_xy, pool, cam, xf, d_out);
    return (int)hipGetLastError();
}
