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
// Calibration: joint Levenberg-Marquardt over theta = (fx, fy, cx, cy, k1, k2, k3, k4) and every used view's (rvec, tvec) with
// dcx_calib.hip's rules, Schur elimination, host loop and fixed summation orders, at NG = 8: a row of [J_theta | J_pose | r] has
// 15 columns, a view's packed symmetric 15 x 15 has 120 entries.  There is no closed-form start for this model: the principal
// point starts at the image centre, fx = fy = focal0 (or max(w, h) / 2, at which every in-frame pixel undistorts: sqrt(2) < pi / 2),
// k = 0, and every view's pose is the fisheye PnP solve at that camera; the start being cruder than Zhang's, the cap is 100
// accepted steps, not 30.  Launches (one wave per view unless noted):
//   init_state (one thread), init_poses, evaluate, decide(init); then per attempt evaluate (after an accepted step), schur,
//   reduce_solve (one workgroup), trial, decide (one workgroup), as in dcx_calib.hip.
// The loop runs on the host and reads a state word after every attempt, so the call synchronises its stream.  No atomics, nothing
// allocated: two calls on the same input give the same bits.  The shared pieces are used as they stand: accumulate_rows,
// lane_entries, schur_view (dcx_mat_dev.h), LmState<8>, lm_source, lm_trial_pose, lm_decide_block, lm_run (dcx_lm_dev.h).
//
// Map and points: dcx_rectify.hip's two kernels with the ray through the fisheye model; a rectified ray with q_z <= 0 is outside.
#include "dcx_fisheye_dev.h"
#include "dcx_pnp_dev.h"
#include "dcx_lm_dev.h"

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

constexpr int kNG = 8;                                    // fx fy cx cy k1 k2 k3 k4
constexpr int kNC = kNG + 7;                              // a row: [J_theta (8) | J_pose (6) | r]
constexpr int kEntries = kNC * (kNC + 1) / 2;             // 120
constexpr int kCost = kEntries - 1;                       // pk<15>(14, 14)
constexpr int kNS = kNG * (kNG + 1) / 2;                  // 36
constexpr int kYZ = 6 * kNG + 6;                          // U*^-1 W^T (6 x 8, row major) and U*^-1 g_b (6)
constexpr int kSC = kNS + kNG;                            // the view's part of S (36 packed) and of the rhs (8)
constexpr int kTot = 2 * kSC;                             // sum V, sum g_a, sum S_i, sum W U*^-1 g_b
constexpr int kRedThreads = kLmThreads;
constexpr int kSlices = kRedThreads / 128;                // reduce_solve: 8 view slices x 128 entry slots
constexpr int kFisheyeMaxIter = 100;                      // accepted steps (fisheye.CALIB_MAX_ITER)
constexpr int kState = 512;                               // bytes reserved for the state
constexpr int kLdsStride = 17;                            // 15 values per row, padded to an odd stride as dcx_calib.hip's

using FcalState = LmState<kNG>;
static_assert(sizeof(FcalState) <= kState, "state");
static_assert(kTot <= 128 && kEntries <= 2 * kLanes, "layout");

struct Ws {
    FcalState* st;
    double *m, *yz, *sc, *pose, *trial_pose, *trial;      // trial = {cost, |dp|^2, |p|^2}
    int* fail;
};

// -> the bytes needed; *w (if given) = the parts of the workspace at base
size_t ws_layout(void* base, int batch, Ws* w) {
    const size_t B = (size_t)batch;
    Carver c{(char*)base, 0};
    Ws r;
    r.st = (FcalState*)c.take<char>(kState);
    r.m = c.take<double>(B * kEntries);
    r.yz = c.take<double>(B * kYZ);
    r.sc = c.take<double>(B * kSC);
    r.pose = c.take<double>(B * 6);
    r.trial_pose = c.take<double>(B * 6);
    r.trial = c.take<double>(B * 3);
    r.fail = c.take<int>(B);
    if (w) *w = r;
    return c.at;
}

struct Theta0 {
    double th[kNG];
};

__global__ void fcal_init_state_kernel(Theta0 t0, Ws ws) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    FcalState* st = ws.st;
    lm_reset(st);
    for (int i = 0; i < kNG; ++i) st->g[i] = st->g_trial[i] = t0.th[i];
    for (int i = 0; i < kNG; ++i) st->dg[i] = 0.0;
    st->prev_cost = 0.0;
    st->code = kNextEvaluate;
}

// the per-view checks and the view's pose at the start camera
__global__ __launch_bounds__(kLanes) void fcal_init_poses_kernel(CornerPool pl, Theta0 t0, int32_t* __restrict__ status,
                                                                 double* __restrict__ pose, Ws ws) {
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

// One point's projection at (theta, pose) -> residual (ru, rv); with JAC its two rows of [J_theta | J_pose]
// (fisheye._project_full's intrinsic columns).  false if the point is not in front of the camera.
template <bool JAC>
__device__ __forceinline__ bool project_point(const FisheyeCamera& cam, const double* p, const double* R, const double (*G)[9], double mx,
                                              double my, double u, double v, double& ru, double& rv, double* ju, double* jv) {
    double q[3], du[3], dv[3], a, b, xd, yd, tt, t2;
    board_point(R, p + 3, mx, my, q);
    if (!project<JAC>(cam, q, u, v, ru, rv, du, dv, a, b, xd, yd, tt, t2)) return false;
    if (!JAC) return true;
    ju[0] = xd;  ju[1] = 0.0; ju[2] = 1.0; ju[3] = 0.0;
    jv[0] = 0.0; jv[1] = yd;  jv[2] = 0.0; jv[3] = 1.0;
    double pw = tt;                            // tt theta^(2j)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        pw *= t2;
        ju[4 + j] = cam.fx * (a * pw);
        jv[4 + j] = cam.fy * (b * pw);
    }
    pose_columns(du, dv, mx, my, G, ju + kNG, jv + kNG);
    return true;
}

__global__ __launch_bounds__(kLanes) void fcal_evaluate_kernel(CornerPool pl, const int32_t* __restrict__ status, Ws ws) {
    __shared__ double sj[2 * kLanes][kLdsStride];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (ws.st->code != kNextEvaluate || status[b] != DCX_PNP_OK) return;
    const Frame f = pl.frame(b);
    const FisheyeCamera cam = fisheye_camera_of(ws.st->g);
    double p[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) p[i] = ws.pose[(long long)b * 6 + i];
    double R[9], G[2][9];
    pose_basis(p, R, G);
    int ea[2], eb[2];
    lane_entries<kNC, 2>(lane, ea, eb);
    double acc[2] = {0, 0};
    bool behind = false;
    accumulate_rows<kNC, 2, kLdsStride>(
        f.n,
        [&](int i, double* ju, double* jv) {
            double mx, my, u, v, ru, rv;
            f.load(i, mx, my, u, v);
            if (!project_point<true>(cam, p, R, G, mx, my, u, v, ru, rv, ju, jv)) return false;
            ju[kNC - 1] = ru;
            jv[kNC - 1] = rv;
            return true;
        },
        sj, ea, eb, acc, behind);
    const bool inf = __any(behind);
    double* m = ws.m + (long long)b * kEntries;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int e = lane + kLanes * q;
        if (e < kEntries) m[e] = (e == kCost && inf) ? INFINITY : acc[q];
    }
}

__global__ __launch_bounds__(kLanes) void fcal_schur_kernel(const int32_t* __restrict__ status, Ws ws) {
    __shared__ double sy[kNG + 1][6];          // U*^-1 W^T's 8 columns, then U*^-1 g_b
    const int b = blockIdx.x, lane = threadIdx.x;
    if (ws.st->code == kFinished || status[b] != DCX_PNP_OK) return;
    const double scale = lm_damping(ws.st->lg);
    const bool ok = schur_view<kNG>(ws.m + (long long)b * kEntries, scale, lane, sy, ws.yz + (long long)b * kYZ,
                                    ws.sc + (long long)b * kSC);
    if (lane == 0) ws.fail[b] = ok ? 0 : 1;
}

// dcx_calib.hip's reduce_solve at NG = 8: the views' parts in 8 slices, the slices added serially, the rolled Cholesky on LDS
__global__ __launch_bounds__(kRedThreads) void fcal_reduce_solve_kernel(int batch, const int32_t* __restrict__ status, Ws ws) {
    __shared__ double part[kSlices][kTot];
    __shared__ int bad[kSlices];
    __shared__ double tot[kTot], S[kNS], L[kNS], rhs[kNG], y[kNG], x[kNG];
    FcalState* st = ws.st;
    if (st->code == kFinished) return;
    const int t = threadIdx.x, e = t % 128, sl = t / 128;
    if (e < kTot) {
        const int src = lm_source<kNG>(e);     // where entry e lives: in the view's 120 (m) or in its Schur part (sc)
        double s = 0.0;
        int f = 0;
        for (int b = sl; b < batch; b += kSlices) {
            if (status[b] != DCX_PNP_OK) continue;
            s += e < kSC ? ws.m[(long long)b * kEntries + src] : ws.sc[(long long)b * kSC + src];
            if (e == 0) f |= ws.fail[b];
        }
        part[sl][e] = s;
        if (e == 0) bad[sl] = f;
    }
    __syncthreads();
    if (t != 0) return;
    int anybad = 0;
    for (int i = 0; i < kTot; ++i) {
        double s = 0.0;
        for (int k = 0; k < kSlices; ++k) s += part[k][i];
        tot[i] = s;
    }
    for (int k = 0; k < kSlices; ++k) anybad |= bad[k];
    if (anybad) {
        lm_fail(st, DCX_CALIB_DEGENERATE);
        return;
    }
    const double scale = lm_damping(st->lg);
    for (int a = 0; a < kNG; ++a) {
        for (int c = a; c < kNG; ++c) S[pk<kNG>(a, c)] = tot[pk<kNG>(a, c)] * (a == c ? scale : 1.0) - tot[kSC + pk<kNG>(a, c)];
        rhs[a] = tot[kNS + a] - tot[kSC + kNS + a];
    }
    for (int i = 0; i < kNG; ++i) {
        for (int j = 0; j <= i; ++j) {
            double s = S[pk<kNG>(i, j)];
            for (int k = 0; k < j; ++k) s -= L[pk<kNG>(i, k)] * L[pk<kNG>(j, k)];
            if (i == j) {
                if (!(s > 0)) {
                    lm_fail(st, DCX_CALIB_DEGENERATE);
                    return;
                }
                L[pk<kNG>(i, i)] = sqrt(s);
            } else {
                L[pk<kNG>(i, j)] = s / L[pk<kNG>(j, j)];
            }
        }
    }
    for (int i = 0; i < kNG; ++i) {
        double s = rhs[i];
        for (int k = 0; k < i; ++k) s -= L[pk<kNG>(i, k)] * y[k];
        y[i] = s / L[pk<kNG>(i, i)];
    }
    for (int i = kNG - 1; i >= 0; --i) {
        double s = y[i];
        for (int k = i + 1; k < kNG; ++k) s -= L[pk<kNG>(k, i)] * x[k];
        x[i] = s / L[pk<kNG>(i, i)];
    }
    for (int i = 0; i < kNG; ++i) {
        st->dg[i] = x[i];
        st->g_trial[i] = st->g[i] - x[i];
    }
}

__global__ __launch_bounds__(kLanes) void fcal_trial_kernel(CornerPool pl, const int32_t* __restrict__ status, Ws ws) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (ws.st->code == kFinished || status[b] != DCX_PNP_OK) return;
    double p[6], dn, pn;
    lm_trial_pose<kNG>(ws.yz + (long long)b * kYZ, ws.st->dg, ws.pose + (long long)b * 6, p, dn, pn);
    const FisheyeCamera cam = fisheye_camera_of(ws.st->g_trial);
    const Frame f = pl.frame(b);
    double R[9];
    rodrigues(p, R);
    double c[1] = {0.0};
    for (int i = lane; i < f.n; i += kLanes) {
        double mx, my, u, v, ru, rv;
        f.load(i, mx, my, u, v);
        if (!project_point<false>(cam, p, R, nullptr, mx, my, u, v, ru, rv, nullptr, nullptr)) {
            c[0] = INFINITY;
            continue;
        }
        c[0] += ru * ru + rv * rv;
    }
    wave_sum(c);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) ws.trial_pose[(long long)b * 6 + k] = p[k];
        ws.trial[(long long)b * 3 + 0] = c[0];
        ws.trial[(long long)b * 3 + 1] = dn;
        ws.trial[(long long)b * 3 + 2] = pn;
    }
}

// init = 1: after the first evaluate (the initial cost); init = 0: after a trial
__global__ __launch_bounds__(kRedThreads) void fcal_decide_kernel(int batch, int init, const int32_t* __restrict__ status,
                                                                  double* __restrict__ pose, Ws ws) {
    lm_decide_block<kNG, false, 16, kFisheyeMaxIter>(
        ws.st, batch, init, ws.pose, ws.trial_pose, [&](int b) { return status[b] == DCX_PNP_OK; },
        [&](int b) { return ws.m[(long long)b * kEntries + kCost]; },
        [&](int b, double* a) {
            const double* tr = ws.trial + (long long)b * 3;
            a[0] += tr[0]; a[1] += tr[1]; a[2] += tr[2];
        },
        [&](int b) { return pose[8 * (long long)b + 7]; },
        [&](int b) {
            double* o = pose + 8 * (long long)b;
#pragma unroll
            for (int k = 0; k < 6; ++k) o[k] = ws.trial_pose[(long long)b * 6 + k];
            o[6] = sqrt(ws.trial[(long long)b * 3] / o[7]);
        });
}

// ---------------------------------------------------------------------------------------------------------------- map and points

constexpr int kMapShift = 5;                 // fractional bits of a map entry (dcx_rectify.hip's)
constexpr double kMapLimit = 32768.0;        // a source position beyond this many px is outside

struct RectXform {
    double R[9];                             // row major
    double fx, fy, cx, cy;                   // the left 3x3 of P
};

// R (NULL: identity) and P (3x4 row major, NULL: K) from the host -> the kernel argument; false if refused
inline bool rect_xform(const double* h_R9, const double* h_P12, const FisheyeCamera& cam, RectXform& x) {
    for (int i = 0; i < 9; ++i) {
        x.R[i] = h_R9 ? h_R9[i] : (i % 4 == 0 ? 1.0 : 0.0);
        if (!isfinite(x.R[i])) return false;
    }
    if (h_P12) {
        if (h_P12[1] != 0.0) return false;
        x.fx = h_P12[0]; x.cx = h_P12[2]; x.fy = h_P12[5]; x.cy = h_P12[6];
    } else {
        x.fx = cam.fx; x.fy = cam.fy; x.cx = cam.cx; x.cy = cam.cy;
    }
    return isfinite(x.fx) && isfinite(x.fy) && isfinite(x.cx) && isfinite(x.cy) && x.fx != 0.0 && x.fy != 0.0;
}

// one thread per output pixel
__global__ __launch_bounds__(256) void dcx_fisheye_map_kernel(FisheyeCamera cam, RectXform xf, int width, int height,
                                                              int32_t* __restrict__ map) {
    const int u = blockIdx.x * 64 + (threadIdx.x & 63), v = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (u >= width || v >= height) return;
    const double x = ((double)u - xf.cx) / xf.fx, y = ((double)v - xf.cy) / xf.fy;
    const double qx = xf.R[0] * x + xf.R[3] * y + xf.R[6];          // R^T (x, y, 1)
    const double qy = xf.R[1] * x + xf.R[4] * y + xf.R[7];
    const double qz = xf.R[2] * x + xf.R[5] * y + xf.R[8];
    double xd, yd, tt, t2, a, b, d;
    fisheye_distort<false>(cam.k, qx / qz, qy / qz, xd, yd, tt, t2, a, b, d);
    const double mx = cam.fx * xd + cam.cx, my = cam.fy * yd + cam.cy;
    int2 e = make_int2(INT32_MIN, INT32_MIN);
    if (qz > 0 && fabs(mx) <= kMapLimit && fabs(my) <= kMapLimit)    // (NaN and inf compare false)
        e = make_int2((int)rint((double)(1 << kMapShift) * mx), (int)rint((double)(1 << kMapShift) * my));
    reinterpret_cast<int2*>(map)[(size_t)v * width + u] = e;
}

// one lane per slot of the pool
__global__ __launch_bounds__(kLanes) void dcx_fisheye_points_kernel(const int32_t* __restrict__ rows, const float* __restrict__ xy,
                                                                    int pool, FisheyeCamera cam, RectXform xf,
                                                                    double* __restrict__ out) {
    const int i = blockIdx.x * kLanes + threadIdx.x;
    if (i >= pool) return;
    double u, v;
    if (xy) {
        u = (double)xy[2 * (size_t)i];
        v = (double)xy[2 * (size_t)i + 1];
    } else {
        u = (double)rows[4 * (size_t)i];
        v = (double)rows[4 * (size_t)i + 1];
    }
    double x, y;
    const bool inside = undistort(cam, u, v, x, y);
    const double X = xf.R[0] * x + xf.R[1] * y + xf.R[2];
    const double Y = xf.R[3] * x + xf.R[4] * y + xf.R[5];
    const double Z = xf.R[6] * x + xf.R[7] * y + xf.R[8];
    double ou = NAN, ov = NAN;
    if (inside && Z > 0) {
        ou = xf.fx * (X / Z) + xf.cx;
        ov = xf.fy * (Y / Z) + xf.cy;
    }
    out[2 * (size_t)i] = ou;
    out[2 * (size_t)i + 1] = ov;
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

extern "C" size_t dcx_fisheye_calibrate_workspace_bytes(int batch) { return batch > 0 ? ws_layout(nullptr, batch, nullptr) : 0; }

extern "C" int dcx_fisheye_calibrate_pool(const int32_t* d_counts, const int32_t* d_starts, const int32_t* d_rows, const float* d_xy,
                                          int batch, int pool, int col_count, int row_count, double square_len, int image_width,
                                          int image_height, double focal0, void* d_workspace, size_t workspace_bytes,
                                          int32_t* d_view_status, double* d_pose, double* h_result, void* stream) {
    CornerPool pl;
    if (!corner_pool(d_counts, d_starts, d_rows, d_xy, batch, pool, col_count, row_count, square_len, pl)) return DCX_E_ARG;
    if (!d_workspace || !d_view_status || !d_pose || !h_result || image_width <= 0 || image_height <= 0) return DCX_E_ARG;
    if (focal0 > 0 && isinf(focal0)) return DCX_E_ARG;
    if (workspace_bytes < ws_layout(nullptr, batch, nullptr)) return DCX_E_WS;
    hipStream_t s = (hipStream_t)stream;
    Ws ws;
    ws_layout(d_workspace, batch, &ws);
    const double f0 = focal0 > 0 ? focal0 : 0.5 * (double)(image_width > image_height ? image_width : image_height);
    const Theta0 t0{{f0, f0, (image_width - 1) * 0.5, (image_height - 1) * 0.5, 0.0, 0.0, 0.0, 0.0}};
    const dim3 views((unsigned)batch), wave(kLanes), one(1), red(kRedThreads);
    hipLaunchKernelGGL(fcal_init_state_kernel, one, dim3(1), 0, s, t0, ws);
    hipLaunchKernelGGL(fcal_init_poses_kernel, views, wave, 0, s, pl, t0, d_view_status, d_pose, ws);
    hipLaunchKernelGGL(fcal_evaluate_kernel, views, wave, 0, s, pl, d_view_status, ws);
    hipLaunchKernelGGL(fcal_decide_kernel, one, red, 0, s, batch, 1, d_view_status, d_pose, ws);
    DCX_CHECK_HIP(hipGetLastError());
    DCX_CHECK_HIP(lm_run(s, &ws.st->code, kFisheyeMaxIter, [&](bool evaluate) {
        if (evaluate) hipLaunchKernelGGL(fcal_evaluate_kernel, views, wave, 0, s, pl, d_view_status, ws);
        hipLaunchKernelGGL(fcal_schur_kernel, views, wave, 0, s, d_view_status, ws);
        hipLaunchKernelGGL(fcal_reduce_solve_kernel, one, red, 0, s, batch, d_view_status, ws);
        hipLaunchKernelGGL(fcal_trial_kernel, views, wave, 0, s, pl, d_view_status, ws);
        hipLaunchKernelGGL(fcal_decide_kernel, one, red, 0, s, batch, 0, d_view_status, d_pose, ws);
    }));
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
    hipLaunchKernelGGL(dcx_fisheye_map_kernel, grid, dim3(256), 0, (hipStream_t)stream, cam, xf, width, height, d_map);
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
    hipLaunchKernelGGL(dcx_fisheye_points_kernel, dim3((unsigned)((pool + kLanes - 1) / kLanes)), dim3(kLanes), 0,
                       (hipStream_t)stream, d_rows, d_xy, pool, cam, xf, d_out);
    return (int)hipGetLastError();
}
