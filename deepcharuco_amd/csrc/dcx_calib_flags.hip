// dcx_calib_flags.hip -- cv2.calibrateCamera's flags and the rational model on the device: dcx_calibrate_flags_pool, the entry beside
// dcx_calibrate_pool (dcx_calib.hip), in a unit of its own so that nothing here can move that unit's or dcx_fisheye.hip's code.
// deepcharuco_amd/calib.py restates every rule (its module docstring; calibrate_camera_host_full with flags is the pin).
//
// The parameter vector is theta12 = fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6 with a mask of free entries.  Two models run it:
//   PinholeCalib (NG = 9)    while k4 k5 k6 are zero and fixed: dcx_calib_dev.h's per-view kernels exactly as the default call runs
//                            them, and reduce_solve with its mask (CalibMask there)
//   RationalCalib (NG = 12)  with DCX_CALIB_RATIONAL_MODEL, or a guess whose k4 k5 k6 are not all zero: the same five kernels
//                            instantiated on the trait below (NC = 19, 190 packed entries, three rounds of lane entries)
// The start:
//   without a guess   dcx_calib.hip's Zhang start into a side state (dcx_calib_zhang_start), then seed: theta12 from it, OpenCV's
//                     aspect rule on K0 under FIX_ASPECT_RATIO
//   with a guess      guess_views (the per-view checks of the default start, without its init rows), then seed: theta12 from the
//                     host-checked model
//   then poses: solve() through the seeded camera, distortion included (dcx_calib.hip's init_poses with another camera).
// Like dcx_calibrate_pool the call synchronises its stream; every sum has a fixed order (no atomics), nothing is allocated.
#include "dcx_calib_dev.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------- the rational model

// the pinhole camera with the denominator live; a type of its own so that project_point() can be overloaded on it
struct RationalCamera : PnpCamera {};

struct RationalCalib : CalibSizes<12, 21, 4> {            // fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6
    using Camera = RationalCamera;
    static constexpr int kMaxIter = kJointMaxIter;
    static constexpr int kRows = 0;                       // (the Zhang start keeps its rows beside the workspace of either model)
    static __device__ __forceinline__ Camera camera(const double* th) {
        RationalCamera c;
        c.fx = th[0]; c.fy = th[1]; c.cx = th[2]; c.cy = th[3];
#pragma unroll
        for (int i = 0; i < 8; ++i) c.k[i] = th[4 + i];
        return c;
    }
};
static_assert(RationalCalib::NC == 19 && RationalCalib::kEntries == 190 && RationalCalib::NQ == 3 && RationalCalib::kTot == 180, "sizes");

// dcx_calib_dev.h's project_point for the rational camera (calib._project_full12): the k1 k2 k3 columns divided by den, and the
// k4 k5 k6 columns -f (x, y) r^2j num / den^2
template <bool JAC>
__device__ __forceinline__ bool project_point(const RationalCamera& cam, const double* p, const double* R, const double (*G)[9], double mx,
                                              double my, double u, double v, double& ru, double& rv, double* ju, double* jv) {
    double q[3], du[3], dv[3], x, y, xd, yd;
    board_point(R, p + 3, mx, my, q);
    if (!project<JAC>(static_cast<const PnpCamera&>(cam), q, u, v, ru, rv, du, dv, x, y, xd, yd)) return false;
    if (!JAC) return true;
    const double* k = cam.k;
    const double r2 = x * x + y * y;
    const double r4 = r2 * r2, r6 = r2 * r2 * r2;
    const double num = 1 + r2 * (k[0] + r2 * (k[1] + r2 * k[4]));
    const double den = 1 + r2 * (k[5] + r2 * (k[6] + r2 * k[7]));
    const double iden = 1.0 / den;
    const double gq = -(num * iden) * iden;
    ju[0] = xd;  ju[1] = 0.0; ju[2] = 1.0; ju[3] = 0.0;
    jv[0] = 0.0; jv[1] = yd;  jv[2] = 0.0; jv[3] = 1.0;
    ju[4] = cam.fx * (x * r2 * iden);     jv[4] = cam.fy * (y * r2 * iden);
    ju[5] = cam.fx * (x * r4 * iden);     jv[5] = cam.fy * (y * r4 * iden);
    ju[6] = cam.fx * (2 * x * y);         jv[6] = cam.fy * (r2 + 2 * y * y);
    ju[7] = cam.fx * (r2 + 2 * x * x);    jv[7] = cam.fy * (2 * x * y);
    ju[8] = cam.fx * (x * r6 * iden);     jv[8] = cam.fy * (y * r6 * iden);
    ju[9] = cam.fx * (x * r2 * gq);       jv[9] = cam.fy * (y * r2 * gq);
    ju[10] = cam.fx * (x * r4 * gq);      jv[10] = cam.fy * (y * r4 * gq);
    ju[11] = cam.fx * (x * r6 * gq);      jv[11] = cam.fy * (y * r6 * gq);
    pose_columns(du, dv, mx, my, G, ju + RationalCalib::NG, jv + RationalCalib::NG);
    return true;
}

// ---------------------------------------------------------------------------------------------------------------- the start

using ZhangState = PinholeCalib::State;      // what dcx_calib_zhang_start writes
constexpr int kZhangRows = PinholeCalib::kRows;

struct Theta12 {
    double th[12];
};

// What the seed needs of the flags: the guess (use_guess) or the rule on Zhang's K0 (ratio: FIX_ASPECT_RATIO without a guess)
struct Seed {
    Theta12 guess;
    int use_guess, ratio;
    double a;
};

// the per-view checks of calib_init_views_kernel without its init rows: the frame, then the DLT homography on the pixels as they are
__global__ __launch_bounds__(kLanes) void calib_guess_views_kernel(CornerPool pl, int32_t* __restrict__ status, double* __restrict__ pose) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int n, s0;
    int st = frame_status(pl, b, n, s0);
    if (st == DCX_PNP_OK) {
        const PnpCamera ident = identity_camera();
        double H[9], mcx, mcy;
        st = homography(pl.frame(b), ident, false, H, mcx, mcy);
    }
    if (lane == 0) {
        status[b] = st;
#pragma unroll
        for (int i = 0; i < 7; ++i) pose[8 * (long long)b + i] = 0.0;
        pose[8 * (long long)b + 7] = (double)n;
    }
}

// One thread: the model's state from the guess, or from the Zhang start's (its failure handed on with its counts).
template <class M>
__global__ void calib_seed_kernel(Seed sd, const ZhangState* __restrict__ zh, Ws<M> ws) {
    constexpr int NG = M::NG;
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    typename M::State* st = ws.st;
    lm_reset(st);
    double th[12];
    for (int i = 0; i < 12; ++i) th[i] = sd.use_guess ? sd.guess.th[i] : 0.0;
    int code = kNextEvaluate;
    if (!sd.use_guess) {
        for (int i = 0; i < 4; ++i) th[i] = zh->g[i];
        if (sd.ratio) {                                   // OpenCV's rule on the init's focal lengths
            const double tf = (th[0] + th[1]) / (sd.a + 1.0);
            th[0] = sd.a * tf;
            th[1] = tf;
        }
        if (zh->code == kFinished) {                      // no views, or a singular init
            for (int i = 0; i < 12; ++i) th[i] = 0.0;
            st->result[NG + 3] = zh->result[12];
            st->result[NG + 4] = zh->result[13];
            st->result[NG + 5] = zh->result[14];
            code = kFinished;
        }
    }
    for (int i = 0; i < NG; ++i) {
        st->g[i] = st->g_trial[i] = th[i];
        st->dg[i] = 0.0;
    }
    st->prev_cost = 0.0;
    st->code = code;
}

// calib_init_poses_kernel of dcx_calib.hip with the seeded camera: solve() through it, distortion included
template <class M>
__global__ __launch_bounds__(kLanes) void calib_flags_poses_kernel(CornerPool pl, int32_t* __restrict__ status, Ws<M> ws) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (ws.st->code == kFinished || status[b] != DCX_PNP_OK) return;
    const PnpCamera cam = M::camera(ws.st->g);
    double out[8];
    const int st = solve(pl.frame(b), cam, out);
    if (lane == 0) {
        if (st != DCX_PNP_OK) status[b] = st;
#pragma unroll
        for (int i = 0; i < 6; ++i) ws.pose[(long long)b * 6 + i] = st == DCX_PNP_OK ? out[i] : 0.0;
    }
}

// ---------------------------------------------------------------------------------------------------------------- host

constexpr int kKnown = DCX_CALIB_USE_INTRINSIC_GUESS | DCX_CALIB_FIX_ASPECT_RATIO | DCX_CALIB_FIX_PRINCIPAL_POINT |
                       DCX_CALIB_ZERO_TANGENT_DIST | DCX_CALIB_FIX_FOCAL_LENGTH | DCX_CALIB_FIX_K1 | DCX_CALIB_FIX_K2 | DCX_CALIB_FIX_K3 |
                       DCX_CALIB_FIX_K4 | DCX_CALIB_FIX_K5 | DCX_CALIB_FIX_K6 | DCX_CALIB_RATIONAL_MODEL;

// the model's workspace, then the Zhang start's side state and rows
template <class M>
size_t flags_layout(void* base, int batch, Ws<M>* w, ZhangState** zh, double** rows) {
    const size_t at = ws_layout<M>(base, batch, w);
    Carver c{(char*)base, at};
    ZhangState* z = (ZhangState*)c.take<char>(kState);
    double* r = c.take<double>((size_t)batch * kZhangRows);
    if (zh) *zh = z;
    if (rows) *rows = r;
    return c.at;
}

struct FlagsCall {
    const int32_t *d_counts, *d_starts, *d_rows;
    const float* d_xy;
    int batch, pool, col_count, row_count;
    double square_len;
    int image_width, image_height;
    void* d_workspace;
    size_t workspace_bytes;
    int32_t* d_view_status;
    double* d_pose;
    double* h_result;
    void* stream;
};

template <class M>
int run(const FlagsCall& a, const CornerPool& pl, const Seed& sd, const CalibMask& mk) {
    constexpr int NG = M::NG, NR = M::kResult;
    Ws<M> ws;
    ZhangState* zh;
    double* rows;
    if (a.workspace_bytes < flags_layout<M>(nullptr, a.batch, nullptr, nullptr, nullptr)) return DCX_E_WS;
    flags_layout<M>(a.d_workspace, a.batch, &ws, &zh, &rows);
    hipStream_t s = (hipStream_t)a.stream;
    const dim3 views((unsigned)a.batch), wave(kLanes), one(1), red(kRedThreads);
    if (sd.use_guess)
        hipLaunchKernelGGL(calib_guess_views_kernel, views, wave, 0, s, pl, a.d_view_status, a.d_pose);
    else
        dcx_calib_zhang_start(a.d_counts, a.d_starts, a.d_rows, a.d_xy, a.batch, a.pool, a.col_count, a.row_count, a.square_len,
                              a.image_width, a.image_height, zh, rows, a.d_view_status, a.d_pose, a.stream);
    hipLaunchKernelGGL(calib_seed_kernel<M>, one, one, 0, s, sd, zh, ws);
    hipLaunchKernelGGL(calib_flags_poses_kernel<M>, views, wave, 0, s, pl, a.d_view_status, ws);
    DCX_CHECK_HIP(calib_lm(s, pl, a.batch, a.d_view_status, a.d_pose, ws, [&] {
        hipLaunchKernelGGL((calib_reduce_solve_kernel<M, CalibMask>), one, red, 0, s, a.batch, a.d_view_status, ws, mk);
    }));
    // the state's result is g (NG), rms, steps, attempts, views, points, status; h_result has theta12 in front
    double r[NR];
    DCX_CHECK_HIP(hipMemcpyAsync(r, ws.st->result, NR * sizeof(double), hipMemcpyDeviceToHost, s));
    DCX_CHECK_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < 20; ++i) a.h_result[i] = 0.0;
    for (int i = 0; i < NG; ++i) a.h_result[i] = r[i];
    for (int i = 0; i < 6; ++i) a.h_result[12 + i] = r[NG + i];
    return 0;
}

bool rational_flags(int flags) { return (flags & DCX_CALIB_RATIONAL_MODEL) != 0; }

}  // namespace

extern "C" size_t dcx_calibrate_flags_workspace_bytes(int batch, int flags) {
    if (batch <= 0 || (flags & ~kKnown)) return 0;
    return rational_flags(flags) ? flags_layout<RationalCalib>(nullptr, batch, nullptr, nullptr, nullptr)
                                 : flags_layout<PinholeCalib>(nullptr, batch, nullptr, nullptr, nullptr);
}

extern "C" int dcx_calibrate_flags_pool(const int32_t* d_counts, const int32_t* d_starts, const int32_t* d_rows, const float* d_xy,
                                        int batch, int pool, int col_count, int row_count, double square_len, int image_width,
                                        int image_height, int flags, const double* h_camera9, const double* h_dist, int n_dist,
                                        void* d_workspace, size_t workspace_bytes, int32_t* d_view_status, double* d_pose,
                                        double* h_result, void* stream) {
    CornerPool pl;
    if (!corner_pool(d_counts, d_starts, d_rows, d_xy, batch, pool, col_count, row_count, square_len, pl)) return DCX_E_ARG;
    if (!d_workspace || !d_view_status || !d_pose || !h_result || image_width <= 0 || image_height <= 0) return DCX_E_ARG;
    if (flags & ~kKnown) return DCX_E_ARG;
    const bool use_guess = flags & DCX_CALIB_USE_INTRINSIC_GUESS, fix_aspect = flags & DCX_CALIB_FIX_ASPECT_RATIO;
    if ((use_guess || fix_aspect) && !h_camera9) return DCX_E_ARG;
    if (!use_guess && (h_dist || n_dist != 0)) return DCX_E_ARG;                  // the coefficients are part of the guess
    PnpCamera cam = {};
    if (h_camera9 && !pnp_camera(h_camera9, h_dist, n_dist, cam)) return DCX_E_ARG;

    Seed sd = {};
    CalibMask mk = {0xFFFu, 0, 0.0};
    if (!(flags & DCX_CALIB_RATIONAL_MODEL)) mk.free &= ~0xE00u;
    if (flags & DCX_CALIB_FIX_PRINCIPAL_POINT) mk.free &= ~0x00Cu;
    if (flags & DCX_CALIB_FIX_FOCAL_LENGTH) mk.free &= ~0x003u;
    if (flags & DCX_CALIB_ZERO_TANGENT_DIST) mk.free &= ~0x0C0u;
    const int fix_k[6][2] = {{DCX_CALIB_FIX_K1, 4}, {DCX_CALIB_FIX_K2, 5}, {DCX_CALIB_FIX_K3, 8},
                             {DCX_CALIB_FIX_K4, 9}, {DCX_CALIB_FIX_K5, 10}, {DCX_CALIB_FIX_K6, 11}};
    for (const auto& f : fix_k)
        if (flags & f[0]) mk.free &= ~(1u << f[1]);
    if (use_guess) {
        sd.use_guess = 1;
        const double th[12] = {cam.fx, cam.fy, cam.cx, cam.cy, cam.k[0], cam.k[1], cam.k[2], cam.k[3], cam.k[4], cam.k[5], cam.k[6], cam.k[7]};
        for (int i = 0; i < 12; ++i) sd.guess.th[i] = th[i];
        if (flags & DCX_CALIB_ZERO_TANGENT_DIST) sd.guess.th[6] = sd.guess.th[7] = 0.0;
    }
    if (fix_aspect) {
        const double a = cam.fx / cam.fy;
        if (!(isfinite(a) && a > 0)) return DCX_E_ARG;
        sd.ratio = use_guess ? 0 : 1;
        sd.a = a;
        if (mk.free & 2u) {                                                       // fy free: fx rides on it
            mk.tie = 1;
            mk.a = a;
            mk.free &= ~1u;
        }
    }
    const bool rational = rational_flags(flags) || (use_guess && (cam.k[5] != 0.0 || cam.k[6] != 0.0 || cam.k[7] != 0.0));
    const FlagsCall a = {d_counts, d_starts, d_rows, d_xy, batch, pool, col_count, row_count, square_len, image_width, image_height,
                         d_workspace, workspace_bytes, d_view_status, d_pose, h_result, stream};
    return rational ? run<RationalCalib>(a, pl, sd, mk) : run<PinholeCalib>(a, pl, sd, mk);
}
