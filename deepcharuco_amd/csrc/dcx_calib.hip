// dcx_calib.hip -- cv2.calibrateCamera (default flags) for a planar board, on the device, read straight from the corner pool
// dcx_infer_batch writes (the views of a ChArUco board: id-labelled corners).  The steps (all fp64) are restated readably in
// deepcharuco_amd/calib.py (calibrate_camera_host_full), which is the pin of these kernels:
//   per-view checks -> initIntrinsicParams2D (principal point at the centre, per-view DLT homography, two rows per view in
//   (1/fx^2, 1/fy^2), least squares) -> every view's pose by the PnP solver (solve(), K0, no distortion) -> joint
//   Levenberg-Marquardt over theta = (fx, fy, cx, cy, k1, k2, p1, p2, k3) and every used view's (rvec, tvec), CvLevMarq's rules,
//   at most 30 accepted steps, stop at |dp| / |p| < DBL_EPSILON.
//
// The normal matrix is block-sparse: a view's 6 pose parameters couple only to the 9 intrinsics.  Per view, [J_theta | J_pose | r]
// (16 columns) gives a symmetric 16x16 [V_i W_i g_a,i; W_i^T U_i g_b,i; . . cost_i], 136 packed entries.  Each LM attempt
// eliminates the 6x6 blocks (Schur complement) and solves one damped 9x9 system:
//   S = V* - sum W_i U_i*^-1 W_i^T,  dtheta = S^-1 (g_a - sum W_i U_i*^-1 g_b,i),  dpose_i = U_i*^-1 g_b,i - U_i*^-1 W_i^T dtheta.
//
// Launches (one 64-lane wave per view unless noted; grid = batch):
//   init_views      per-view checks, the view's homography, its two init rows
//   init_reduce     (one workgroup) the rows reduced, the 2x2 least squares -> K0
//   init_poses      solve() with K0 and zero distortion
//   evaluate        after init and after each accepted step: the view's 136 entries.  The per-point rows of [J | r] are staged
//                   in LDS, 64 points at a time, and lane l sums the entries l, l + 64, l + 128 over them in point order
//                   (a 136-value butterfly would not fit the registers)
//   schur           per attempt: damping, 6x6 Cholesky of U_i*, U_i*^-1 [W_i^T | g_b,i], the view's part of S and of the rhs
//   reduce_solve    (one workgroup) the parts summed in a fixed order, diag(sum V) damped, 9x9 Cholesky -> dtheta
//   trial           the view's dpose, trial pose and trial cost, its share of |dp|^2 and |p|^2
//   decide          (one workgroup) accept or reject, lg, the stop test; a state word for the host, the outputs when done
// The LM loop runs on the host: it reads the state word after every attempt (the number of attempts depends on the data), so
// the call synchronises its stream and cannot be captured in a graph.  Every sum has a fixed order (no atomics): two calls on
// the same input give the same bits.  Nothing is allocated: the caller passes the workspace.
// Shared with dcx_stereo.hip through dcx_mat_dev.h: schur's body (schur_view), the lane's entries (lane_entries), the one-workgroup
// tree (block_tree), the workspace carver; evaluate's LDS-staged loop mirrors accumulate_rows there (see the kernel).  The camera
// model, its derivative and the pose columns are dcx_camera_dev.h's (project, pose_basis, pose_columns); project_point() below
// adds the nine intrinsic columns.  The LM machinery is dcx_lm_dev.h's, shared with dcx_stereo.hip: the state and the accept /
// reject / forced / stop automaton (LmState<9>, lm_decide with STOP_FORCED = false), decide's body (lm_decide_block), trial's
// prologue (lm_trial_pose), reduce_solve's entry -> source mapping (lm_source), the damping and the host loop (lm_run).  The
// reduction in front of the 9x9 solve (8 slices x 128, added serially) is this unit's own: its order is part of the output bits.
// The pool is dcx_pnp_dev.h's CornerPool (frame(b), frame_status), which its host check corner_pool() fills or refuses.
#include "dcx_pnp_dev.h"
#include "dcx_lm_dev.h"

namespace {

constexpr int kRedThreads = kLmThreads;                   // one-workgroup reductions over views
constexpr int kSlices = kRedThreads / 128;                // reduce_solve: 8 view slices x 128 entry slots
constexpr int kEntries = 136;                             // packed 16x16: [J_theta (9) | J_pose (6) | r]
constexpr int kCost = 135;                                // pk<16>(15, 15)

using CalibState = LmState<9>;             // g = theta; result = h_result

// per-view workspace, in doubles
constexpr int kRows = 6;                 // the two init rows (a0, a1, b) x 2
constexpr int kYZ = 60;                  // U*^-1 W^T (6 x 9, row major) and U*^-1 g_b (6)
constexpr int kSC = 54;                  // the view's part of S (45 packed) and of the rhs (9)
constexpr int kState = 512;              // bytes reserved for CalibState
static_assert(sizeof(CalibState) <= kState, "state");

struct Ws {
    CalibState* st;
    double *rows, *m, *yz, *sc, *pose, *trial_pose, *trial;   // trial = {cost, |dp|^2, |p|^2}
    int* fail;
};

// -> the bytes needed; *w (if given) = the parts of the workspace at base
size_t ws_layout(void* base, int batch, Ws* w) {
    const size_t B = (size_t)batch;
    Carver c{(char*)base, 0};
    Ws r;
    r.st = (CalibState*)c.take<char>(kState);
    r.rows = c.take<double>(B * kRows);
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

// ---------------------------------------------------------------------------------------------------------------- init

__global__ __launch_bounds__(kLanes) void calib_init_views_kernel(CornerPool pl, double cx, double cy, int32_t* __restrict__ status,
                                                                  double* __restrict__ pose, Ws ws) {
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
                                                                        const double* __restrict__ pose, Ws ws) {
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

__global__ __launch_bounds__(kLanes) void calib_init_poses_kernel(CornerPool pl, int32_t* __restrict__ status, Ws ws) {
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

// ---------------------------------------------------------------------------------------------------------------- LM

// One point's projection at (theta, pose) -> residual (ru, rv); with JAC its two rows of [J_theta | J_pose]: calib._project_full's
// intrinsic columns here, the model, its derivative and the pose columns by the header.  false if the point is not in front of
// the camera.
template <bool JAC>
__device__ __forceinline__ bool project_point(const PnpCamera& cam, const double* p, const double* R, const double (*G)[9], double mx,
                                              double my, double u, double v, double& ru, double& rv, double* ju, double* jv) {
    double q[3], du[3], dv[3], x, y, xd, yd;
    board_point(R, p + 3, mx, my, q);
    if (!project<JAC>(cam, q, u, v, ru, rv, du, dv, x, y, xd, yd)) return false;
    if (!JAC) return true;
    const double r2 = x * x + y * y;
    const double r4 = r2 * r2, r6 = r2 * r2 * r2;
    ju[0] = xd;  ju[1] = 0.0; ju[2] = 1.0; ju[3] = 0.0;
    jv[0] = 0.0; jv[1] = yd;  jv[2] = 0.0; jv[3] = 1.0;
    ju[4] = cam.fx * (x * r2);            jv[4] = cam.fy * (y * r2);
    ju[5] = cam.fx * (x * r4);            jv[5] = cam.fy * (y * r4);
    ju[6] = cam.fx * (2 * x * y);         jv[6] = cam.fy * (r2 + 2 * y * y);
    ju[7] = cam.fx * (r2 + 2 * x * x);    jv[7] = cam.fy * (2 * x * y);
    ju[8] = cam.fx * (x * r6);            jv[8] = cam.fy * (y * r6);
    pose_columns(du, dv, mx, my, G, ju + 9, jv + 9);
    return true;
}

constexpr int kLdsStride = 17;     // 16 values per row, padded

__global__ __launch_bounds__(kLanes) void calib_evaluate_kernel(CornerPool pl, const int32_t* __restrict__ status, Ws ws) {
    __shared__ double sj[2 * kLanes][kLdsStride];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (ws.st->code != kNextEvaluate || status[b] != DCX_PNP_OK) return;
    const Frame f = pl.frame(b);
    const PnpCamera cam = camera_of(ws.st->g);
    double p[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) p[i] = ws.pose[(long long)b * 6 + i];
    double R[9], G[2][9];
    pose_basis(p, R, G);
    int ea[3], eb[3];
    lane_entries<16, 3>(lane, ea, eb);
    double acc[3] = {0, 0, 0};
    bool behind = false;
    // dcx_mat_dev.h's accumulate_rows<16, 3, 17>, spelt out: called through it, this kernel's code generation moves (the compiler
    // then shares the sine and cosine range reductions of pose_basis: 46 instructions fewer, other opcode counts than before).  The
    // stereo solve runs the shared loop; a change there is a change here.
    for (int c0 = 0; c0 < f.n; c0 += kLanes) {
        const int i = c0 + lane;
        double ju[16], jv[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) ju[j] = jv[j] = 0.0;
        if (i < f.n) {
            double mx, my, u, v, ru, rv;
            f.load(i, mx, my, u, v);
            if (project_point<true>(cam, p, R, G, mx, my, u, v, ru, rv, ju, jv)) {
                ju[15] = ru;
                jv[15] = rv;
            } else {
                behind = true;
#pragma unroll
                for (int j = 0; j < 16; ++j) ju[j] = jv[j] = 0.0;
            }
        }
        __syncthreads();                     // the previous chunk's rows have been read
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            sj[2 * lane][j] = ju[j];
            sj[2 * lane + 1][j] = jv[j];
        }
        __syncthreads();
        const int rows = 2 * min(kLanes, f.n - c0);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if (ea[q] < 0) continue;
            double s = acc[q];
            for (int r = 0; r < rows; ++r) s += sj[r][ea[q]] * sj[r][eb[q]];
            acc[q] = s;
        }
    }
    const bool inf = __any(behind);
    double* m = ws.m + (long long)b * kEntries;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int e = lane + kLanes * q;
        if (e < kEntries) m[e] = (e == kCost && inf) ? INFINITY : acc[q];
    }
}

__global__ __launch_bounds__(kLanes) void calib_schur_kernel(const int32_t* __restrict__ status, Ws ws) {
    __shared__ double sy[10][6];             // U*^-1 W^T's 9 columns, then U*^-1 g_b
    const int b = blockIdx.x, lane = threadIdx.x;
    if (ws.st->code == kFinished || status[b] != DCX_PNP_OK) return;
    const double scale = lm_damping(ws.st->lg);
    const bool ok = schur_view<9>(ws.m + (long long)b * kEntries, scale, lane, sy, ws.yz + (long long)b * kYZ,
                                  ws.sc + (long long)b * kSC);
    if (lane == 0) ws.fail[b] = ok ? 0 : 1;
}

__global__ __launch_bounds__(kRedThreads) void calib_reduce_solve_kernel(int batch, const int32_t* __restrict__ status, Ws ws) {
    constexpr int kTot = 108;                // sum V (45), sum g_a (9), sum S_i (45), sum W U*^-1 g_b (9)
    __shared__ double part[kSlices][kTot];
    __shared__ int bad[kSlices];
    // thread 0's small dense solve, indexed in loops: kept in LDS rather than in (scratch-backed) private arrays, and rolled, so it
    // is spelt out here and is not the header's unrolled cholesky_factor / cholesky_substitute on registers
    __shared__ double tot[kTot], S[45], L[45], rhs[9], y[9], x[9];
    CalibState* st = ws.st;
    if (st->code == kFinished) return;
    const int t = threadIdx.x, e = t % 128, sl = t / 128;
    if (e < kTot) {
        const int src = lm_source<9>(e);     // where entry e lives: in the view's 136 (m) or in its Schur part (sc)
        double s = 0.0;
        int f = 0;
        for (int b = sl; b < batch; b += kSlices) {
            if (status[b] != DCX_PNP_OK) continue;
            s += e < 54 ? ws.m[(long long)b * kEntries + src] : ws.sc[(long long)b * kSC + src];
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
    for (int a = 0; a < 9; ++a) {
        for (int c = a; c < 9; ++c) S[pk<9>(a, c)] = tot[pk<9>(a, c)] * (a == c ? scale : 1.0) - tot[54 + pk<9>(a, c)];
        rhs[a] = tot[45 + a] - tot[99 + a];
    }
    for (int i = 0; i < 9; ++i) {
        for (int j = 0; j <= i; ++j) {
            double s = S[pk<9>(i, j)];
            for (int k = 0; k < j; ++k) s -= L[pk<9>(i, k)] * L[pk<9>(j, k)];
            if (i == j) {
                if (!(s > 0)) {
                    lm_fail(st, DCX_CALIB_DEGENERATE);
                    return;
                }
                L[pk<9>(i, i)] = sqrt(s);
            } else {
                L[pk<9>(i, j)] = s / L[pk<9>(j, j)];
            }
        }
    }
    for (int i = 0; i < 9; ++i) {
        double s = rhs[i];
        for (int k = 0; k < i; ++k) s -= L[pk<9>(i, k)] * y[k];
        y[i] = s / L[pk<9>(i, i)];
    }
    for (int i = 8; i >= 0; --i) {
        double s = y[i];
        for (int k = i + 1; k < 9; ++k) s -= L[pk<9>(k, i)] * x[k];
        x[i] = s / L[pk<9>(i, i)];
    }
    for (int i = 0; i < 9; ++i) {
        st->dg[i] = x[i];
        st->g_trial[i] = st->g[i] - x[i];
    }
}

__global__ __launch_bounds__(kLanes) void calib_trial_kernel(CornerPool pl, const int32_t* __restrict__ status, Ws ws) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (ws.st->code == kFinished || status[b] != DCX_PNP_OK) return;
    // dcx_lm_dev.h's lm_trial_pose<9>, spelt out: called through it, this kernel's SGPR spills rise from 38 to 62 (the 75 uniform
    // doubles of yz, dtheta and the pose do not fit the scalar registers and the compiler then orders their loads otherwise).  The
    // stereo solve runs the shared prologue; a change there is a change here.
    const double* yz = ws.yz + (long long)b * kYZ;
    double p0[6], p[6];
    double dn = 0.0, pn = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double s = yz[54 + k];
#pragma unroll
        for (int j = 0; j < 9; ++j) s -= yz[k * 9 + j] * ws.st->dg[j];
        p0[k] = ws.pose[(long long)b * 6 + k];
        p[k] = p0[k] - s;
        dn += (p[k] - p0[k]) * (p[k] - p0[k]);
        pn += p0[k] * p0[k];
    }
    const PnpCamera cam = camera_of(ws.st->g_trial);
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
__global__ __launch_bounds__(kRedThreads) void calib_decide_kernel(int batch, int init, const int32_t* __restrict__ status,
                                                                   double* __restrict__ pose, Ws ws) {
    lm_decide_block<9, false>(
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

}  // namespace

extern "C" size_t dcx_calibrate_workspace_bytes(int batch) { return batch > 0 ? ws_layout(nullptr, batch, nullptr) : 0; }

extern "C" int dcx_calibrate_pool(const int32_t* d_counts, const int32_t* d_starts, const int32_t* d_rows, const float* d_xy,
                                  int batch, int pool, int col_count, int row_count, double square_len, int image_width,
                                  int image_height, void* d_workspace, size_t workspace_bytes, int32_t* d_view_status,
                                  double* d_pose, double* h_result, void* stream) {
    CornerPool pl;
    if (!corner_pool(d_counts, d_starts, d_rows, d_xy, batch, pool, col_count, row_count, square_len, pl)) return DCX_E_ARG;
    if (!d_workspace || !d_view_status || !d_pose || !h_result || image_width <= 0 || image_height <= 0) return DCX_E_ARG;
    if (workspace_bytes < ws_layout(nullptr, batch, nullptr)) return DCX_E_WS;
    hipStream_t s = (hipStream_t)stream;
    Ws ws;
    ws_layout(d_workspace, batch, &ws);
    const double cx = (image_width - 1) * 0.5, cy = (image_height - 1) * 0.5;
    const dim3 views((unsigned)batch), wave(kLanes), one(1), red(kRedThreads);
    hipLaunchKernelGGL(calib_init_views_kernel, views, wave, 0, s, pl, cx, cy, d_view_status, d_pose, ws);
    hipLaunchKernelGGL(calib_init_reduce_kernel, one, red, 0, s, batch, cx, cy, d_view_status, d_pose, ws);
    hipLaunchKernelGGL(calib_init_poses_kernel, views, wave, 0, s, pl, d_view_status, ws);
    hipLaunchKernelGGL(calib_evaluate_kernel, views, wave, 0, s, pl, d_view_status, ws);
    hipLaunchKernelGGL(calib_decide_kernel, one, red, 0, s, batch, 1, d_view_status, d_pose, ws);
    DCX_CHECK_HIP(hipGetLastError());
    DCX_CHECK_HIP(lm_run(s, &ws.st->code, kJointMaxIter, [&](bool evaluate) {
        if (evaluate) hipLaunchKernelGGL(calib_evaluate_kernel, views, wave, 0, s, pl, d_view_status, ws);
        hipLaunchKernelGGL(calib_schur_kernel, views, wave, 0, s, d_view_status, ws);
        hipLaunchKernelGGL(calib_reduce_solve_kernel, one, red, 0, s, batch, d_view_status, ws);
        hipLaunchKernelGGL(calib_trial_kernel, views, wave, 0, s, pl, d_view_status, ws);
        hipLaunchKernelGGL(calib_decide_kernel, one, red, 0, s, batch, 0, d_view_status, d_pose, ws);
    }));
    DCX_CHECK_HIP(hipMemcpyAsync(h_result, ws.st->result, 16 * sizeof(double), hipMemcpyDeviceToHost, s));
    DCX_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
}
