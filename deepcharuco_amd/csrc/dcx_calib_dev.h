// dcx_calib_dev.h -- the joint Levenberg-Marquardt of the single-camera calibrations, one text for both camera models:
// dcx_calib.hip (the pinhole with rational + tangential distortion, NG = 9 intrinsics) and dcx_fisheye.hip (the fisheye, NG = 8)
// instantiate the five kernels and the launch loop below on a model trait and keep what is theirs: the start (Zhang's init kernels
// there, Theta0 and the fisheye PnP solve here) and the C entries.
//
// The normal matrix is block-sparse: a view's 6 pose parameters couple only to the NG intrinsics.  Per view, [J_theta | J_pose | r]
// (NC = NG + 7 columns) gives a symmetric NC x NC [V_i W_i g_a,i; W_i^T U_i g_b,i; . . cost_i], NC (NC + 1) / 2 packed entries
// (136 at NG = 9, 120 at NG = 8).  Each LM attempt eliminates the 6x6 blocks (Schur complement) and solves one damped NG x NG system:
//   S = V* - sum W_i U_i*^-1 W_i^T,  dtheta = S^-1 (g_a - sum W_i U_i*^-1 g_b,i),  dpose_i = U_i*^-1 g_b,i - U_i*^-1 W_i^T dtheta.
//
// Launches (one 64-lane wave per view unless noted; grid = batch):
//   evaluate        after the start and after each accepted step: the view's packed entries.  The per-point rows of [J | r] are
//                   staged in LDS, 64 points at a time, and lane l sums the entries l, l + 64, l + 128 over them in point order
//                   (a 136-value butterfly would not fit the registers)
//   schur           per attempt: damping, 6x6 Cholesky of U_i*, U_i*^-1 [W_i^T | g_b,i], the view's part of S and of the rhs
//   reduce_solve    (one workgroup) the parts summed in a fixed order, diag(sum V) damped, NG x NG Cholesky -> dtheta
//   trial           the view's dpose, trial pose and trial cost, its share of |dp|^2 and |p|^2
//   decide          (one workgroup) accept or reject, lg, the stop test; a state word for the host, the outputs when done
// The LM loop runs on the host: it reads the state word after every attempt (the number of attempts depends on the data), so
// the call synchronises its stream and cannot be captured in a graph.  Every sum has a fixed order (no atomics): two calls on
// the same input give the same bits.  Nothing is allocated: the caller passes the workspace.
// Shared with dcx_stereo.hip through dcx_mat_dev.h: schur's body (schur_view), the lane's entries (lane_entries), the one-workgroup
// tree (block_tree), the workspace carver; evaluate's LDS-staged loop mirrors accumulate_rows there (see the kernel).  The camera
// models, their derivatives and the pose columns are dcx_camera_dev.h's and dcx_fisheye_dev.h's (project, pose_basis,
// pose_columns); the project_point() overloads below add the intrinsic columns.  The LM machinery is dcx_lm_dev.h's, shared with
// dcx_stereo.hip: the state and the accept / reject / forced / stop automaton (LmState<NG>, lm_decide with STOP_FORCED = false),
// decide's body (lm_decide_block), trial's prologue (lm_trial_pose), reduce_solve's entry -> source mapping (lm_source), the
// damping and the host loop (lm_run).  The reduction in front of the NG x NG solve (8 slices x 128, added serially) is this
// header's own: its order is part of the output bits.  The pool is dcx_pnp_dev.h's CornerPool (frame(b), frame_status), which its
// host check corner_pool() fills or refuses.
// dcx_calib_flags.hip (cv2's calibration flags and the rational model, NG = 12) is the third unit on this header.  Its sizes do not
// fit the two layout constants the other models share, so both are the model's: the LDS row stride of evaluate (17; 21 at NG = 12,
// NC = 19) and reduce_solve's split of its 1024 threads into view slices x entry slots (8 x 128; 4 x 256 at NG = 12, kTot = 180).
// The order of the view sum at NG = 12 is therefore: view b goes to slice b % 4, each slice adds its views in ascending b, the four
// slices are added serially 0..3.  The flags themselves are a linear map on the intrinsic columns that commutes with the Schur
// complement, so a flagged solve runs the per-view kernels as they are and only reduce_solve knows the mask (CalibMask below).
#pragma once
#include "dcx_fisheye_dev.h"
#include "dcx_pnp_dev.h"
#include "dcx_lm_dev.h"

// dcx_calib.hip's: Zhang's start up to K0, shared with dcx_calib_flags.hip (plain pointers: the types below are each unit's own)
__attribute__((visibility("hidden"))) void dcx_calib_zhang_start(const int32_t* d_counts, const int32_t* d_starts, const int32_t* d_rows, const float* d_xy, int batch, int pool,
                           int col_count, int row_count, double square_len, int image_width, int image_height, void* d_state,
                           double* d_init_rows, int32_t* d_view_status, double* d_pose, void* stream);

namespace {

constexpr int kRedThreads = kLmThreads;                   // one-workgroup reductions over views
constexpr int kSlices = kRedThreads / 128;                // reduce_solve: 8 view slices x 128 entry slots
constexpr int kState = 512;                               // bytes reserved for the state
constexpr int kLdsStride = 17;                            // a row's NC <= 16 values, padded to an odd stride

// ---- the models.  A model names its camera class, NG, theta -> camera, the cap on accepted steps and the doubles per view its
// start keeps in the workspace; every size of the solve follows from NG here and nowhere else.
template <int NG_, int STRIDE_ = kLdsStride, int SLICES_ = kSlices>
struct CalibSizes {
    static constexpr int NG = NG_;
    static constexpr int kLdsStride = STRIDE_;            // evaluate: a row's NC values, padded to an odd stride
    static constexpr int kSlices = SLICES_;               // reduce_solve: view slices ...
    static constexpr int kSlots = kRedThreads / SLICES_;  // ... x entry slots
    static constexpr int kResult = NG_ + 6 <= 16 ? 16 : 20;   // h_result's words (LmState's NR)
    static constexpr int NC = NG + 7;                     // a row: [J_theta (NG) | J_pose (6) | r]
    static constexpr int kEntries = NC * (NC + 1) / 2;    // the view's packed NC x NC
    static constexpr int kCost = kEntries - 1;            // pk<NC>(NC - 1, NC - 1)
    static constexpr int NQ = (kEntries + kLanes - 1) / kLanes;   // entries of one lane
    static constexpr int NS = NG * (NG + 1) / 2;          // packed NG x NG
    static constexpr int kYZ = 6 * NG + 6;                // U*^-1 W^T (6 x NG, row major) and U*^-1 g_b (6)
    static constexpr int kSC = NS + NG;                   // the view's part of S (NS packed) and of the rhs (NG)
    static constexpr int kTot = 2 * kSC;                  // sum V (NS), sum g_a (NG), sum S_i (NS), sum W U*^-1 g_b (NG)
    using State = LmState<NG, kResult>;                   // g = theta; result = h_result
    static_assert(sizeof(State) <= kState, "state");
    static_assert(NC < kLdsStride && kLdsStride % 2 == 1 && kTot <= kSlots && kSlices * kSlots == kRedThreads, "layout");
};

struct PinholeCalib : CalibSizes<9> {                     // fx fy cx cy k1 k2 p1 p2 k3
    using Camera = PnpCamera;
    static constexpr int kMaxIter = kJointMaxIter;
    static constexpr int kRows = 6;                       // the two init rows (a0, a1, b) x 2
    static __device__ __forceinline__ Camera camera(const double* th) { return camera_of(th); }
};

struct FisheyeCalib : CalibSizes<8> {                     // fx fy cx cy k1 k2 k3 k4
    using Camera = FisheyeCamera;
    static constexpr int kMaxIter = 100;                  // accepted steps (fisheye.CALIB_MAX_ITER): the start is cruder than Zhang's
    static constexpr int kRows = 0;
    static __device__ __forceinline__ Camera camera(const double* th) { return fisheye_camera_of(th); }
};

// The workspace: the state, then per view, in doubles.  `rows`, what the model's start keeps per view (M::kRows), is a member only
// where there is any: a kernel's argument block is then the one it had when each unit had a Ws of its own, and so is its code.
// (With a `rows` that the fisheye kernels never read, their reduce_solve loaded its pointers in other groups, 1900 instructions
// for 1899, and took 342.4 us for 336.3 on the 4,096-view pool: 78 % of the call, which then missed the parent's time.)
template <class M, bool ROWS = (M::kRows > 0)>
struct WsHead {
    typename M::State* st;
    double* rows;
};
template <class M>
struct WsHead<M, false> {
    typename M::State* st;
};
template <class M>
struct Ws : WsHead<M> {
    double *m, *yz, *sc, *pose, *trial_pose, *trial;          // trial = {cost, |dp|^2, |p|^2}
    int* fail;
};

// -> the bytes needed; *w (if given) = the parts of the workspace at base
template <class M>
size_t ws_layout(void* base, int batch, Ws<M>* w) {
    const size_t B = (size_t)batch;
    Carver c{(char*)base, 0};
    Ws<M> r;
    r.st = (typename M::State*)c.take<char>(kState);
    if constexpr (M::kRows > 0) r.rows = c.take<double>(B * M::kRows);
    r.m = c.take<double>(B * M::kEntries);
    r.yz = c.take<double>(B * M::kYZ);
    r.sc = c.take<double>(B * M::kSC);
    r.pose = c.take<double>(B * 6);
    r.trial_pose = c.take<double>(B * 6);
    r.trial = c.take<double>(B * 3);
    r.fail = c.take<int>(B);
    if (w) *w = r;
    return c.at;
}

// ---------------------------------------------------------------------------------------------------------------- LM

// One point's projection at (theta, pose) -> residual (ru, rv); with JAC its two rows of [J_theta | J_pose]: the intrinsic columns
// here (calib._project_full's, fisheye._project_full's), the model, its derivative and the pose columns by the headers.  false if
// the point is not in front of the camera.
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
    pose_columns(du, dv, mx, my, G, ju + PinholeCalib::NG, jv + PinholeCalib::NG);
    return true;
}

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
    pose_columns(du, dv, mx, my, G, ju + FisheyeCalib::NG, jv + FisheyeCalib::NG);
    return true;
}

template <class M>
__global__ __launch_bounds__(kLanes) void calib_evaluate_kernel(CornerPool pl, const int32_t* __restrict__ status, Ws<M> ws) {
    constexpr int NC = M::NC, NQ = M::NQ;
    __shared__ double sj[2 * kLanes][M::kLdsStride];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (ws.st->code != kNextEvaluate || status[b] != DCX_PNP_OK) return;
    const Frame f = pl.frame(b);
    const typename M::Camera cam = M::camera(ws.st->g);
    double p[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) p[i] = ws.pose[(long long)b * 6 + i];
    double R[9], G[2][9];
    pose_basis(p, R, G);
    int ea[NQ], eb[NQ];
    lane_entries<NC, NQ>(lane, ea, eb);
    double acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
    bool behind = false;
    // dcx_mat_dev.h's accumulate_rows<NC, NQ, 17>, spelt out: called through it, the code generation of both instantiations
    // moves, in opposite directions.  The pinhole kernel then shares the sine and cosine range reductions of pose_basis (46
    // instructions fewer, v_trig_preop_f64 12 -> 6, other opcode counts than the kernel has always had).  The fisheye kernel ran
    // the helper before it had this text and shares them through it, not here: 1760 instructions for 1718, 220 VGPRs for 176 (two
    // waves per SIMD either way), v_trig_preop_f64 12 for 6, every other fp opcode count equal, the same bits, and a calibration of
    // 4,096 views within the spread of the parent's own times.  The stereo solve runs the shared loop; a change
    // there is a change here.
    for (int c0 = 0; c0 < f.n; c0 += kLanes) {
        const int i = c0 + lane;
        double ju[NC], jv[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) ju[j] = jv[j] = 0.0;
        if (i < f.n) {
            double mx, my, u, v, ru, rv;
            f.load(i, mx, my, u, v);
            if (project_point<true>(cam, p, R, G, mx, my, u, v, ru, rv, ju, jv)) {
                ju[NC - 1] = ru;
                jv[NC - 1] = rv;
            } else {
                behind = true;
#pragma unroll
                for (int j = 0; j < NC; ++j) ju[j] = jv[j] = 0.0;
            }
        }
        __syncthreads();                     // the previous chunk's rows have been read
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            sj[2 * lane][j] = ju[j];
            sj[2 * lane + 1][j] = jv[j];
        }
        __syncthreads();
        const int rows = 2 * min(kLanes, f.n - c0);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            if (ea[q] < 0) continue;
            double s = acc[q];
            for (int r = 0; r < rows; ++r) s += sj[r][ea[q]] * sj[r][eb[q]];
            acc[q] = s;
        }
    }
    const bool inf = __any(behind);
    double* m = ws.m + (long long)b * M::kEntries;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int e = lane + kLanes * q;
        if (e < M::kEntries) m[e] = (e == M::kCost && inf) ? INFINITY : acc[q];
    }
}

template <class M>
__global__ __launch_bounds__(kLanes) void calib_schur_kernel(const int32_t* __restrict__ status, Ws<M> ws) {
    __shared__ double sy[M::NG + 1][6];      // U*^-1 W^T's NG columns, then U*^-1 g_b
    const int b = blockIdx.x, lane = threadIdx.x;
    if (ws.st->code == kFinished || status[b] != DCX_PNP_OK) return;
    const double scale = lm_damping(ws.st->lg);
    const bool ok = schur_view<M::NG>(ws.m + (long long)b * M::kEntries, scale, lane, sy, ws.yz + (long long)b * M::kYZ,
                                      ws.sc + (long long)b * M::kSC);
    if (lane == 0) ws.fail[b] = ok ? 0 : 1;
}

// What a flagged solve holds fixed (dcx_calib_flags.hip; calib.py's module docstring has the rules).  Bit i of `free`: theta[i] moves.
// tie: fx = a fy, with fy free and fx not.  The map T on the intrinsic columns (a times column fx added to column fy, fixed columns
// dropped) is applied to the sums, T^T (sum V) T and T^T (sum W U*^-1 W^T) T and both right-hand sides likewise, before the damping;
// a fixed parameter then gets a 1 on its diagonal, so its step is zero, and the step is scattered back to all NG slots.
struct CalibMask {
    unsigned free;
    int tie;
    double a;
};

// packed symmetric NG x NG P and the vector v under CalibMask's T, in place (thread 0's, on LDS)
template <int NG>
__device__ __forceinline__ void calib_mask_apply(double* P, double* v, const CalibMask& mk, double fixed_diag) {
    if (mk.tie) {
        const double p11 = P[pk<NG>(1, 1)] + mk.a * P[pk<NG>(0, 1)], p10 = P[pk<NG>(0, 1)] + mk.a * P[pk<NG>(0, 0)];
        P[pk<NG>(1, 1)] = p11 + mk.a * p10;
        for (int j = 2; j < NG; ++j) P[pk<NG>(1, j)] += mk.a * P[pk<NG>(0, j)];
        v[1] += mk.a * v[0];
    }
    for (int i = 0; i < NG; ++i) {
        if ((mk.free >> i) & 1u) continue;
        for (int j = 0; j < NG; ++j) P[pk<NG>(i, j)] = 0.0;
        P[pk<NG>(i, i)] = fixed_diag;
        v[i] = 0.0;
    }
}

__device__ __forceinline__ CalibMask calib_mask_of() { return CalibMask{}; }
__device__ __forceinline__ CalibMask calib_mask_of(const CalibMask& mk) { return mk; }

// Mask: nothing (the default solve: this kernel's argument block and code are the ones it has always had; the text stays in the
// kernel, as a function called from two kernels it compiles otherwise) or one CalibMask (a flagged solve)
template <class M, class... Mask>
__global__ __launch_bounds__(kRedThreads) void calib_reduce_solve_kernel(int batch, const int32_t* __restrict__ status, Ws<M> ws,
                                                                         Mask... mask) {
    constexpr bool MASKED = sizeof...(Mask) > 0;
    static_assert(sizeof...(Mask) <= 1, "mask");
    [[maybe_unused]] const CalibMask mk = calib_mask_of(mask...);
    constexpr int NG = M::NG, NS = M::NS, kSC = M::kSC, kTot = M::kTot, kSlices = M::kSlices;
    __shared__ double part[kSlices][kTot];
    __shared__ int bad[kSlices];
    // thread 0's small dense solve, indexed in loops: kept in LDS rather than in (scratch-backed) private arrays, and rolled, so it
    // is spelt out here and is not dcx_mat_dev.h's unrolled cholesky_factor / cholesky_substitute on registers
    __shared__ double tot[kTot], S[NS], L[NS], rhs[NG], y[NG], x[NG];
    typename M::State* st = ws.st;
    if (st->code == kFinished) return;
    const int t = threadIdx.x, e = t % M::kSlots, sl = t / M::kSlots;
    if (e < kTot) {
        const int src = lm_source<NG>(e);    // where entry e lives: in the view's packed entries (m) or in its Schur part (sc)
        double s = 0.0;
        int f = 0;
        for (int b = sl; b < batch; b += kSlices) {
            if (status[b] != DCX_PNP_OK) continue;
            s += e < kSC ? ws.m[(long long)b * M::kEntries + src] : ws.sc[(long long)b * kSC + src];
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
    if constexpr (MASKED) {
        calib_mask_apply<NG>(tot, tot + NS, mk, 1.0);
        calib_mask_apply<NG>(tot + kSC, tot + kSC + NS, mk, 0.0);
    }
    for (int a = 0; a < NG; ++a) {
        for (int c = a; c < NG; ++c) S[pk<NG>(a, c)] = tot[pk<NG>(a, c)] * (a == c ? scale : 1.0) - tot[kSC + pk<NG>(a, c)];
        rhs[a] = tot[NS + a] - tot[kSC + NS + a];
    }
    for (int i = 0; i < NG; ++i) {
        for (int j = 0; j <= i; ++j) {
            double s = S[pk<NG>(i, j)];
            for (int k = 0; k < j; ++k) s -= L[pk<NG>(i, k)] * L[pk<NG>(j, k)];
            if (i == j) {
                if (!(s > 0)) {
                    lm_fail(st, DCX_CALIB_DEGENERATE);
                    return;
                }
                L[pk<NG>(i, i)] = sqrt(s);
            } else {
                L[pk<NG>(i, j)] = s / L[pk<NG>(j, j)];
            }
        }
    }
    for (int i = 0; i < NG; ++i) {
        double s = rhs[i];
        for (int k = 0; k < i; ++k) s -= L[pk<NG>(i, k)] * y[k];
        y[i] = s / L[pk<NG>(i, i)];
    }
    for (int i = NG - 1; i >= 0; --i) {
        double s = y[i];
        for (int k = i + 1; k < NG; ++k) s -= L[pk<NG>(k, i)] * x[k];
        x[i] = s / L[pk<NG>(i, i)];
    }
    if constexpr (!MASKED) {
        for (int i = 0; i < NG; ++i) {
            st->dg[i] = x[i];
            st->g_trial[i] = st->g[i] - x[i];
        }
    } else {
        for (int i = 0; i < NG; ++i) {           // a fixed parameter keeps its bits
            const bool moves = (mk.free >> i) & 1u;
            st->dg[i] = moves ? x[i] : 0.0;
            st->g_trial[i] = moves ? st->g[i] - x[i] : st->g[i];
        }
        if (mk.tie) {
            st->dg[0] = mk.a * st->dg[1];
            st->g_trial[0] = mk.a * st->g_trial[1];
        }
    }
}


template <class M>
__global__ __launch_bounds__(kLanes) void calib_trial_kernel(CornerPool pl, const int32_t* __restrict__ status, Ws<M> ws) {
    constexpr int NG = M::NG;
    const int b = blockIdx.x, lane = threadIdx.x;
    if (ws.st->code == kFinished || status[b] != DCX_PNP_OK) return;
    // dcx_lm_dev.h's lm_trial_pose<NG>, spelt out: called through it, the pinhole kernel's SGPR spills rise from 38 to 62 (the 75
    // uniform doubles of yz, dtheta and the pose do not fit the scalar registers and the compiler then orders their loads
    // otherwise); the fisheye kernel, which ran the helper before it had this text, has 38 for 40 and 1022 instructions for 1096.
    // The stereo solve runs the shared prologue; a change there is a change here.
    const double* yz = ws.yz + (long long)b * M::kYZ;
    double p0[6], p[6];
    double dn = 0.0, pn = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double s = yz[6 * NG + k];
#pragma unroll
        for (int j = 0; j < NG; ++j) s -= yz[k * NG + j] * ws.st->dg[j];
        p0[k] = ws.pose[(long long)b * 6 + k];
        p[k] = p0[k] - s;
        dn += (p[k] - p0[k]) * (p[k] - p0[k]);
        pn += p0[k] * p0[k];
    }
    const typename M::Camera cam = M::camera(ws.st->g_trial);
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
template <class M>
__global__ __launch_bounds__(kRedThreads) void calib_decide_kernel(int batch, int init, const int32_t* __restrict__ status,
                                                                   double* __restrict__ pose, Ws<M> ws) {
    lm_decide_block<M::NG, false, M::kResult, M::kMaxIter>(
        ws.st, batch, init, ws.pose, ws.trial_pose, [&](int b) { return status[b] == DCX_PNP_OK; },
        [&](int b) { return ws.m[(long long)b * M::kEntries + M::kCost]; },
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

// ---------------------------------------------------------------------------------------------------------------- host

// What both *_calibrate_pool entries check in front of their own: the pool, the pointers, the image size (DCX_E_ARG), then the
// workspace (DCX_E_WS) -> 0 with pl and ws filled
template <class M>
inline int calib_args(const int32_t* d_counts, const int32_t* d_starts, const int32_t* d_rows, const float* d_xy, int batch, int pool,
                      int col_count, int row_count, double square_len, int image_width, int image_height, void* d_workspace,
                      size_t workspace_bytes, const int32_t* d_view_status, const double* d_pose, const double* h_result,
                      CornerPool& pl, Ws<M>& ws) {
    if (!corner_pool(d_counts, d_starts, d_rows, d_xy, batch, pool, col_count, row_count, square_len, pl)) return DCX_E_ARG;
    if (!d_workspace || !d_view_status || !d_pose || !h_result || image_width <= 0 || image_height <= 0) return DCX_E_ARG;
    if (workspace_bytes < ws_layout<M>(nullptr, batch, nullptr)) return DCX_E_WS;
    ws_layout(d_workspace, batch, &ws);
    return 0;
}

// The solve behind a model's start (the state at kNextEvaluate or kFinished, every used view's pose in ws.pose): evaluate and
// decide(init) queued, then one attempt per turn of lm_run until the state word says finished.
// launch_solve(): the attempt's reduce_solve, the default one or the masked one of a flagged call.
template <class M, class Solve>
inline hipError_t calib_lm(hipStream_t s, const CornerPool& pl, int batch, int32_t* d_view_status, double* d_pose, const Ws<M>& ws,
                           const Solve& launch_solve) {
    const dim3 views((unsigned)batch), wave(kLanes), one(1), red(kRedThreads);
    hipLaunchKernelGGL(calib_evaluate_kernel<M>, views, wave, 0, s, pl, d_view_status, ws);
    hipLaunchKernelGGL(calib_decide_kernel<M>, one, red, 0, s, batch, 1, d_view_status, d_pose, ws);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return lm_run(s, &ws.st->code, M::kMaxIter, [&](bool evaluate) {
        if (evaluate) hipLaunchKernelGGL(calib_evaluate_kernel<M>, views, wave, 0, s, pl, d_view_status, ws);
        hipLaunchKernelGGL(calib_schur_kernel<M>, views, wave, 0, s, d_view_status, ws);
        launch_solve();
        hipLaunchKernelGGL(calib_trial_kernel<M>, views, wave, 0, s, pl, d_view_status, ws);
        hipLaunchKernelGGL(calib_decide_kernel<M>, one, red, 0, s, batch, 0, d_view_status, d_pose, ws);
    });
}

template <class M>
inline hipError_t calib_lm(hipStream_t s, const CornerPool& pl, int batch, int32_t* d_view_status, double* d_pose, const Ws<M>& ws) {
    return calib_lm(s, pl, batch, d_view_status, d_pose, ws, [&] {
        hipLaunchKernelGGL(calib_reduce_solve_kernel<M>, dim3(1), dim3(kRedThreads), 0, s, batch, d_view_status, ws);
    });
}

}  // namespace
