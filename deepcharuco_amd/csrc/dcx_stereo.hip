// dcx_stereo.hip -- cv2.stereoCalibrate with CALIB_FIX_INTRINSIC for a planar ChArUco board, on the device, read straight from the
// two corner pools dcx_infer_batch writes for two rigidly mounted cameras: the rig transform X = (R, T), q1 = R q0 + T, and the
// board's pose P_t in camera 0's frame per timestamp.  The two views of a timestamp need no common id.  The steps (all fp64) are
// restated readably in deepcharuco_amd/stereo.py (stereo_calibrate_host_full), which is the pin of these kernels:
//   per-view checks (an optional per-slot mask drops rows first) -> every view's pose by the PnP solver (solve(), its camera's
//   model) -> a timestamp whose two views are OK is a pair -> rig init: R_t = R1_t R0_t^T, T_t = t1_t - R_t t0_t per pair, the
//   element-wise lower median over the pairs, the polar factor, rvec_of -> joint Levenberg-Marquardt over X (6) and every pair's
//   P_t (6), CvLevMarq's rules, at most 30 accepted steps, stop at |dp| / |p| < DBL_EPSILON.
//
// The normal matrix is block-sparse: a pair's P_t couples only to X.  Per pair, [J_X | J_P | r] (13 columns; J_X = 0 on camera 0's
// rows) gives a symmetric 13x13 [V_t W_t g_a,t; W_t^T U_t g_b,t; . . cost_t], 91 packed entries.  Each LM attempt eliminates the
// 6x6 blocks U_t (Schur complement) and solves one damped 6x6 system:
//   S = V* - sum W_t U_t*^-1 W_t^T,  dX = S^-1 (g_a - sum W_t U_t*^-1 g_b,t),  dP_t = U_t*^-1 g_b,t - U_t*^-1 W_t^T dX.
//
// Launches (one 64-lane wave per timestamp unless noted):
//   overlap         only for a pool with a mask (one wave per view against every other view): a view's kept rows are listed at its
//                   own slots of the workspace, so its views' slot ranges must not meet
//   ident           the index list 0, 1, 2, ... that a pool without a mask reads its rows through
//   init_views      grid (timestamp, camera): the checks; with a mask the kept rows compacted in order (ballot + prefix popcount,
//                   64 rows at a time) into an index list; solve() over an IndexedFrame either way, so a NULL mask and a mask of
//                   ones run the same instructions on the same values
//   pairs           (one lane per timestamp) which timestamps pair, their R_t, T_t, P_t = camera 0's pose
//   (host)          one copy of the T x 12 doubles and the pair flags; the lower medians by std::nth_element
//   rig             (one wave) the median matrix's polar factor, rvec_of -> X0; the state
//   evaluate        after the init and after each accepted step: the pair's 91 entries.  The lanes stride over camera 0's rows,
//                   then camera 1's; the per-row rows of [J | r] are staged in LDS, 64 rows at a time, and lane l sums the
//                   entries l and l + 64 over them in row order.  The row count is not capped
//   schur           per attempt: damping, 6x6 Cholesky of U_t*, U_t*^-1 [W_t^T | g_b,t], the pair's part of S and of the rhs
//   reduce          (one 64-lane block per kChunk = 16 timestamps) the block's 54 partial sums, each by one lane in order
//   reduce_solve    (one workgroup, kSlices = 16 slices x 64 entry slots) the partials summed slice-wise, the slices by a fixed
//                   tree, diag(sum V) damped, 6x6 Cholesky -> dX.  4,096 timestamps: 16 + 16 serial additions and 4 tree levels
//   trial           the pair's dP, trial pose and trial cost per camera, its share of |dp|^2 and |p|^2
//   decide          (one workgroup) accept or reject, lg, the stop test; a state word for the host, the outputs when done
// The LM loop runs on the host: it reads the state word after every attempt (the number of attempts depends on the data), so the
// call synchronises its stream and cannot be captured in a graph.  Every sum has a fixed order (no atomics): two calls on the same
// input give the same bits.  No device memory is allocated: the caller passes the workspace.
// Shared with dcx_calib.hip through dcx_mat_dev.h: evaluate's LDS-staged loop (accumulate_rows), schur's body (schur_view), the
// rig's polar_factor, block_tree, the workspace carver; overlap is dcx_pnp_dev.h's ranges_overlap, and each camera's pool is that
// header's CornerPool (both carry the board), filled by its host check corner_pool(), with the optional mask beside it
// (MaskedPool).  The camera model, its
// derivative and the pose columns are dcx_camera_dev.h's (project, pose_basis, pose_columns); stereo_row() adds the chain
// through R_X and the rig columns.  It, MaskedPool, the overlap and ident kernels, init_views' body (view_solve), the pairs
// kernel's relative_pose, accumulate_view and view_cost are dcx_stereo_dev.h's, shared with dcx_rig.hip (2 .. 8 cameras).  The LM machinery is dcx_lm_dev.h's, shared with dcx_calib.hip: the state and the accept /
// reject / forced / stop automaton (LmState<6>, lm_decide with STOP_FORCED = true: a step forced with a point behind a camera ends
// the solve), decide's body (lm_decide_block), trial's prologue (lm_trial_pose), reduce's entry -> source mapping (lm_source), the
// damping and the host loop (lm_run).  The two fan-ins kChunk / kSlices in front of the 6x6 solve are this unit's own: their order
// is part of the output bits.
#include "dcx_stereo_dev.h"

#include <algorithm>
#include <vector>

namespace {

constexpr int kRedThreads = kLmThreads;                       // decide's one-workgroup reduction over timestamps
constexpr int kChunk = 16;                                // reduce: timestamps per block (first fan-in)
constexpr int kSlices = 16;                               // reduce_solve: slices of the blocks' partials (second fan-in)
constexpr int kEntries = 91;                              // packed 13x13: [J_X (6) | J_P (6) | r]
constexpr int kCost = 90;                                 // pk<13>(12, 12)
constexpr int kTot = 54;                                  // sum V (21), sum g_a (6), sum S_t (21), sum W U*^-1 g_b (6)
constexpr int kYZ = 42;                                   // U*^-1 W^T (6 x 6, row major) and U*^-1 g_b (6)
constexpr int kSC = 27;                                   // the pair's part of S (21 packed) and of the rhs (6)

enum : int { kOverlap = 0, kHeadWords = 2 };

using StereoState = LmState<6>;          // g = X; result = h_result
constexpr int kState = 512;              // bytes reserved for StereoState
static_assert(sizeof(StereoState) <= kState, "state");

struct Med {
    double v[12];                        // the lower medians of R_t (9, row major) and T_t (3)
};

struct Ws {
    StereoState* st;
    double *m, *yz, *sc, *part, *pose, *trial_pose, *trial, *vpose, *rig;   // trial = {cost 0, cost 1, |dp|^2, |p|^2}
    int32_t *head, *pair, *fail, *pfail, *count, *idx0, *idx1, *ident;
};

inline int chunks_of(int batch) { return (batch + kChunk - 1) / kChunk; }

size_t ws_layout(void* base, int batch, int pool0, int pool1, Ws* w) {
    const size_t B = (size_t)batch, G = (size_t)chunks_of(batch);
    Carver c{(char*)base, 0};
    Ws r;
    r.st = (StereoState*)c.take<char>(kState);
    r.m = c.take<double>(B * kEntries);
    r.yz = c.take<double>(B * kYZ);
    r.sc = c.take<double>(B * kSC);
    r.part = c.take<double>(G * kTot);
    r.pose = c.take<double>(B * 6);
    r.trial_pose = c.take<double>(B * 6);
    r.trial = c.take<double>(B * 4);
    r.vpose = c.take<double>(B * 12);
    r.rig = c.take<double>(B * 12);
    r.head = c.take<int32_t>(kHeadWords);
    r.pair = c.take<int32_t>(B);
    r.fail = c.take<int32_t>(B);
    r.pfail = c.take<int32_t>(G);
    r.count = c.take<int32_t>(B * 2);
    r.idx0 = c.take<int32_t>((size_t)pool0);
    r.idx1 = c.take<int32_t>((size_t)pool1);
    r.ident = c.take<int32_t>((size_t)(pool0 > pool1 ? pool0 : pool1));
    if (w) *w = r;
    return c.at;
}

bool sizes_ok(int batch, int pool0, int pool1) { return batch > 0 && pool0 >= 0 && pool1 >= 0; }

// View (t, c) as the later kernels read it: its kept rows through the index list init_views left.
__device__ __forceinline__ IndexedFrame view_frame(const MaskedPool& pl, const Ws& ws, int t, int c) {
    const long long s0 = pl.p.starts[t];
    return IndexedFrame{pl.p.frame(pl.p.counts[t], s0), pl.mask ? (c ? ws.idx1 : ws.idx0) + s0 : ws.ident, ws.count[2 * t + c]};
}

// ---------------------------------------------------------------------------------------------------------------- init

// CAM, here and in evaluate and trial: PnpCamera, or AnyCamera for a pair with a fisheye camera in it
// (dcx_stereo_calibrate_models_pool).  The kernels' text knows no model: on AnyCamera it is chosen inside the step, by the AnyCamera
// overloads of view_solve, accumulate_view and view_cost (dcx_stereo_dev.h); the tags are kernel arguments, so every branch is uniform.
template <class CAM>
__global__ __launch_bounds__(kLanes) void stereo_init_views_kernel(MaskedPool pl0, MaskedPool pl1, CAM cam0, CAM cam1,
                                                                   int32_t* __restrict__ status, double* __restrict__ view_info,
                                                                   Ws ws) {
    const int t = blockIdx.x, c = blockIdx.y, lane = threadIdx.x;
    const MaskedPool pl = c ? pl1 : pl0;
    double out[8];
    int kept;
    const int st = view_solve(pl, c ? cam1 : cam0, t, c ? ws.idx1 : ws.idx0, ws.ident, out, kept);
    if (lane == 0) {
        const long long v = 2 * (long long)t + c;
        status[v] = st;
        view_info[2 * v] = 0.0;
        view_info[2 * v + 1] = (double)kept;
        ws.count[v] = kept;
#pragma unroll
        for (int i = 0; i < 6; ++i) ws.vpose[6 * v + i] = st == DCX_PNP_OK ? out[i] : 0.0;
    }
}

__global__ __launch_bounds__(kLanes) void stereo_pairs_kernel(int batch, const int32_t* __restrict__ status,
                                                              double* __restrict__ pose, Ws ws) {
    const int t = blockIdx.x * kLanes + threadIdx.x;
    if (t >= batch) return;
    const bool pr = status[2 * (long long)t] == DCX_PNP_OK && status[2 * (long long)t + 1] == DCX_PNP_OK;
    ws.pair[t] = pr ? 1 : 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) pose[8 * (long long)t + i] = 0.0;
    double p0[6], p1[6], rig[12];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        p0[i] = ws.vpose[12 * (long long)t + i];
        p1[i] = ws.vpose[12 * (long long)t + 6 + i];
    }
    relative_pose(p0, p1, rig);
#pragma unroll
    for (int i = 0; i < 12; ++i) ws.rig[12 * (long long)t + i] = pr ? rig[i] : 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) ws.pose[6 * (long long)t + i] = pr ? p0[i] : 0.0;
}

__global__ __launch_bounds__(kLanes) void stereo_rig_kernel(Med med, int npairs, int batch, Ws ws) {
    StereoState* st = ws.st;
    const bool writer = threadIdx.x == 0;
    double points[1] = {0.0};            // the rows of the pairs found: reported whatever the status
    for (int t = threadIdx.x; t < batch; t += kLanes)
        if (ws.pair[t]) points[0] += (double)(ws.count[2 * t] + ws.count[2 * t + 1]);
    wave_sum(points);
    if (writer) {
        lm_reset(st);
        st->result[9] = (double)npairs;
        st->result[10] = points[0];
        st->code = kFinished;
    }
    if (npairs == 0) {
        if (writer) st->result[11] = DCX_STEREO_NO_PAIRS;
        return;
    }
    // the median matrix's polar factor, as init_pose orthonormalises its decomposition
    double Q[9], x[6];
    if (!polar_factor(med.v, Q)) {
        if (writer) st->result[11] = DCX_STEREO_DEGENERATE;
        return;
    }
    rvec_of(Q, x);
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) x[3 + i] = med.v[9 + i];
#pragma unroll
    for (int i = 0; i < 6; ++i) finite &= isfinite(x[i]);
    if (!writer) return;
    if (!finite) {
        st->result[11] = DCX_STEREO_NONFINITE;
        return;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) st->g[i] = x[i];
    st->code = kNextEvaluate;
}

// ---------------------------------------------------------------------------------------------------------------- LM

template <class CAM>
__global__ __launch_bounds__(kLanes) void stereo_evaluate_kernel(MaskedPool pl0, MaskedPool pl1, CAM cam0, CAM cam1, Ws ws) {
    __shared__ double sj[2 * kLanes][kLdsStride];
    const int t = blockIdx.x, lane = threadIdx.x;
    if (ws.st->code != kNextEvaluate || !ws.pair[t]) return;
    double x[6], p[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        x[i] = ws.st->g[i];
        p[i] = ws.pose[(long long)t * 6 + i];
    }
    PairBasis B;
    pair_basis<true>(x, p, B);
    int ea[2], eb[2];
    lane_entries<13, 2>(lane, ea, eb);
    double acc[2] = {0, 0};
    bool behind = false;
    accumulate_view<false>(view_frame(pl0, ws, t, 0), cam0, B, sj, ea, eb, acc, behind);
    accumulate_view<true>(view_frame(pl1, ws, t, 1), cam1, B, sj, ea, eb, acc, behind);
    const bool inf = __any(behind);
    double* m = ws.m + (long long)t * kEntries;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int e = lane + kLanes * q;
        if (e < kEntries) m[e] = (e == kCost && inf) ? INFINITY : acc[q];
    }
}

__global__ __launch_bounds__(kLanes) void stereo_schur_kernel(Ws ws) {
    __shared__ double sy[7][6];              // U*^-1 W^T's 6 columns, then U*^-1 g_b
    const int t = blockIdx.x, lane = threadIdx.x;
    if (ws.st->code == kFinished || !ws.pair[t]) return;
    const double scale = lm_damping(ws.st->lg);
    const bool ok = schur_view<6>(ws.m + (long long)t * kEntries, scale, lane, sy, ws.yz + (long long)t * kYZ,
                                  ws.sc + (long long)t * kSC);
    if (lane == 0) ws.fail[t] = ok ? 0 : 1;
}

// First fan-in: block g sums the kTot values over its kChunk timestamps, lane e one value in timestamp order.
__global__ __launch_bounds__(kLanes) void stereo_reduce_kernel(int batch, Ws ws) {
    if (ws.st->code == kFinished) return;
    const int g = blockIdx.x, e = threadIdx.x;
    const int src = lm_source<6>(e);         // where value e lives: in the pair's 91 (m) or in its Schur part (sc)
    double s = 0.0;
    int f = 0;
    const int end = min(batch, (g + 1) * kChunk);
    for (int t = g * kChunk; t < end; ++t) {
        if (!ws.pair[t]) continue;
        if (e < kTot) s += e < 27 ? ws.m[(long long)t * kEntries + src] : ws.sc[(long long)t * kSC + src];
        if (e == 0) f |= ws.fail[t];
    }
    if (e < kTot) ws.part[(long long)g * kTot + e] = s;
    if (e == 0) ws.pfail[g] = f;
}

// Second fan-in and the solve: slice sl sums the blocks sl, sl + kSlices, ... in order, the slices meet in a fixed tree.
__global__ __launch_bounds__(kSlices * kLanes) void stereo_reduce_solve_kernel(int chunks, Ws ws) {
    __shared__ double part[kSlices][kLanes];
    __shared__ int bad[kSlices];
    StereoState* st = ws.st;
    if (st->code == kFinished) return;
    const int t = threadIdx.x, e = t % kLanes, sl = t / kLanes;
    double s = 0.0;
    int f = 0;
    for (int g = sl; g < chunks; g += kSlices) {
        if (e < kTot) s += ws.part[(long long)g * kTot + e];
        if (e == 0) f |= ws.pfail[g];
    }
    part[sl][e] = s;
    if (e == 0) bad[sl] = f;
    for (int h = kSlices / 2; h >= 1; h >>= 1) {
        __syncthreads();
        if (sl < h) {
            part[sl][e] += part[sl + h][e];
            if (e == 0) bad[sl] |= bad[sl + h];
        }
    }
    __syncthreads();
    if (t != 0) return;
    if (bad[0]) {
        lm_fail(st, DCX_STEREO_DEGENERATE);
        return;
    }
    const double scale = lm_damping(st->lg);
    double S[21], rhs[6], x[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int c = a; c < 6; ++c) S[pk<6>(a, c)] = part[0][pk<6>(a, c)] * (a == c ? scale : 1.0) - part[0][27 + pk<6>(a, c)];
        rhs[a] = part[0][21 + a] - part[0][48 + a];
    }
    if (!cholesky_solve(S, rhs, 1.0, x)) {
        lm_fail(st, DCX_STEREO_DEGENERATE);
        return;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        st->dg[i] = x[i];
        st->g_trial[i] = st->g[i] - x[i];
    }
}

template <class CAM>
__global__ __launch_bounds__(kLanes) void stereo_trial_kernel(MaskedPool pl0, MaskedPool pl1, CAM cam0, CAM cam1, Ws ws) {
    const int t = blockIdx.x, lane = threadIdx.x;
    if (ws.st->code == kFinished || !ws.pair[t]) return;
    double x[6], p[6], dn, pn;
    lm_trial_pose<6>(ws.yz + (long long)t * kYZ, ws.st->dg, ws.pose + (long long)t * 6, p, dn, pn);
#pragma unroll
    for (int k = 0; k < 6; ++k) x[k] = ws.st->g_trial[k];
    PairBasis B;
    pair_basis<false>(x, p, B);
    const double c0 = view_cost<false>(view_frame(pl0, ws, t, 0), cam0, B);
    const double c1 = view_cost<true>(view_frame(pl1, ws, t, 1), cam1, B);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) ws.trial_pose[(long long)t * 6 + k] = p[k];
        ws.trial[(long long)t * 4 + 0] = c0;
        ws.trial[(long long)t * 4 + 1] = c1;
        ws.trial[(long long)t * 4 + 2] = dn;
        ws.trial[(long long)t * 4 + 3] = pn;
    }
}

// init = 1: after the first evaluate (the initial cost); init = 0: after a trial
__global__ __launch_bounds__(kRedThreads) void stereo_decide_kernel(int batch, int init, double* __restrict__ pose,
                                                                    double* __restrict__ view_info, Ws ws) {
    lm_decide_block<6, true>(
        ws.st, batch, init, ws.pose, ws.trial_pose, [&](int b) { return ws.pair[b] != 0; },
        [&](int b) { return ws.m[(long long)b * kEntries + kCost]; },
        [&](int b, double* a) {
            const double* tr = ws.trial + (long long)b * 4;
            a[0] += tr[0] + tr[1]; a[1] += tr[2]; a[2] += tr[3];
        },
        [&](int b) { return (double)(ws.count[2 * b] + ws.count[2 * b + 1]); },
        [&](int b) {
            double* o = pose + 8 * (long long)b;
            const double* tr = ws.trial + (long long)b * 4;
            const double n0 = (double)ws.count[2 * b], n1 = (double)ws.count[2 * b + 1];
#pragma unroll
            for (int k = 0; k < 6; ++k) o[k] = ws.trial_pose[(long long)b * 6 + k];
            o[6] = sqrt((tr[0] + tr[1]) / (n0 + n1));
            o[7] = n0 + n1;
            view_info[4 * (long long)b] = sqrt(tr[0] / n0);
            view_info[4 * (long long)b + 2] = sqrt(tr[1] / n1);
        });
}

// Everything after the two cameras are made: the entry points' common body.
template <class CAM>
int stereo_calibrate(MaskedPool pl0, MaskedPool pl1, const CAM& cam0, const CAM& cam1, int batch, int pool0, int pool1,
                     void* d_workspace, size_t workspace_bytes, int32_t* d_view_status, double* d_pose, double* d_view_info,
                     double* h_result, void* stream) {
    const uint8_t *d_mask0 = pl0.mask, *d_mask1 = pl1.mask;
    if (workspace_bytes < ws_layout(nullptr, batch, pool0, pool1, nullptr)) return DCX_E_WS;
    Ws ws;
    ws_layout(d_workspace, batch, pool0, pool1, &ws);
    hipStream_t s = (hipStream_t)stream;
    const int chunks = chunks_of(batch);
    const dim3 stamps((unsigned)batch), views((unsigned)batch, 2), wave(kLanes), one(1), red(kRedThreads);
    const dim3 blocks((unsigned)chunks), per_lane((unsigned)((batch + kLanes - 1) / kLanes)), solve_threads(kSlices * kLanes);

    DCX_CHECK_HIP(hipMemsetAsync(ws.head, 0, kHeadWords * sizeof(int32_t), s));
    if (d_mask0) hipLaunchKernelGGL(stereo_overlap_kernel, stamps, wave, 0, s, pl0.p, batch, ws.head);
    if (d_mask1) hipLaunchKernelGGL(stereo_overlap_kernel, stamps, wave, 0, s, pl1.p, batch, ws.head);
    const int n_ident = !d_mask0 && !d_mask1 ? (pool0 > pool1 ? pool0 : pool1) : !d_mask0 ? pool0 : !d_mask1 ? pool1 : 0;
    if (n_ident > 0) hipLaunchKernelGGL(stereo_ident_kernel, dim3((unsigned)((n_ident + 255) / 256)), dim3(256), 0, s, n_ident, ws.ident);
    hipLaunchKernelGGL(stereo_init_views_kernel<CAM>, views, wave, 0, s, pl0, pl1, cam0, cam1, d_view_status, d_view_info, ws);
    hipLaunchKernelGGL(stereo_pairs_kernel, per_lane, wave, 0, s, batch, d_view_status, d_pose, ws);
    DCX_CHECK_HIP(hipGetLastError());

    // the rig init's medians, on the host: one copy of the pairs' R_t, T_t and flags (and the overlap word)
    std::vector<double> rig((size_t)batch * 12);
    std::vector<int32_t> pair((size_t)batch);
    int32_t head[kHeadWords] = {0, 0};
    DCX_CHECK_HIP(hipMemcpyAsync(rig.data(), ws.rig, rig.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    DCX_CHECK_HIP(hipMemcpyAsync(pair.data(), ws.pair, pair.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    DCX_CHECK_HIP(hipMemcpyAsync(head, ws.head, sizeof(head), hipMemcpyDeviceToHost, s));
    DCX_CHECK_HIP(hipStreamSynchronize(s));
    if (head[kOverlap]) return DCX_E_ARG;    // two views of a masked pool share slots
    Med med;
    int npairs = 0;
    {
        std::vector<double> col;
        col.reserve((size_t)batch);
        for (int e = 0; e < 12; ++e) {
            col.clear();
            for (int t = 0; t < batch; ++t)
                if (pair[(size_t)t]) col.push_back(rig[(size_t)t * 12 + e]);
            npairs = (int)col.size();
            med.v[e] = 0.0;
            if (npairs) {
                std::nth_element(col.begin(), col.begin() + (npairs - 1) / 2, col.end());
                med.v[e] = col[(size_t)(npairs - 1) / 2];
            }
        }
    }
    hipLaunchKernelGGL(stereo_rig_kernel, one, wave, 0, s, med, npairs, batch, ws);
    hipLaunchKernelGGL(stereo_evaluate_kernel<CAM>, stamps, wave, 0, s, pl0, pl1, cam0, cam1, ws);
    hipLaunchKernelGGL(stereo_decide_kernel, one, red, 0, s, batch, 1, d_pose, d_view_info, ws);
    DCX_CHECK_HIP(hipGetLastError());
    DCX_CHECK_HIP(lm_run(s, &ws.st->code, kJointMaxIter, [&](bool evaluate) {
        if (evaluate) hipLaunchKernelGGL(stereo_evaluate_kernel<CAM>, stamps, wave, 0, s, pl0, pl1, cam0, cam1, ws);
        hipLaunchKernelGGL(stereo_schur_kernel, stamps, wave, 0, s, ws);
        hipLaunchKernelGGL(stereo_reduce_kernel, blocks, wave, 0, s, batch, ws);
        hipLaunchKernelGGL(stereo_reduce_solve_kernel, one, solve_threads, 0, s, chunks, ws);
        hipLaunchKernelGGL(stereo_trial_kernel<CAM>, stamps, wave, 0, s, pl0, pl1, cam0, cam1, ws);
        hipLaunchKernelGGL(stereo_decide_kernel, one, red, 0, s, batch, 0, d_pose, d_view_info, ws);
    }));
    DCX_CHECK_HIP(hipMemcpyAsync(h_result, ws.st->result, 16 * sizeof(double), hipMemcpyDeviceToHost, s));
    DCX_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
}

// The two pools and the pointers every entry point checks before it makes its cameras -> false if anything is refused
bool pools_and_outputs(const int32_t* d_counts0, const int32_t* d_starts0, const int32_t* d_rows0, const float* d_xy0,
                       const int32_t* d_counts1, const int32_t* d_starts1, const int32_t* d_rows1, const float* d_xy1, int batch,
                       int pool0, int pool1, int col_count, int row_count, double square_len, const void* d_workspace,
                       const int32_t* d_view_status, const double* d_pose, const double* d_view_info, const double* h_result,
                       CornerPool& p0, CornerPool& p1) {
    if (!corner_pool(d_counts0, d_starts0, d_rows0, d_xy0, batch, pool0, col_count, row_count, square_len, p0) ||
        !corner_pool(d_counts1, d_starts1, d_rows1, d_xy1, batch, pool1, col_count, row_count, square_len, p1))
        return false;
    return d_workspace && d_view_status && d_pose && d_view_info && h_result && !((uintptr_t)d_workspace & 7);
}

}  // namespace

extern "C" size_t dcx_stereo_calibrate_workspace_bytes(int batch, int pool0, int pool1) {
    if (!sizes_ok(batch, pool0, pool1)) return 0;
    return ws_layout(nullptr, batch, pool0, pool1, nullptr);
}

extern "C" int dcx_stereo_calibrate_pool(const int32_t* d_counts0, const int32_t* d_starts0, const int32_t* d_rows0,
                                         const float* d_xy0, const uint8_t* d_mask0, const int32_t* d_counts1,
                                         const int32_t* d_starts1, const int32_t* d_rows1, const float* d_xy1,
                                         const uint8_t* d_mask1, int batch, int pool0, int pool1, int col_count, int row_count,
                                         double square_len, const double* h_camera9_0, const double* h_dist0, int n_dist0,
                                         const double* h_camera9_1, const double* h_dist1, int n_dist1, void* d_workspace,
                                         size_t workspace_bytes, int32_t* d_view_status, double* d_pose, double* d_view_info,
                                         double* h_result, void* stream) {
    MaskedPool pl0{{}, d_mask0}, pl1{{}, d_mask1};
    if (!pools_and_outputs(d_counts0, d_starts0, d_rows0, d_xy0, d_counts1, d_starts1, d_rows1, d_xy1, batch, pool0, pool1, col_count,
                           row_count, square_len, d_workspace, d_view_status, d_pose, d_view_info, h_result, pl0.p, pl1.p))
        return DCX_E_ARG;
    PnpCamera cam0, cam1;
    if (!pnp_camera(h_camera9_0, h_dist0, n_dist0, cam0) || !pnp_camera(h_camera9_1, h_dist1, n_dist1, cam1)) return DCX_E_ARG;
    return stereo_calibrate(pl0, pl1, cam0, cam1, batch, pool0, pool1, d_workspace, workspace_bytes, d_view_status, d_pose,
                            d_view_info, h_result, stream);
}

// model0 = model1 = DCX_CAMERA_PINHOLE: dcx_stereo_calibrate_pool, the same kernels on the same arguments.
extern "C" int dcx_stereo_calibrate_models_pool(const int32_t* d_counts0, const int32_t* d_starts0, const int32_t* d_rows0,
                                         const float* d_xy0, const uint8_t* d_mask0, const int32_t* d_counts1,
                                         const int32_t* d_starts1, const int32_t* d_rows1, const float* d_xy1,
                                         const uint8_t* d_mask1, int batch, int pool0, int pool1, int col_count, int row_count,
                                         double square_len, const double* h_camera9_0, const double* h_dist0, int n_dist0,
                                         const double* h_camera9_1, const double* h_dist1, int n_dist1, int model0, int model1, void* d_workspace,
                                         size_t workspace_bytes, int32_t* d_view_status, double* d_pose, double* d_view_info,
                                         double* h_result, void* stream) {
    if ((model0 != DCX_CAMERA_PINHOLE && model0 != DCX_CAMERA_FISHEYE) || (model1 != DCX_CAMERA_PINHOLE && model1 != DCX_CAMERA_FISHEYE))
        return DCX_E_ARG;
    if (model0 == DCX_CAMERA_PINHOLE && model1 == DCX_CAMERA_PINHOLE)
        return dcx_stereo_calibrate_pool(d_counts0, d_starts0, d_rows0, d_xy0, d_mask0, d_counts1, d_starts1, d_rows1, d_xy1, d_mask1,
                                         batch, pool0, pool1, col_count, row_count, square_len, h_camera9_0, h_dist0, n_dist0,
                                         h_camera9_1, h_dist1, n_dist1, d_workspace, workspace_bytes, d_view_status, d_pose,
                                         d_view_info, h_result, stream);
    MaskedPool pl0{{}, d_mask0}, pl1{{}, d_mask1};
    if (!pools_and_outputs(d_counts0, d_starts0, d_rows0, d_xy0, d_counts1, d_starts1, d_rows1, d_xy1, batch, pool0, pool1, col_count,
                           row_count, square_len, d_workspace, d_view_status, d_pose, d_view_info, h_result, pl0.p, pl1.p))
        return DCX_E_ARG;
    AnyCamera cam0, cam1;
    if (!any_camera(model0, h_camera9_0, h_dist0, n_dist0, cam0) || !any_camera(model1, h_camera9_1, h_dist1, n_dist1, cam1))
        return DCX_E_ARG;
    return stereo_calibrate(pl0, pl1, cam0, cam1, batch, pool0, pool1, d_workspace, workspace_bytes, d_view_status, d_pose,
                            d_view_info, h_result, stream);
}
