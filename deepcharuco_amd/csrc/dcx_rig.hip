// dcx_rig.hip -- joint extrinsic calibration of a rig of C = 2 .. 8 rigidly mounted cameras, on the device, read straight from the C
// corner pools dcx_infer_batch writes: X_c = (R_c, T_c), q_c = R_c q_0 + T_c, for c = 1 .. C - 1 and the board's pose P_t in camera
// 0's frame per timestamp.  dcx_stereo.hip with n = 6 (C - 1) shared parameters in place of its 6.  The steps (all fp64) are
// restated readably in deepcharuco_amd/rig.py (rig_calibrate_host_full), which is the pin of these kernels:
//   per-view checks and poses as in dcx_stereo.hip -> a view is usable if it is OK, a timestamp is used if two of its views are ->
//   the camera graph (cameras share a timestamp where both are usable), walked breadth first from camera 0, children ascending ->
//   per tree edge the stereo rig init over the shared timestamps (lower medians, polar factor, rvec_of), composed along the tree ->
//   P_t from the timestamp's lowest usable camera -> joint Levenberg-Marquardt over all X_c and every used P_t, CvLevMarq's rules,
//   at most 30 accepted steps, stop at |dp| / |p| < DBL_EPSILON.
//
// The normal matrix is block-sparse: P_t couples only to the X_c of the cameras that saw timestamp t, and X_c only to itself.  Per
// usable view (t, c), [J_Xc | J_P | r] (13 columns; J_X = 0 for camera 0) gives dcx_stereo.hip's packed 13x13, 91 entries.  Per
// attempt the 6x6 blocks U_t = sum_c U_t,c are eliminated and one damped n x n system remains:
//   S = V* - sum_t W_t U_t*^-1 W_t^T,  dX = S^-1 (g_a - sum_t W_t U_t*^-1 g_b,t),  dP_t = U_t*^-1 g_b,t - U_t*^-1 W_t^T dX,
// V block diagonal (one 6x6 per camera), W_t the stacked W_t,c (zero for a camera that did not see t).
//
// Launches (one 64-lane wave per unit unless noted):
//   overlap, ident  dcx_stereo_dev.h's, per pool with / without a mask
//   init_views      grid (timestamp, camera): dcx_stereo_dev.h's view_solve
//   stamps          (one lane per timestamp) which timestamps are used and their rows; d_pose zeroed
//   (host)          one copy of the statuses and row counts: the tree (integers only), the counts; NO_STAMPS / DISCONNECTED end here
//   edges           grid (64 timestamps, tree edge): R_t, T_t of parent -> child where both are usable
//   (host)          one copy of them; per edge the lower medians over its shared timestamps by std::nth_element
//   start           (one wave) per edge, in placement order, the polar factor, rvec_of, the composition with the parent's X; then
//                   P_t's start, the lanes striding over the timestamps; the state
//   evaluate        grid (timestamp, camera): a usable view's 91 entries through accumulate_view; the row count is not capped
//   schur           per timestamp: U_t and g_b,t summed over the usable cameras ascending, damping, one 6x6 Cholesky, lane 6 (c - 1)
//                   + j solves column j of Y_c = U*^-1 W_c^T, lane n solves z = U*^-1 g_b; then the lanes stride over the
//                   n (n + 1) / 2 + n entries of the timestamp's part of S (W_c Y_c') and of the rhs (W_c z); a camera missing from
//                   the timestamp has W_c = Y_c = 0 exactly
//   reduce          (one 256-thread block per kChunk = 16 timestamps) every entry of sum V (21 per camera), sum g_a (n), sum S_t,
//                   sum rhs_t over the block's timestamps in order, by one thread
//   reduce_solve    (one workgroup, kSlices = 16 slices x 64 entry slots, 64 entries at a time) slice s sums the blocks s,
//                   s + kSlices, ... in order, the slices meet in a fixed tree; then the damped n x n system by Cholesky in LDS with
//                   run-time n: column by column, each entry updated by one thread in column order -> dX
//   trial           grid (timestamp, camera): dP_t = z - sum_c Y_c dX_c (cameras ascending), the view's trial cost; camera 0's block
//                   also writes the trial pose and the timestamp's share of |dp|^2 and |p|^2
//   decide          (one workgroup) lm_decide_block with STOP_FORCED
// init_views, evaluate and trial, the three that meet a camera, are templates on the camera table (dcx_stereo_dev.h): RigCams, or
// MixedCams for a rig with a fisheye camera in it (dcx_rig_calibrate_models_pool).  The kernels' text knows no model: on a table of AnyCamera the model is
// chosen per view, inside the step (the AnyCamera overloads of view_solve, accumulate_view and view_cost in dcx_stereo_dev.h), and
// uniformly per workgroup, which works on camera blockIdx.y alone.  The other launches never see a camera.
// The LM loop runs on the host (lm_run): the call synchronises its stream and cannot be captured in a graph.  Every sum has a fixed
// order (no atomics): two calls on the same input give the same bits.  No device memory is allocated.
// The state is LmState<42, 48> whatever C is: the parameters past n stay zero, which adds exact zeros to lm_decide's two norms.
#include "dcx_stereo_dev.h"

#include <algorithm>
#include <vector>

namespace {

constexpr int kMaxG = 6 * (kMaxCams - 1);                 // 42 shared parameters at the most
constexpr int kResWords = 48;                             // LmState::result: g (42), rms, steps, attempts, stamps, points, status
constexpr int kRedThreads = kLmThreads;                   // decide's one-workgroup reduction over timestamps
constexpr int kChunk = 16;                                // reduce: timestamps per block (first fan-in)
constexpr int kSlices = 16;                               // reduce_solve: slices of the blocks' partials (second fan-in)
constexpr int kEntries = 91;                              // packed 13x13: [J_Xc (6) | J_P (6) | r]
constexpr int kCost = 90;                                 // pk<13>(12, 12)
constexpr int kReduceThreads = 256;
constexpr int kMaxTot = 21 * (kMaxCams - 1) + kMaxG + kMaxG * (kMaxG + 1) / 2 + kMaxG;   // 1134

enum : int { kOverlap = 0, kHeadWords = 2 };

using RigState = LmState<kMaxG, kResWords>;
constexpr int kState = 1536;             // bytes reserved for RigState
static_assert(sizeof(RigState) <= kState, "state");

struct Tree {
    int parent[kMaxCams];                // -1 for camera 0
    int order[kMaxCams];                 // the cameras in placement order; order[0] = 0
};

struct Med {
    double v[kMaxCams - 1][12];          // per camera c - 1: the lower medians of its edge's R_t (9, row major) and T_t (3)
};

struct Ws {
    RigState* st;
    // m [B][C][91]; y [B][C-1][6][6] (Y_c, row k = pose parameter, column j = parameter of X_c); z [B][6]; sc [B][ns + n];
    // part [G][tot]; trial [B][C + 2] = {cost per camera, |dp|^2, |p|^2}; vpose [B][C][6]; edge [B][C-1][12]
    double *m, *y, *z, *sc, *part, *pose, *trial_pose, *trial, *vpose, *edge;
    int32_t *head, *used, *rows, *fail, *pfail, *count, *ident;   // rows [B]: the rows of a used timestamp's usable views
    int32_t* idx[kMaxCams];
    int C, n, ns, tot;                   // cameras; 6 (C - 1); n (n + 1) / 2; 21 (C - 1) + n + ns + n
};

inline int chunks_of(int batch) { return (batch + kChunk - 1) / kChunk; }

size_t ws_layout(void* base, int C, int batch, const int* pools, Ws* w) {
    const size_t B = (size_t)batch, G = (size_t)chunks_of(batch), Cm = (size_t)(C - 1);
    Carver c{(char*)base, 0};
    Ws r;
    r.C = C;
    r.n = 6 * (C - 1);
    r.ns = r.n * (r.n + 1) / 2;
    r.tot = 21 * (C - 1) + r.n + r.ns + r.n;
    r.st = (RigState*)c.take<char>(kState);
    r.m = c.take<double>(B * C * kEntries);
    r.y = c.take<double>(B * Cm * 36);
    r.z = c.take<double>(B * 6);
    r.sc = c.take<double>(B * (size_t)(r.ns + r.n));
    r.part = c.take<double>(G * (size_t)r.tot);
    r.pose = c.take<double>(B * 6);
    r.trial_pose = c.take<double>(B * 6);
    r.trial = c.take<double>(B * (size_t)(C + 2));
    r.vpose = c.take<double>(B * C * 6);
    r.edge = c.take<double>(B * Cm * 12);
    r.head = c.take<int32_t>(kHeadWords);
    r.used = c.take<int32_t>(B);
    r.rows = c.take<int32_t>(B);
    r.fail = c.take<int32_t>(B);
    r.pfail = c.take<int32_t>(G);
    r.count = c.take<int32_t>(B * C);
    int most = 0;
    for (int k = 0; k < kMaxCams; ++k) {
        r.idx[k] = k < C ? c.take<int32_t>((size_t)pools[k]) : nullptr;
        if (k < C && pools[k] > most) most = pools[k];
    }
    r.ident = c.take<int32_t>((size_t)most);
    if (w) *w = r;
    return c.at;
}

bool sizes_ok(int C, int batch, const int* pools) {
    if (C < 2 || C > kMaxCams || batch <= 0 || !pools) return false;
    for (int k = 0; k < C; ++k)
        if (pools[k] < 0) return false;
    return true;
}

__device__ __forceinline__ bool usable(const int32_t* status, const Ws& ws, int t, int c) {
    return status[(long long)t * ws.C + c] == DCX_PNP_OK;
}

// View (t, c) as the later kernels read it: its kept rows through the index list init_views left.
__device__ __forceinline__ IndexedFrame view_frame(const MaskedPool& pl, const Ws& ws, int t, int c) {
    const long long s0 = pl.p.starts[t];
    return IndexedFrame{pl.p.frame(pl.p.counts[t], s0), pl.mask ? ws.idx[c] + s0 : ws.ident, ws.count[(long long)t * ws.C + c]};
}

// packed upper triangle of a symmetric n x n, n at run time: pk<N> and unpk<N> of dcx_mat_dev.h
__device__ __forceinline__ int pkn(int n, int i, int j) { return i * n - i * (i - 1) / 2 + (j - i); }   // i <= j

__device__ __forceinline__ void unpkn(int n, int e, int& a, int& b) {
    int r = 0, first = 0;
    while (first + (n - r) <= e) { first += n - r; ++r; }
    a = r;
    b = r + (e - first);
}

// ---------------------------------------------------------------------------------------------------------------- init

// CAMS, here and in evaluate and trial: RigCams or MixedCams
template <class CAMS>
__global__ __launch_bounds__(kLanes) void rig_init_views_kernel(CAMS cams, int32_t* __restrict__ status, double* __restrict__ view_info,
                                                                Ws ws) {
    const int t = blockIdx.x, c = blockIdx.y, lane = threadIdx.x;
    double out[8];
    int kept;
    const int st = view_solve(cams.pl[c], cams.cam[c], t, ws.idx[c], ws.ident, out, kept);
    if (lane == 0) {
        const long long v = (long long)t * ws.C + c;
        status[v] = st;
        view_info[2 * v] = 0.0;
        view_info[2 * v + 1] = (double)kept;
        ws.count[v] = kept;
#pragma unroll
        for (int i = 0; i < 6; ++i) ws.vpose[6 * v + i] = st == DCX_PNP_OK ? out[i] : 0.0;
    }
}

__global__ __launch_bounds__(kLanes) void rig_stamps_kernel(int batch, const int32_t* __restrict__ status, double* __restrict__ pose,
                                                            Ws ws) {
    const int t = blockIdx.x * kLanes + threadIdx.x;
    if (t >= batch) return;
    int seen = 0, rows = 0;
    for (int c = 0; c < ws.C; ++c) {
        if (!usable(status, ws, t, c)) continue;
        ++seen;
        rows += ws.count[(long long)t * ws.C + c];
    }
    ws.used[t] = seen >= 2 ? 1 : 0;
    ws.rows[t] = seen >= 2 ? rows : 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) pose[8 * (long long)t + i] = 0.0;
}

// grid (64 timestamps, camera c - 1): R_t, T_t of the tree edge parent(c) -> c where both views are usable, zeros elsewhere
__global__ __launch_bounds__(kLanes) void rig_edges_kernel(int batch, const int32_t* __restrict__ status, Tree tree, Ws ws) {
    const int t = blockIdx.x * kLanes + threadIdx.x, c = blockIdx.y + 1;
    if (t >= batch) return;
    const int a = tree.parent[c];
    double e[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) e[i] = 0.0;
    if (usable(status, ws, t, a) && usable(status, ws, t, c)) {
        double pa[6], pc[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            pa[i] = ws.vpose[6 * ((long long)t * ws.C + a) + i];
            pc[i] = ws.vpose[6 * ((long long)t * ws.C + c) + i];
        }
        relative_pose(pa, pc, e);
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) ws.edge[12 * ((long long)t * (ws.C - 1) + c - 1) + i] = e[i];
}

__device__ __forceinline__ void mat3_mul(const double* A, const double* B, double* out) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) out[a * 3 + b] = A[a * 3] * B[b] + A[a * 3 + 1] * B[3 + b] + A[a * 3 + 2] * B[6 + b];
}

// One wave: the initial rig along the tree, then every used timestamp's initial pose.
__global__ __launch_bounds__(kLanes) void rig_start_kernel(Med med, Tree tree, int stamps, double points, int batch,
                                                           const int32_t* __restrict__ status, Ws ws) {
    __shared__ double X[kMaxCams][6];    // every lane computes the same values; lane 0's are kept
    RigState* st = ws.st;
    const bool writer = threadIdx.x == 0;
    if (writer) {
        lm_reset(st);
        for (int i = 0; i < kMaxG; ++i) st->g[i] = st->g_trial[i] = st->dg[i] = 0.0;
        st->prev_cost = 0.0;
        st->result[kMaxG + 3] = (double)stamps;
        st->result[kMaxG + 4] = points;
        st->code = kFinished;
#pragma unroll
        for (int i = 0; i < 6; ++i) X[0][i] = 0.0;
    }
    __syncthreads();
    for (int k = 1; k < ws.C; ++k) {
        const int c = tree.order[k], a = tree.parent[c];
        double Q[9], x[6];
        int bad = 0;
        if (!polar_factor(med.v[c - 1], Q)) {
            bad = DCX_RIG_DEGENERATE;
        } else {
            rvec_of(Q, x);
            bool finite = true;
#pragma unroll
            for (int i = 0; i < 3; ++i) x[3 + i] = med.v[c - 1][9 + i];
#pragma unroll
            for (int i = 0; i < 6; ++i) finite &= isfinite(x[i]);
            if (finite && a != 0) {
                // X_c = Z o X_a
                double xa[6], RZ[9], RA[9], Rc[9], z[6];
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    xa[i] = X[a][i];
                    z[i] = x[i];
                }
                rodrigues(z, RZ);
                rodrigues(xa, RA);
                mat3_mul(RZ, RA, Rc);
                rvec_of(Rc, x);
#pragma unroll
                for (int i = 0; i < 3; ++i) x[3 + i] = RZ[i * 3] * xa[3] + RZ[i * 3 + 1] * xa[4] + RZ[i * 3 + 2] * xa[5] + z[3 + i];
#pragma unroll
                for (int i = 0; i < 6; ++i) finite &= isfinite(x[i]);
            }
            if (!finite) bad = DCX_RIG_NONFINITE;
        }
        if (bad) {
            if (writer) st->result[kMaxG + 5] = bad;
            return;
        }
        __syncthreads();
        if (writer) {
#pragma unroll
            for (int i = 0; i < 6; ++i) X[c][i] = x[i];
        }
        __syncthreads();
    }
    for (int t = threadIdx.x; t < batch; t += kLanes) {
        if (!ws.used[t]) continue;
        int c = 0;
        while (!usable(status, ws, t, c)) ++c;       // (a used timestamp has two usable views)
        double p[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) p[i] = ws.vpose[6 * ((long long)t * ws.C + c) + i];
        if (c != 0) {
            // P_t = X_c^-1 o pose
            double xc[6], Rc[9], Rp[9], Rt[9], R[9];
#pragma unroll
            for (int i = 0; i < 6; ++i) xc[i] = X[c][i];
            rodrigues(xc, Rc);
            rodrigues(p, Rp);
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) Rt[i * 3 + j] = Rc[j * 3 + i];
            mat3_mul(Rt, Rp, R);
            const double d[3] = {p[3] - xc[3], p[4] - xc[4], p[5] - xc[5]};
            rvec_of(R, p);
#pragma unroll
            for (int i = 0; i < 3; ++i) p[3 + i] = Rt[i * 3] * d[0] + Rt[i * 3 + 1] * d[1] + Rt[i * 3 + 2] * d[2];
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) ws.pose[(long long)t * 6 + i] = p[i];
    }
    if (writer) {
        for (int c = 1; c < ws.C; ++c)
#pragma unroll
            for (int i = 0; i < 6; ++i) st->g[6 * (c - 1) + i] = X[c][i];
        st->code = kNextEvaluate;
    }
}

// ---------------------------------------------------------------------------------------------------------------- LM

// X_c from the state (g or g_trial); camera 0: zeros (the identity, not used by its rows)
__device__ __forceinline__ void camera_x(const double* g, int c, double* x) {
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] = c ? g[6 * (c - 1) + i] : 0.0;
}

template <class CAMS>
__global__ __launch_bounds__(kLanes) void rig_evaluate_kernel(CAMS cams, const int32_t* __restrict__ status, Ws ws) {
    __shared__ double sj[2 * kLanes][kLdsStride];
    const int t = blockIdx.x, c = blockIdx.y, lane = threadIdx.x;
    if (ws.st->code != kNextEvaluate || !ws.used[t] || !usable(status, ws, t, c)) return;
    double x[6], p[6];
    camera_x(ws.st->g, c, x);
#pragma unroll
    for (int i = 0; i < 6; ++i) p[i] = ws.pose[(long long)t * 6 + i];
    PairBasis B;
    pair_basis<true>(x, p, B);
    int ea[2], eb[2];
    lane_entries<13, 2>(lane, ea, eb);
    double acc[2] = {0, 0};
    bool behind = false;
    const IndexedFrame f = view_frame(cams.pl[c], ws, t, c);
    if (c) accumulate_view<true>(f, cams.cam[c], B, sj, ea, eb, acc, behind);
    else accumulate_view<false>(f, cams.cam[c], B, sj, ea, eb, acc, behind);
    const bool inf = __any(behind);
    double* m = ws.m + ((long long)t * ws.C + c) * kEntries;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int e = lane + kLanes * q;
        if (e < kEntries) m[e] = (e == kCost && inf) ? INFINITY : acc[q];
    }
}

__global__ __launch_bounds__(kLanes) void rig_schur_kernel(const int32_t* __restrict__ status, Ws ws) {
    __shared__ double sw[kMaxG][6];          // W_t: row 6 (c - 1) + j = row j of W_t,c (zero for a camera that is not there)
    __shared__ double sy[kMaxG + 1][6];      // Y's n columns, then z
    const int t = blockIdx.x, lane = threadIdx.x;
    if (ws.st->code == kFinished || !ws.used[t]) return;
    const int C = ws.C, n = ws.n, ns = ws.ns;
    const double scale = lm_damping(ws.st->lg);
    double* sc = ws.sc + (long long)t * (ns + n);
    // U_t and g_b,t over the usable cameras, ascending; every lane factors U* itself
    double u[21], gb[6], L[21];
#pragma unroll
    for (int i = 0; i < 21; ++i) u[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) gb[i] = 0.0;
    for (int c = 0; c < C; ++c) {
        if (!usable(status, ws, t, c)) continue;
        const double* m = ws.m + ((long long)t * C + c) * kEntries;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int j = i; j < 6; ++j) u[pk<6>(i, j)] += m[pk<13>(6 + i, 6 + j)];
            gb[i] += m[pk<13>(6 + i, 12)];
        }
    }
    if (!cholesky_factor<6>(u, scale, L)) {
        for (int e = lane; e < ns + n; e += kLanes) sc[e] = 0.0;
        if (lane == 0) ws.fail[t] = 1;
        return;
    }
    if (lane <= n) {
        double rhs[6], x[6];
        if (lane < n) {
            const int c = 1 + lane / 6, j = lane % 6;
            const bool in = usable(status, ws, t, c);
            const double* m = ws.m + ((long long)t * C + c) * kEntries;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                rhs[k] = in ? m[pk<13>(j, 6 + k)] : 0.0;
                sw[lane][k] = rhs[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 6; ++k) rhs[k] = gb[k];
        }
        cholesky_substitute<6>(L, rhs, x);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            sy[lane][k] = x[k];
            if (lane < n) ws.y[((long long)t * (C - 1) + lane / 6) * 36 + k * 6 + lane % 6] = x[k];
            else ws.z[(long long)t * 6 + k] = x[k];
        }
    }
    __syncthreads();
    for (int e = lane; e < ns + n; e += kLanes) {
        int a = e - ns, b = n;
        if (e < ns) unpkn(n, e, a, b);
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) s += sw[a][k] * sy[b][k];
        sc[e] = s;
    }
    if (lane == 0) ws.fail[t] = 0;
}

// First fan-in: block g sums every entry over its kChunk timestamps, one thread per entry, in timestamp order.
__global__ __launch_bounds__(kReduceThreads) void rig_reduce_kernel(int batch, const int32_t* __restrict__ status, Ws ws) {
    if (ws.st->code == kFinished) return;
    const int g = blockIdx.x, C = ws.C, n = ws.n, nv = 21 * (C - 1);
    const int end = min(batch, (g + 1) * kChunk);
    for (int e = threadIdx.x; e < ws.tot; e += kReduceThreads) {
        // where entry e lives: a camera's V block or g_a in its view's 91 (m), or the timestamp's Schur part (sc)
        int cam = 0, src;
        if (e < nv) {
            int a, b;
            unpk<6>(e % 21, a, b);
            cam = 1 + e / 21;
            src = pk<13>(a, b);
        } else if (e < nv + n) {
            cam = 1 + (e - nv) / 6;
            src = pk<13>((e - nv) % 6, 12);
        } else {
            src = e - (nv + n);
        }
        double s = 0.0;
        for (int t = g * kChunk; t < end; ++t) {
            if (!ws.used[t]) continue;
            if (cam) {
                if (usable(status, ws, t, cam)) s += ws.m[((long long)t * C + cam) * kEntries + src];
            } else {
                s += ws.sc[(long long)t * (ws.ns + n) + src];
            }
        }
        ws.part[(long long)g * ws.tot + e] = s;
    }
    if (threadIdx.x == 0) {
        int f = 0;
        for (int t = g * kChunk; t < end; ++t)
            if (ws.used[t]) f |= ws.fail[t];
        ws.pfail[g] = f;
    }
}

// Second fan-in and the solve: slice sl sums the blocks sl, sl + kSlices, ... in order, the slices meet in a fixed tree, 64 entries
// at a time; then the damped n x n system by Cholesky on LDS, the whole workgroup.
__global__ __launch_bounds__(kSlices * kLanes) void rig_reduce_solve_kernel(int chunks, Ws ws) {
    __shared__ double part[kSlices][kLanes];
    __shared__ double tot[kMaxTot];
    __shared__ double A[kMaxG][kMaxG + 1];   // the lower triangle: S, then L in place
    __shared__ double rhs[kMaxG];            // the right-hand side, then y, then x in place
    __shared__ int bad[kSlices];
    __shared__ int notpd;
    RigState* st = ws.st;
    if (st->code == kFinished) return;
    const int t = threadIdx.x, el = t % kLanes, sl = t / kLanes;
    const int C = ws.C, n = ws.n, ns = ws.ns, nv = 21 * (C - 1);
    if (el == 0) {
        int f = 0;
        for (int g = sl; g < chunks; g += kSlices) f |= ws.pfail[g];
        bad[sl] = f;
    }
    if (t == 0) notpd = 0;
    for (int base = 0; base < ws.tot; base += kLanes) {
        const int e = base + el;
        double s = 0.0;
        if (e < ws.tot)
            for (int g = sl; g < chunks; g += kSlices) s += ws.part[(long long)g * ws.tot + e];
        part[sl][el] = s;
        for (int h = kSlices / 2; h >= 1; h >>= 1) {
            __syncthreads();
            if (sl < h) part[sl][el] += part[sl + h][el];
        }
        if (sl == 0 && e < ws.tot) tot[e] = part[0][el];
        __syncthreads();                     // part is free again; tot is seen
    }
    int anybad = 0;
    for (int k = 0; k < kSlices; ++k) anybad |= bad[k];
    if (anybad) {
        if (t == 0) lm_fail(st, DCX_RIG_DEGENERATE);
        return;
    }
    const double scale = lm_damping(st->lg);
    for (int e = t; e < ns; e += kSlices * kLanes) {
        int a, b;
        unpkn(n, e, a, b);                   // a <= b
        const double v = a / 6 == b / 6 ? tot[21 * (a / 6) + pk<6>(a % 6, b % 6)] : 0.0;
        A[b][a] = v * (a == b ? scale : 1.0) - tot[nv + n + e];
    }
    if (t < n) rhs[t] = tot[nv + t] - tot[nv + n + ns + t];
    __syncthreads();
    // right-looking Cholesky: column j is finished, then taken off every later entry by that entry's own thread
    for (int j = 0; j < n; ++j) {
        if (t == 0) {
            const double d = A[j][j];
            if (!(d > 0)) notpd = 1;
            A[j][j] = sqrt(d);
        }
        __syncthreads();
        if (notpd) break;
        if (t > j && t < n) A[t][j] = A[t][j] / A[j][j];
        __syncthreads();
        const int rem = n - 1 - j;           // rows / columns j + 1 .. n - 1
        for (int q = t; q < rem * (rem + 1) / 2; q += kSlices * kLanes) {
            int a, b;
            unpkn(rem, q, a, b);             // a <= b
            A[j + 1 + b][j + 1 + a] -= A[j + 1 + b][j] * A[j + 1 + a][j];
        }
        __syncthreads();
    }
    if (notpd) {
        if (t == 0) lm_fail(st, DCX_RIG_DEGENERATE);
        return;
    }
    for (int j = 0; j < n; ++j) {            // L y = rhs
        if (t == 0) rhs[j] = rhs[j] / A[j][j];
        __syncthreads();
        if (t > j && t < n) rhs[t] -= A[t][j] * rhs[j];
        __syncthreads();
    }
    for (int j = n - 1; j >= 0; --j) {       // L^T x = y
        if (t == 0) rhs[j] = rhs[j] / A[j][j];
        __syncthreads();
        if (t < j) rhs[t] -= A[j][t] * rhs[j];
        __syncthreads();
    }
    if (t < n) {
        st->dg[t] = rhs[t];
        st->g_trial[t] = st->g[t] - rhs[t];
    }
}

template <class CAMS>
__global__ __launch_bounds__(kLanes) void rig_trial_kernel(CAMS cams, const int32_t* __restrict__ status, Ws ws) {
    const int t = blockIdx.x, c = blockIdx.y, lane = threadIdx.x;
    if (ws.st->code == kFinished || !ws.used[t]) return;
    const int C = ws.C;
    // the timestamp's trial pose p = pose - (z - sum_c Y_c dX_c), the same in every block of the timestamp
    double p[6], dn = 0.0, pn = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double s = ws.z[(long long)t * 6 + k];
        for (int cc = 1; cc < C; ++cc) {         // (a camera that is not there: schur left Y_c = 0, which takes off exact zeros)
            const double* y = ws.y + ((long long)t * (C - 1) + cc - 1) * 36 + k * 6;
#pragma unroll
            for (int j = 0; j < 6; ++j) s -= y[j] * ws.st->dg[6 * (cc - 1) + j];
        }
        const double p0 = ws.pose[(long long)t * 6 + k];
        p[k] = p0 - s;
        dn += (p[k] - p0) * (p[k] - p0);
        pn += p0 * p0;
    }
    double cost = 0.0;
    if (usable(status, ws, t, c)) {
        double x[6];
        camera_x(ws.st->g_trial, c, x);
        PairBasis B;
        pair_basis<false>(x, p, B);
        const IndexedFrame f = view_frame(cams.pl[c], ws, t, c);
        cost = c ? view_cost<true>(f, cams.cam[c], B) : view_cost<false>(f, cams.cam[c], B);
    }
    if (lane == 0) {
        double* tr = ws.trial + (long long)t * (C + 2);
        tr[c] = cost;
        if (c == 0) {
#pragma unroll
            for (int k = 0; k < 6; ++k) ws.trial_pose[(long long)t * 6 + k] = p[k];
            tr[C] = dn;
            tr[C + 1] = pn;
        }
    }
}

// init = 1: after the first evaluate (the initial cost); init = 0: after a trial
__global__ __launch_bounds__(kRedThreads) void rig_decide_kernel(int batch, int init, const int32_t* __restrict__ status,
                                                                 double* __restrict__ pose, double* __restrict__ view_info, Ws ws) {
    const int C = ws.C;
    lm_decide_block<kMaxG, true>(
        ws.st, batch, init, ws.pose, ws.trial_pose, [&](int b) { return ws.used[b] != 0; },
        [&](int b) {
            double s = 0.0;
            for (int c = 0; c < C; ++c)
                if (usable(status, ws, b, c)) s += ws.m[((long long)b * C + c) * kEntries + kCost];
            return s;
        },
        [&](int b, double* a) {
            const double* tr = ws.trial + (long long)b * (C + 2);
            double s = 0.0;
            for (int c = 0; c < C; ++c) s += tr[c];      // (trial wrote an exact zero for a camera that is not there)
            a[0] += s; a[1] += tr[C]; a[2] += tr[C + 1];
        },
        [&](int b) { return (double)ws.rows[b]; },
        [&](int b) {
            double* o = pose + 8 * (long long)b;
            const double* tr = ws.trial + (long long)b * (C + 2);
            double s = 0.0, rows = 0.0;
            for (int c = 0; c < C; ++c) {
                if (!usable(status, ws, b, c)) continue;
                const double nc = (double)ws.count[(long long)b * C + c];
                s += tr[c];
                rows += nc;
                view_info[2 * ((long long)b * C + c)] = sqrt(tr[c] / nc);
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) o[k] = ws.trial_pose[(long long)b * 6 + k];
            o[6] = sqrt(s / rows);
            o[7] = rows;
        });
}

// Everything after the camera table is made: the entry points' common body.
template <class CAMS>
int rig_calibrate(const CAMS& cams, const int* pools, int C, int batch, void* d_workspace, size_t workspace_bytes,
                  int32_t* d_view_status, double* d_pose, double* d_view_info, int32_t* h_parents, double* h_result, void* stream) {
    const int n = 6 * (C - 1);
    if (!d_workspace || !d_view_status || !d_pose || !d_view_info || !h_parents || !h_result || ((uintptr_t)d_workspace & 7))
        return DCX_E_ARG;
    if (workspace_bytes < ws_layout(nullptr, C, batch, pools, nullptr)) return DCX_E_WS;
    Ws ws;
    ws_layout(d_workspace, C, batch, pools, &ws);
    hipStream_t s = (hipStream_t)stream;
    const int chunks = chunks_of(batch);
    const dim3 stamps((unsigned)batch), views((unsigned)batch, (unsigned)C), wave(kLanes), one(1), red(kRedThreads);
    const dim3 blocks((unsigned)chunks), per_lane((unsigned)((batch + kLanes - 1) / kLanes)), solve_threads(kSlices * kLanes);
    const dim3 edges((unsigned)((batch + kLanes - 1) / kLanes), (unsigned)(C - 1));

    DCX_CHECK_HIP(hipMemsetAsync(ws.head, 0, kHeadWords * sizeof(int32_t), s));
    int n_ident = 0;
    for (int c = 0; c < C; ++c) {
        if (cams.pl[c].mask) hipLaunchKernelGGL(stereo_overlap_kernel, stamps, wave, 0, s, cams.pl[c].p, batch, ws.head + kOverlap);
        else if (pools[c] > n_ident) n_ident = pools[c];
    }
    if (n_ident > 0) hipLaunchKernelGGL(stereo_ident_kernel, dim3((unsigned)((n_ident + 255) / 256)), dim3(256), 0, s, n_ident, ws.ident);
    hipLaunchKernelGGL(rig_init_views_kernel<CAMS>, views, wave, 0, s, cams, d_view_status, d_view_info, ws);
    hipLaunchKernelGGL(rig_stamps_kernel, per_lane, wave, 0, s, batch, d_view_status, d_pose, ws);
    DCX_CHECK_HIP(hipGetLastError());

    // the tree, on the host: one copy of the statuses and the row counts (and the overlap word)
    const size_t nviews = (size_t)batch * C;
    std::vector<int32_t> status(nviews), count(nviews);
    int32_t head[kHeadWords] = {0, 0};
    DCX_CHECK_HIP(hipMemcpyAsync(status.data(), d_view_status, nviews * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    DCX_CHECK_HIP(hipMemcpyAsync(count.data(), ws.count, nviews * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    DCX_CHECK_HIP(hipMemcpyAsync(head, ws.head, sizeof(head), hipMemcpyDeviceToHost, s));
    DCX_CHECK_HIP(hipStreamSynchronize(s));
    if (head[kOverlap]) return DCX_E_ARG;    // two views of a masked pool share slots
    auto ok = [&](int t, int c) { return status[(size_t)t * C + c] == DCX_PNP_OK; };
    bool share[kMaxCams][kMaxCams] = {};
    int n_stamps = 0;
    long long points = 0;
    for (int t = 0; t < batch; ++t) {
        int seen = 0;
        for (int c = 0; c < C; ++c) seen += ok(t, c) ? 1 : 0;
        if (seen < 2) continue;
        ++n_stamps;
        for (int a = 0; a < C; ++a) {
            if (!ok(t, a)) continue;
            points += count[(size_t)t * C + a];
            for (int c = 0; c < C; ++c) share[a][c] |= ok(t, c);
        }
    }
    Tree tree;
    bool placed[kMaxCams] = {true};
    int n_placed = 1;
    for (int c = 0; c < kMaxCams; ++c) tree.parent[c] = -1, tree.order[c] = 0;
    if (n_stamps > 0) {
        for (int i = 0; i < n_placed; ++i) {
            const int a = tree.order[i];
            for (int c = 0; c < C; ++c) {
                if (placed[c] || !share[a][c]) continue;
                tree.parent[c] = a;
                placed[c] = true;
                tree.order[n_placed++] = c;
            }
        }
    }
    for (int c = 0; c < C; ++c) h_parents[c] = tree.parent[c];
    for (int i = 0; i < 8 + n; ++i) h_result[i] = 0.0;
    h_result[3] = (double)n_stamps;
    h_result[4] = (double)points;
    if (n_stamps == 0 || n_placed < C) {
        h_result[5] = n_stamps == 0 ? DCX_RIG_NO_STAMPS : DCX_RIG_DISCONNECTED;
        return 0;
    }

    // the edges' medians, on the host: one copy of the tree edges' R_t, T_t
    hipLaunchKernelGGL(rig_edges_kernel, edges, wave, 0, s, batch, d_view_status, tree, ws);
    DCX_CHECK_HIP(hipGetLastError());
    std::vector<double> edge((size_t)batch * (C - 1) * 12);
    DCX_CHECK_HIP(hipMemcpyAsync(edge.data(), ws.edge, edge.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    DCX_CHECK_HIP(hipStreamSynchronize(s));
    Med med{};
    {
        std::vector<double> col;
        col.reserve((size_t)batch);
        for (int c = 1; c < C; ++c) {
            const int a = tree.parent[c];
            for (int e = 0; e < 12; ++e) {
                col.clear();
                for (int t = 0; t < batch; ++t)
                    if (ok(t, a) && ok(t, c)) col.push_back(edge[((size_t)t * (C - 1) + c - 1) * 12 + e]);
                const size_t mid = (col.size() - 1) / 2;         // (the edge exists: its cameras share a timestamp)
                std::nth_element(col.begin(), col.begin() + mid, col.end());
                med.v[c - 1][e] = col[mid];
            }
        }
    }
    hipLaunchKernelGGL(rig_start_kernel, one, wave, 0, s, med, tree, n_stamps, (double)points, batch, d_view_status, ws);
    hipLaunchKernelGGL(rig_evaluate_kernel<CAMS>, views, wave, 0, s, cams, d_view_status, ws);
    hipLaunchKernelGGL(rig_decide_kernel, one, red, 0, s, batch, 1, d_view_status, d_pose, d_view_info, ws);
    DCX_CHECK_HIP(hipGetLastError());
    DCX_CHECK_HIP(lm_run(s, &ws.st->code, kJointMaxIter, [&](bool evaluate) {
        if (evaluate) hipLaunchKernelGGL(rig_evaluate_kernel<CAMS>, views, wave, 0, s, cams, d_view_status, ws);
        hipLaunchKernelGGL(rig_schur_kernel, stamps, wave, 0, s, d_view_status, ws);
        hipLaunchKernelGGL(rig_reduce_kernel, blocks, dim3(kReduceThreads), 0, s, batch, d_view_status, ws);
        hipLaunchKernelGGL(rig_reduce_solve_kernel, one, solve_threads, 0, s, chunks, ws);
        hipLaunchKernelGGL(rig_trial_kernel<CAMS>, views, wave, 0, s, cams, d_view_status, ws);
        hipLaunchKernelGGL(rig_decide_kernel, one, red, 0, s, batch, 0, d_view_status, d_pose, d_view_info, ws);
    }));
    double res[kResWords];
    DCX_CHECK_HIP(hipMemcpyAsync(res, ws.st->result, sizeof(res), hipMemcpyDeviceToHost, s));
    DCX_CHECK_HIP(hipStreamSynchronize(s));
    h_result[0] = res[kMaxG];                // rms
    h_result[1] = res[kMaxG + 1];            // accepted steps
    h_result[2] = res[kMaxG + 2];            // attempts
    h_result[3] = res[kMaxG + 3];
    h_result[4] = res[kMaxG + 4];
    h_result[5] = res[kMaxG + 5];
    for (int i = 0; i < n; ++i) h_result[8 + i] = res[i];
    return 0;
}

}  // namespace

extern "C" size_t dcx_rig_calibrate_workspace_bytes(int n_cams, int batch, const int* h_pools) {
    if (!sizes_ok(n_cams, batch, h_pools)) return 0;
    return ws_layout(nullptr, n_cams, batch, h_pools, nullptr);
}

extern "C" int dcx_rig_calibrate_pool(int n_cams, const DcxRigCamera* h_cams, int batch, int col_count, int row_count,
                                      double square_len, void* d_workspace, size_t workspace_bytes, int32_t* d_view_status,
                                      double* d_pose, double* d_view_info, int32_t* h_parents, double* h_result, void* stream) {
    RigCams cams{};
    int pools[kMaxCams];
    if (!camera_table(n_cams, h_cams, batch, col_count, row_count, square_len, cams, pools,
                      [](int, const DcxRigCamera& h, PnpCamera& cam) { return pnp_camera(h.camera9, h.dist, h.n_dist, cam); }))
        return DCX_E_ARG;
    return rig_calibrate(cams, pools, n_cams, batch, d_workspace, workspace_bytes, d_view_status, d_pose, d_view_info, h_parents,
                         h_result, stream);
}

// h_models NULL or all DCX_CAMERA_PINHOLE: dcx_rig_calibrate_pool, the same kernels on the same table.
extern "C" int dcx_rig_calibrate_models_pool(int n_cams, const DcxRigCamera* h_cams, const int* h_models, int batch, int col_count,
                                             int row_count, double square_len, void* d_workspace, size_t workspace_bytes,
                                             int32_t* d_view_status, double* d_pose, double* d_view_info, int32_t* h_parents,
                                             double* h_result, void* stream) {
    bool mixed = false;
    if (h_models && n_cams >= 2 && n_cams <= kMaxCams)
        for (int c = 0; c < n_cams; ++c) {
            if (h_models[c] != DCX_CAMERA_PINHOLE && h_models[c] != DCX_CAMERA_FISHEYE) return DCX_E_ARG;
            mixed |= h_models[c] == DCX_CAMERA_FISHEYE;
        }
    if (!mixed)
        return dcx_rig_calibrate_pool(n_cams, h_cams, batch, col_count, row_count, square_len, d_workspace, workspace_bytes,
                                      d_view_status, d_pose, d_view_info, h_parents, h_result, stream);
    MixedCams cams{};
    int pools[kMaxCams];
    if (!camera_table(n_cams, h_cams, batch, col_count, row_count, square_len, cams, pools, [&](int c, const DcxRigCamera& h, AnyCamera& cam) {
            return any_camera(h_models[c], h.camera9, h.dist, h.n_dist, cam);
        }))
        return DCX_E_ARG;
    return rig_calibrate(cams, pools, n_cams, batch, d_workspace, workspace_bytes, d_view_status, d_pose, d_view_info, h_parents,
                         h_result, stream);
}
