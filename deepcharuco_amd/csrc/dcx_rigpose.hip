// dcx_rigpose.hip -- the board's pose from every camera of a calibrated rig of C = 2 .. 8 cameras, on the device, read straight from
// the C corner pools dcx_infer_batch writes: with X_c = (R_c, T_c), q_c = R_c q_0 + T_c, held fixed, the pose P_t in camera 0's frame
// per timestamp, over every row any camera saw then.  Every timestamp is solved on its own.  The steps (all fp64) are restated
// readably in deepcharuco_amd/rig.py (rig_pose_host_full), which is the pin of these kernels:
//   per-view checks and poses as in dcx_rig.hip -> a view's rows CONTRIBUTE if it is not TRUNCATED, has a kept row, every kept id is
//   on the board and (fisheye) every kept pixel is inside the model, whatever its status: a view of 1 .. 3 rows or of collinear rows
//   contributes -> every OK view is a seed, P = X_c^-1 o pose_{c,t}, scored by the joint cost over every contributing row; the lowest
//   score starts, the lowest camera among equals -> the PnP Levenberg-Marquardt (dcx_pnp_dev.h's solve, unchanged: FLT_EPSILON, 20
//   accepted steps, cost <= prev_cost) over P_t's 6 parameters on that joint cost.
//
// Launches (one 64-lane wave per unit):
//   overlap, ident  dcx_stereo_dev.h's, per pool with / without a mask; the overlap word lives in the workspace
//   views           grid (timestamp, camera): dcx_stereo_dev.h's view_solve (the mask compacted into the view's index list, the
//                   view's own pose to vpose), and beside it the view's "contributes" flag: the id check and the inside check over
//                   the kept rows, which view_solve skips where it answers TOO_FEW first.  With the overlap word set nothing is
//                   read: every view is written TRUNCATED
//   solve           per timestamp: the seeds scored, cameras ascending; then solve() of dcx_pnp_dev.h on a JointFrame, whose
//                   evaluate walks the contributing views, cameras ascending, the lanes striding over each view's rows through its
//                   IndexedFrame; each lane adds up {cost, JtJ (21), Jtr (6)} from stereo_row<JAC, SECOND>'s P columns, one wave_sum
//                   butterfly at the end, and every lane runs the 6 x 6 Cholesky itself, as solve() has it; then the views' rms at
//                   the solution.  With the overlap word set: TRUNCATED and zeros for every timestamp, and d_head[0] = 1
// views and solve are templates on the camera table (dcx_stereo_dev.h): RigCams, or MixedCams for a rig with a fisheye camera in
// it.  The kernels' text knows no model: on a table of AnyCamera the model is chosen per view, inside the step.
// solve() itself is not restated: JointFrame and JointCamera are a frame and a camera class of its template, with their own
// points_inside, has_distortion, init_pose (the chosen seed) and evaluate below.
// No LDS but view_solve's own, no atomics, no barrier beyond view_solve's; every sum has a fixed order: two calls on the same input
// give the same bits.  Nothing is read on the host: the call does not synchronise, allocates nothing and can be captured in a graph.
#include "dcx_stereo_dev.h"

namespace {

enum : int { kOverlap = 0, kHeadWords = 2 };

struct RigX {
    double x[kMaxCams][6];               // X_c = (rvec, T); x[0] = 0: camera 0 is the reference
};

struct Ws {
    double* vpose;                       // [B][C][6] a view's own pose (zero unless it is OK)
    int32_t *head, *count, *contrib, *ident;   // head [2]; count, contrib [B][C]: the view's kept rows, whether they contribute
    int32_t* idx[kMaxCams];
    int C;
};

// the whole argument block of a kernel: the camera table, the rig, the workspace, the output pointers and scalars
static_assert(sizeof(MixedCams) + sizeof(RigX) + sizeof(Ws) + 128 <= 4096, "kernel arguments");

size_t ws_layout(void* base, int C, int batch, const int* pools, Ws* w) {
    const size_t B = (size_t)batch;
    Carver c{(char*)base, 0};
    Ws r;
    r.C = C;
    r.vpose = c.take<double>(B * C * 6);
    r.head = c.take<int32_t>(kHeadWords);
    r.count = c.take<int32_t>(B * C);
    r.contrib = c.take<int32_t>(B * C);
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

// View (t, c) as the solve reads it: its kept rows through the index list view_solve left.
__device__ __forceinline__ IndexedFrame view_frame(const MaskedPool& pl, const Ws& ws, int t, int c) {
    const long long s0 = pl.p.starts[t];
    return IndexedFrame{pl.p.frame(pl.p.counts[t], s0), pl.mask ? ws.idx[c] + s0 : ws.ident, ws.count[(long long)t * ws.C + c]};
}

// ---------------------------------------------------------------------------------------------------------------- views

// Do the kept rows of a view that is not TRUNCATED contribute?  The checks view_solve makes only on a view of four rows or more,
// made on every view: a kept row, every kept id on the board, every kept pixel inside the camera's model.  Wave-wide.
template <class CAM>
__device__ __forceinline__ bool view_contributes(const IndexedFrame& f, const CornerPool& pl, const CAM& cam) {
    if (f.n < 1) return false;
    bool bad = false;
    for (int i = threadIdx.x; i < f.n; i += kLanes) {
        const int id = f.base.rows[4 * f.idx[i] + 2];
        bad |= id < 0 || id >= pl.n_ids;
    }
    if (__any(bad)) return false;
    return points_inside(f, cam);
}

__device__ __forceinline__ bool view_contributes(const IndexedFrame& f, const CornerPool& pl, const AnyCamera& cam) {
    return with_camera(cam, [&](const auto& k) { return view_contributes(f, pl, k); });
}

// CAMS, here and in solve: RigCams or MixedCams
template <class CAMS>
__global__ __launch_bounds__(kLanes) void rig_pose_views_kernel(CAMS cams, int32_t* __restrict__ status, double* __restrict__ view_info,
                                                                Ws ws) {
    const int t = blockIdx.x, c = blockIdx.y, lane = threadIdx.x;
    const long long v = (long long)t * ws.C + c;
    double out[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = 0.0;
    int kept = 0, st = DCX_PNP_TRUNCATED;
    bool in = false;
    if (!ws.head[kOverlap]) {                // (uniform; with the word set no list is written and none is read)
        st = view_solve(cams.pl[c], cams.cam[c], t, ws.idx[c], ws.ident, out, kept);
        if (st != DCX_PNP_TRUNCATED && kept > 0) {
            const long long s0 = cams.pl[c].p.starts[t];
            const IndexedFrame f{cams.pl[c].p.frame(cams.pl[c].p.counts[t], s0), cams.pl[c].mask ? ws.idx[c] + s0 : ws.ident, kept};
            in = view_contributes(f, cams.pl[c].p, cams.cam[c]);
        }
    }
    if (lane == 0) {
        status[v] = st;
        view_info[2 * v] = 0.0;
        view_info[2 * v + 1] = (double)kept;
        ws.count[v] = kept;
        ws.contrib[v] = in ? 1 : 0;
#pragma unroll
        for (int i = 0; i < 6; ++i) ws.vpose[6 * v + i] = st == DCX_PNP_OK ? out[i] : 0.0;
    }
}

// ---------------------------------------------------------------------------------------------------------------- solve

// A timestamp's contributing rows of every camera as solve() of dcx_pnp_dev.h takes a frame: n is its row count, and the four
// functions below are what solve() asks of a frame and its camera.  The cameras ride inside the frame: JointCamera is a tag.
template <class CAMS>
struct JointFrame {
    const CAMS& cams;
    const RigX& rig;
    const Ws& ws;
    int t, n;
    double start[6];                     // the chosen seed: solve()'s init_pose
};

struct JointCamera {};

template <class CAMS>
__device__ __forceinline__ bool points_inside(const JointFrame<CAMS>&, const JointCamera&) { return true; }   // (views checked them)

__device__ __forceinline__ bool has_distortion(const JointCamera&) { return false; }                            // (init_pose's business)

template <class CAMS>
__device__ __forceinline__ int init_pose(const JointFrame<CAMS>& f, const JointCamera&, bool, double* p0) {
#pragma unroll
    for (int i = 0; i < 6; ++i) p0[i] = f.start[i];
    return DCX_PNP_OK;
}

// One view's rows added to this lane's {cost, JtJ, Jtr}: evaluate()'s loop of dcx_pnp_dev.h on stereo_row's P columns
template <bool JAC, bool SECOND, class CAM>
__device__ __forceinline__ void joint_view(const IndexedFrame& f, const CAM& cam, const PairBasis& B, double (&acc)[28]) {
    for (int i = threadIdx.x; i < f.n; i += kLanes) {
        double mx, my, u, v, ru, rv, ju[12], jv[12];
        f.load(i, mx, my, u, v);
        if (!stereo_row<JAC, SECOND>(cam, B, mx, my, u, v, ru, rv, JAC ? ju : nullptr, JAC ? jv : nullptr)) {
            acc[0] = INFINITY;
            continue;
        }
        acc[0] += ru * ru + rv * rv;
        if (!JAC) continue;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
#pragma unroll
            for (int b = a; b < 6; ++b) acc[1 + pk<6>(a, b)] += ju[6 + a] * ju[6 + b] + jv[6 + a] * jv[6 + b];
            acc[22 + a] += ju[6 + a] * ru + jv[6 + a] * rv;
        }
    }
}

template <bool JAC, bool SECOND>
__device__ __forceinline__ void joint_view(const IndexedFrame& f, const AnyCamera& cam, const PairBasis& B, double (&acc)[28]) {
    with_camera(cam, [&](const auto& k) { joint_view<JAC, SECOND>(f, k, B, acc); return 0; });
}

// The joint cost at pose p (+inf if a row is not in front of its camera) and, with JAC, JtJ (21, packed) and Jtr (6) over every
// contributing row: cameras ascending, the lanes striding over each view's rows, one butterfly at the end.  acc identical in every
// lane on return: evaluate()'s contract in dcx_pnp_dev.h.
template <bool JAC, class CAMS>
__device__ __forceinline__ void evaluate(const JointFrame<CAMS>& f, const JointCamera&, const double* p, double (&acc)[28]) {
#pragma unroll
    for (int i = 0; i < 28; ++i) acc[i] = 0.0;
    const int C = f.ws.C;
#pragma unroll 1
    for (int c = 0; c < C; ++c) {
        if (!f.ws.contrib[(long long)f.t * C + c]) continue;
        PairBasis B;
        pair_basis<JAC>(f.rig.x[c], p, B);
        const IndexedFrame v = view_frame(f.cams.pl[c], f.ws, f.t, c);
        if (c) joint_view<JAC, true>(v, f.cams.cam[c], B, acc);
        else joint_view<JAC, false>(v, f.cams.cam[c], B, acc);
    }
    wave_sum(acc);
}

// P = X_c^-1 o pose (rig.py's _seed_pose): p in place
__device__ __forceinline__ void seed_pose(const double* x, double* p) {
    double Rc[9], Rp[9], R[9];
    rodrigues(x, Rc);
    rodrigues(p, Rp);
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) R[a * 3 + b] = Rc[a] * Rp[b] + Rc[3 + a] * Rp[3 + b] + Rc[6 + a] * Rp[6 + b];     // R_c^T R_p
    const double d[3] = {p[3] - x[3], p[4] - x[4], p[5] - x[5]};
    rvec_of(R, p);
#pragma unroll
    for (int a = 0; a < 3; ++a) p[3 + a] = Rc[a] * d[0] + Rc[3 + a] * d[1] + Rc[6 + a] * d[2];
}

template <class CAMS>
__global__ __launch_bounds__(kLanes) void rig_pose_solve_kernel(CAMS cams, RigX rig, int32_t* __restrict__ head,
                                                                int32_t* __restrict__ status, double* __restrict__ pose,
                                                                int32_t* __restrict__ info, int32_t* __restrict__ view_status,
                                                                double* __restrict__ view_info, Ws ws) {
    const int t = blockIdx.x, lane = threadIdx.x, C = ws.C;
    const bool overlap = ws.head[kOverlap] != 0;
    if (t == 0 && lane == 0) {
        head[0] = overlap ? 1 : 0;
        head[1] = 0;
    }
    double out[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = 0.0;
    int st = DCX_PNP_TRUNCATED, seed = -1, rows = 0;
    JointFrame<CAMS> f{cams, rig, ws, t, 0, {0, 0, 0, 0, 0, 0}};
    if (!overlap) {
        for (int c = 0; c < C; ++c)
            if (ws.contrib[(long long)t * C + c]) rows += ws.count[(long long)t * C + c];
        f.n = rows;
        st = DCX_PNP_TOO_FEW;                // no view solves on its own
        double best = INFINITY;
#pragma unroll 1
        for (int c = 0; c < C; ++c) {
            if (view_status[(long long)t * C + c] != DCX_PNP_OK) continue;
            st = DCX_PNP_DEGENERATE;         // seeds, and so far none with every row in front of its camera
            double p[6], acc[28];
#pragma unroll
            for (int i = 0; i < 6; ++i) p[i] = ws.vpose[6 * ((long long)t * C + c) + i];
            if (c) seed_pose(rig.x[c], p);
            evaluate<false>(f, JointCamera{}, p, acc);
            if (acc[0] < best) {
                best = acc[0];
                seed = c;
#pragma unroll
                for (int i = 0; i < 6; ++i) f.start[i] = p[i];
            }
        }
        if (seed >= 0) st = solve(f, JointCamera{}, out);
    }
    const bool ok = st == DCX_PNP_OK;
    double p[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) p[i] = out[i];
#pragma unroll 1
    for (int c = 0; c < C; ++c) {
        const long long v = (long long)t * C + c;
        double rms = 0.0;
        if (ok && ws.contrib[v]) {
            PairBasis B;
            pair_basis<false>(rig.x[c], p, B);
            const IndexedFrame g = view_frame(cams.pl[c], ws, t, c);
            const double cost = c ? view_cost<true>(g, cams.cam[c], B) : view_cost<false>(g, cams.cam[c], B);
            rms = sqrt(cost / (double)g.n);
        }
        if (lane == 0) {
            view_info[2 * v] = rms;
            if (overlap) {
                view_status[v] = DCX_PNP_TRUNCATED;
                view_info[2 * v + 1] = 0.0;
            }
        }
    }
    if (lane == 0) {
        status[t] = st;
#pragma unroll
        for (int i = 0; i < 8; ++i) pose[8 * (long long)t + i] = ok ? out[i] : 0.0;
        info[2 * (long long)t] = seed;
        info[2 * (long long)t + 1] = rows;
    }
}

// Everything after the camera table is made: the entry point's body for either table.
template <class CAMS>
int rig_pose(const CAMS& cams, const RigX& rig, const int* pools, int C, int batch, void* d_workspace, size_t workspace_bytes,
             int32_t* d_head, int32_t* d_status, double* d_pose, int32_t* d_info, int32_t* d_view_status, double* d_view_info,
             void* stream) {
    if (!d_workspace || !d_head || !d_status || !d_pose || !d_info || !d_view_status || !d_view_info || ((uintptr_t)d_workspace & 7))
        return DCX_E_ARG;
    if (workspace_bytes < ws_layout(nullptr, C, batch, pools, nullptr)) return DCX_E_WS;
    Ws ws;
    ws_layout(d_workspace, C, batch, pools, &ws);
    hipStream_t s = (hipStream_t)stream;
    const dim3 stamps((unsigned)batch), views((unsigned)batch, (unsigned)C), wave(kLanes);
    DCX_CHECK_HIP(hipMemsetAsync(ws.head, 0, kHeadWords * sizeof(int32_t), s));
    int n_ident = 0;
    for (int c = 0; c < C; ++c) {
        if (cams.pl[c].mask) hipLaunchKernelGGL(stereo_overlap_kernel, stamps, wave, 0, s, cams.pl[c].p, batch, ws.head + kOverlap);
        else if (pools[c] > n_ident) n_ident = pools[c];
    }
    if (n_ident > 0) hipLaunchKernelGGL(stereo_ident_kernel, dim3((unsigned)((n_ident + 255) / 256)), dim3(256), 0, s, n_ident, ws.ident);
    hipLaunchKernelGGL(rig_pose_views_kernel<CAMS>, views, wave, 0, s, cams, d_view_status, d_view_info, ws);
    hipLaunchKernelGGL(rig_pose_solve_kernel<CAMS>, stamps, wave, 0, s, cams, rig, d_head, d_status, d_pose, d_info, d_view_status,
                       d_view_info, ws);
    DCX_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" size_t dcx_rig_pose_workspace_bytes(int n_cams, int batch, const int* h_pools) {
    if (!sizes_ok(n_cams, batch, h_pools)) return 0;
    return ws_layout(nullptr, n_cams, batch, h_pools, nullptr);
}

extern "C" int dcx_rig_pose_pool(int n_cams, const DcxRigCamera* h_cams, const int* h_models, const double* h_rig, int batch,
                                 int col_count, int row_count, double square_len, void* d_workspace, size_t workspace_bytes,
                                 int32_t* d_head, int32_t* d_status, double* d_pose, int32_t* d_info, int32_t* d_view_status,
                                 double* d_view_info, void* stream) {
    if (n_cams < 2 || n_cams > kMaxCams || !h_rig) return DCX_E_ARG;
    RigX rig{};
    for (int c = 1; c < n_cams; ++c)
        for (int i = 0; i < 6; ++i) {
            rig.x[c][i] = h_rig[6 * (c - 1) + i];
            if (!isfinite(rig.x[c][i])) return DCX_E_ARG;
        }
    bool mixed = false;
    if (h_models)
        for (int c = 0; c < n_cams; ++c) {
            if (h_models[c] != DCX_CAMERA_PINHOLE && h_models[c] != DCX_CAMERA_FISHEYE) return DCX_E_ARG;
            mixed |= h_models[c] == DCX_CAMERA_FISHEYE;
        }
    int pools[kMaxCams];
    if (!mixed) {
        RigCams cams{};
        if (!camera_table(n_cams, h_cams, batch, col_count, row_count, square_len, cams, pools,
                          [](int, const DcxRigCamera& h, PnpCamera& cam) { return pnp_camera(h.camera9, h.dist, h.n_dist, cam); }))
            return DCX_E_ARG;
        return rig_pose(cams, rig, pools, n_cams, batch, d_workspace, workspace_bytes, d_head, d_status, d_pose, d_info, d_view_status,
                        d_view_info, stream);
    }
    MixedCams cams{};
    if (!camera_table(n_cams, h_cams, batch, col_count, row_count, square_len, cams, pools, [&](int c, const DcxRigCamera& h, AnyCamera& cam) {
            return any_camera(h_models[c], h.camera9, h.dist, h.n_dist, cam);
        }))
        return DCX_E_ARG;
    return rig_pose(cams, rig, pools, n_cams, batch, d_workspace, workspace_bytes, d_head, d_status, d_pose, d_info, d_view_status,
                    d_view_info, stream);
}
