// dcx_pnp_ransac.hip -- the PnP solver of dcx_pnp.hip behind a consensus search (cv2.solvePnPRansac's role), read in place from the
// corner pool.  deepcharuco_amd/pnp.py restates every step (solve_pnp_ransac_host_full), which is the pin of these kernels.
//
// Two launches on the caller's stream, all fp64:
//   hypotheses  grid (frame, block of 64 hypotheses), one LANE per hypothesis: an integer counter hash of (seed, n, h, draw) picks
//               four rows with distinct ids and no collinear triple, the homography through them comes in closed form (H = B adj(A)
//               of the two projective bases: four points determine it, so the 9x9 eigenproblem of the DLT has nothing to add and its
//               81-double eigenvector matrix would not fit a lane), init_pose's decomposition turns it into a pose, and a serial loop over
//               the frame's rows (every lane reads the same row) counts those within reproj_error px.  Score (-1: no hypothesis)
//               and pose go to the workspace.
//   select      one wave per frame: first maximum of the scores in a fixed order, the winner's mask recomputed and written, its
//               slots compacted in order into an index list, then the unchanged solve() (init + LM) over that list.
// The sampler never looks at the frame's position in the batch, nothing is allocated, no atomics, no early exit: the work is fixed,
// two runs give the same bits and the call can be captured in a hipGraph.
// The pool type and its host check (CornerPool, corner_pool), frame_status, the sampler, the four-point homography, row_error2,
// best_hypothesis and solve() are dcx_pnp_dev.h's; append_kept is dcx_mat_dev.h's.
// Both kernels are templates on the camera's class.  On FisheyeCamera (dcx_fisheye_solve_pnp_ransac_pool) the sample's four pixels
// go through that model's undistort, a sample with a pixel outside the model has no hypothesis, the rows are scored by forward
// projection through the model, and solve() may answer DCX_PNP_DEGENERATE for a winner's inlier outside it.  Sampler, score order,
// mask and info are the same.
#include "dcx_fisheye_dev.h"
#include "dcx_pnp_dev.h"

extern "C" size_t dcx_solve_pnp_ransac_workspace_bytes(int batch, int pool, int iterations);

namespace {

// does every pixel of the sample undistort?  A pinhole's always does.
__device__ __forceinline__ bool sample_inside(const PnpCamera&, const Sample&) { return true; }

__device__ __forceinline__ bool sample_inside(const FisheyeCamera&, const Sample& q) {
    bool in = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) in &= isfinite(q.x[k]) && isfinite(q.y[k]);
    return in;
}

// hypothesis h of frame f in this lane -> its score, or -1 if it has none; p0 = its pose
template <class CAM>
__device__ __forceinline__ int hypothesis(const Frame& f, const CAM& cam, bool dist, uint32_t seed, int h, double thr2, double* p0) {
    int s[4];
    if (!ransac_sample(f.rows, seed, f.n, h, f.rm1, s)) return -1;
    Sample q;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double u, v;
        f.load(s[k], q.mx[k], q.my[k], u, v);
        undistort(cam, dist, u, v, q.x[k], q.y[k]);
    }
    if (!sample_inside(cam, q)) return -1;
    if (init_pose(q, cam, dist, p0) != DCX_PNP_OK) return -1;
    double R[9];
    rodrigues(p0, R);
    int score = 0;
    for (int i = 0; i < f.n; ++i) {
        double bx, by, u, v;
        f.load(i, bx, by, u, v);
        score += row_error2(R, p0 + 3, cam, bx, by, u, v) <= thr2 ? 1 : 0;
    }
    return score;
}

// Both kernels take the pool as loose __restrict__ parameters and make the CornerPool in their first line, as dcx_solve_pnp_kernel
// does and for its reason (see there).  CAM: PnpCamera or FisheyeCamera.
template <class CAM>
__global__ __launch_bounds__(kLanes) void dcx_pnp_ransac_hypotheses_kernel(
    const int32_t* __restrict__ counts, const int32_t* __restrict__ starts, const int32_t* __restrict__ rows,
    const float* __restrict__ xy, int pool, int n_ids, int rm1, double square_len, CAM cam, int iterations, double thr2,
    uint32_t seed, int32_t* __restrict__ scores, double* __restrict__ poses) {
    const int b = blockIdx.x, h = blockIdx.y * kLanes + threadIdx.x;
    const CornerPool pl{counts, starts, rows, xy, pool, n_ids, rm1, square_len};
    int n, s0;
    if (frame_status(pl, b, n, s0) != DCX_PNP_OK) return;   // select reports it and reads no score
    if (h >= iterations) return;
    const Frame f = pl.frame(n, s0);
    double p0[6] = {0, 0, 0, 0, 0, 0};
    const int score = hypothesis(f, cam, has_distortion(cam), seed, h, thr2, p0);
    const long long at = (long long)b * iterations + h;
    scores[at] = score;
#pragma unroll
    for (int i = 0; i < 6; ++i) poses[6 * at + i] = p0[i];
}

template <class CAM>
__global__ __launch_bounds__(kLanes) void dcx_pnp_ransac_select_kernel(
    const int32_t* __restrict__ counts, const int32_t* __restrict__ starts, const int32_t* __restrict__ rows,
    const float* __restrict__ xy, int pool, int n_ids, int rm1, double square_len, CAM cam, int iterations, double thr2,
    int min_inliers, const int32_t* __restrict__ scores, const double* __restrict__ poses, int32_t* idx,
    int32_t* __restrict__ status, double* __restrict__ pose, int32_t* __restrict__ info, uint8_t* __restrict__ inliers) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const CornerPool pl{counts, starts, rows, xy, pool, n_ids, rm1, square_len};
    int n, s0;
    int st = frame_status(pl, b, n, s0);
    double out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int winner = -1, count = 0;
    if (st == DCX_PNP_OK) {
        int best, bh;
        best_hypothesis(scores + (long long)b * iterations, iterations, best, bh);
        if (best < 0) {
            st = DCX_PNP_DEGENERATE;
        } else {
            winner = bh;
            const Frame f = pl.frame(n, s0);
            double p[6], R[9];
#pragma unroll
            for (int i = 0; i < 6; ++i) p[i] = poses[6 * ((long long)b * iterations + winner) + i];
            rodrigues(p, R);
            int32_t* list = idx + s0;                      // this frame's share of the index list: its own slots
            for (int base = 0; base < n; base += kLanes) {
                const int i = base + lane;
                bool in = false;
                if (i < n) {
                    double bx, by, u, v;
                    f.load(i, bx, by, u, v);
                    in = row_error2(R, p + 3, cam, bx, by, u, v) <= thr2;
                    if (inliers) inliers[(long long)s0 + i] = in ? 1 : 0;
                }
                const int at = append_kept(in, lane, count);
                if (in) list[at] = i;
            }
            __syncthreads();                               // one wave: the list is read below by other lanes than wrote it
            if (count < max(min_inliers, 4)) {
                st = DCX_PNP_NO_CONSENSUS;
            } else {
                const IndexedFrame g{f, list, count};
                st = solve(g, cam, out);
            }
        }
    }
    if (st != DCX_PNP_OK) {
#pragma unroll
        for (int i = 0; i < 8; ++i) out[i] = 0.0;
        count = 0;
        // no pose, no inliers: every slot of the frame that lies in the pool (the lane that wrote a slot above rewrites it)
        if (inliers && n > 0 && s0 >= 0)
            for (long long i = lane; i < n && s0 + i < pl.pool; i += kLanes) inliers[s0 + i] = 0;
    }
    if (lane == 0) {
        status[b] = st;
#pragma unroll
        for (int i = 0; i < 8; ++i) pose[8 * (long long)b + i] = out[i];
        info[2 * (long long)b] = count;
        info[2 * (long long)b + 1] = winner;
    }
}

// What the two entries share once their camera is made: the checks, the workspace's parts, the two launches.
template <class CAM>
int ransac_launch(const CornerPool& pl, const CAM& cam, int batch, int pool, int iterations, double reproj_error, int min_inliers,
                  unsigned seed, void* d_workspace, size_t workspace_bytes, int32_t* d_status, double* d_pose, int32_t* d_info,
                  uint8_t* d_inliers, void* stream) {
    if (iterations < 1 || iterations > kMaxIterations || !isfinite(reproj_error) || !(reproj_error > 0)) return DCX_E_ARG;
    if (workspace_bytes < dcx_solve_pnp_ransac_workspace_bytes(batch, pool, iterations) || ((uintptr_t)d_workspace & 7)) return DCX_E_ARG;
    const size_t hyp = (size_t)batch * (size_t)iterations;
    double* poses = (double*)d_workspace;
    int32_t* scores = (int32_t*)(poses + 6 * hyp);
    int32_t* idx = scores + hyp;
    const double thr2 = reproj_error * reproj_error;
    hipLaunchKernelGGL(dcx_pnp_ransac_hypotheses_kernel<CAM>, dim3((unsigned)batch, (unsigned)((iterations + kLanes - 1) / kLanes)),
                       dim3(kLanes), 0, (hipStream_t)stream, pl.counts, pl.starts, pl.rows, pl.xy, pl.pool, pl.n_ids, pl.rm1,
                       pl.square_len, cam, iterations, thr2, (uint32_t)seed, scores, poses);
    hipLaunchKernelGGL(dcx_pnp_ransac_select_kernel<CAM>, dim3((unsigned)batch), dim3(kLanes), 0, (hipStream_t)stream, pl.counts,
                       pl.starts, pl.rows, pl.xy, pl.pool, pl.n_ids, pl.rm1, pl.square_len, cam, iterations, thr2, min_inliers, scores,
                       poses, idx, d_status, d_pose, d_info, d_inliers);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int dcx_solve_pnp_ransac_pool(const int32_t* d_counts, const int32_t* d_starts, const int32_t* d_rows, const float* d_xy,
                                         int batch, int pool, int col_count, int row_count, double square_len,
                                         const double* h_camera9, const double* h_dist, int n_dist, int iterations,
                                         double reproj_error, int min_inliers, unsigned seed, void* d_workspace,
                                         size_t workspace_bytes, int32_t* d_status, double* d_pose, int32_t* d_info,
                                         uint8_t* d_inliers, void* stream) {
    CornerPool pl;
    PnpCamera cam;
    if (!corner_pool(d_counts, d_starts, d_rows, d_xy, batch, pool, col_count, row_count, square_len, pl)) return DCX_E_ARG;
    if (!h_camera9 || !d_status || !d_pose || !d_info || !d_workspace || !pnp_camera(h_camera9, h_dist, n_dist, cam)) return DCX_E_ARG;
    return ransac_launch(pl, cam, batch, pool, iterations, reproj_error, min_inliers, seed, d_workspace, workspace_bytes, d_status,
                         d_pose, d_info, d_inliers, stream);
}

extern "C" int dcx_fisheye_solve_pnp_ransac_pool(const int32_t* d_counts, const int32_t* d_starts, const int32_t* d_rows,
                                                 const float* d_xy, int batch, int pool, int col_count, int row_count,
                                                 double square_len, const double* h_camera9, const double* h_dist4, int iterations,
                                                 double reproj_error, int min_inliers, unsigned seed, void* d_workspace,
                                                 size_t workspace_bytes, int32_t* d_status, double* d_pose, int32_t* d_info,
                                                 uint8_t* d_inliers, void* stream) {
    CornerPool pl;
    FisheyeCamera cam;
    if (!corner_pool(d_counts, d_starts, d_rows, d_xy, batch, pool, col_count, row_count, square_len, pl)) return DCX_E_ARG;
    if (!d_status || !d_pose || !d_info || !d_workspace || !fisheye_camera(h_camera9, h_dist4, cam)) return DCX_E_ARG;
    // (a short workspace has its own code here, as in the entries after dcx_solve_pnp_ransac_pool, which keeps answering DCX_E_ARG)
    if (iterations >= 1 && iterations <= kMaxIterations && workspace_bytes < dcx_solve_pnp_ransac_workspace_bytes(batch, pool, iterations))
        return DCX_E_WS;
    return ransac_launch(pl, cam, batch, pool, iterations, reproj_error, min_inliers, seed, d_workspace, workspace_bytes, d_status,
                         d_pose, d_info, d_inliers, stream);
}

// workspace: poses f64 [B][iterations][6] | scores int32 [B][iterations] | inlier index list int32 [pool]
extern "C" size_t dcx_solve_pnp_ransac_workspace_bytes(int batch, int pool, int iterations) {
    if (batch <= 0 || pool < 0 || iterations < 1 || iterations > kMaxIterations) return 0;
    const size_t hyp = (size_t)batch * (size_t)iterations;
    return (hyp * (6 * sizeof(double) + sizeof(int32_t)) + (size_t)pool * sizeof(int32_t) + 7) & ~(size_t)7;
}
