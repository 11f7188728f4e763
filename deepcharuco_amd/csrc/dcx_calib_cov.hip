// dcx_calib_cov.hip -- how well a single-camera calibration is determined: the covariances of the intrinsics and of every used view's
// pose at a solved model, read from the corner pool the calibration read.  deepcharuco_amd/calib.py restates the definition
// (calibration_uncertainty_host, _lm.schur_covariance) and is the pin of these kernels.  With the undamped normal blocks of
// dcx_calib_dev.h at the solution (U_i 6x6, W_i NG x 6, V NG x NG over the used views' kept rows):
//   S = V - sum W_i U_i^-1 W_i^T,  Y_i = U_i^-1 W_i^T,  dof = 2 points - NG - 6 views,  sigma^2 = sum |r|^2 / dof,
//   cov_intrinsics = sigma^2 S^-1,  cov_pose_i = sigma^2 (U_i^-1 + Y_i S^-1 Y_i^T),  the standard deviations their diagonals' roots.
// Instantiated on PinholeCalib (NG = 9) and FisheyeCalib (NG = 8).  Four launches, all fp64, every sum in a fixed order, no atomics,
// no host loop and no synchronisation (the call can be captured in a graph); one 64-lane wave per view unless noted, grid = batch:
//   evaluate        the view's packed NC x NC entries at (theta, pose) by dcx_mat_dev.h's accumulate_rows; a row whose mask byte
//                   is 0 is a row of zeros (adding 0.0 changes no bit, so a masked pool gives the bits of the compacted one); the
//                   view's kept-row count; a flag if a kept point is not in front of the camera or the view's slots leave the pool
//   schur           schur_view at scale 1.0 -> Y_i and the view's part of S; U_i^-1 by the 6x6 Cholesky against the unit vectors
//   reduce_invert   (one workgroup) the views' parts summed in reduce_solve's order (8 slices, added serially), S, its Cholesky in
//                   LDS, S^-1 by NG substitutions, the cost, the counts, dof, sigma^2, the status; writes the global block
//   pose            cov_pose_i and its standard deviations; zeros for a view that was not used or a status other than OK
// The existing calibration kernels are not instantiated here and their text is not touched: this unit has a workspace of its own.
#include "dcx_calib_dev.h"

namespace {

constexpr int kCovHead = 64;                              // doubles: S^-1 packed (NS <= 45), then sigma^2 and the status
constexpr int kHeadSigma2 = 48, kHeadStatus = 49;
constexpr int kGlobal = DCX_COV_GLOBAL_WORDS;
constexpr int kPoseCov = DCX_COV_POSE_WORDS;

struct CovTheta {
    double v[9];
};

// The workspace: the head, then per view.  One layout for both models, sized by the larger (the pinhole's); a model's kernels
// stride by their own sizes inside it.
struct CovWs {
    double *head, *m, *yz, *sc, *uinv;                    // uinv: U_i^-1 packed (21)
    int* info;                                            // per view: failed, kept rows
};

size_t cov_layout(void* base, int batch, CovWs* w) {
    using P = PinholeCalib;
    static_assert(FisheyeCalib::kEntries <= P::kEntries && FisheyeCalib::kYZ <= P::kYZ && FisheyeCalib::kSC <= P::kSC, "layout");
    const size_t B = (size_t)batch;
    Carver c{(char*)base, 0};
    CovWs r;
    r.head = c.take<double>(kCovHead);
    r.m = c.take<double>(B * P::kEntries);
    r.yz = c.take<double>(B * P::kYZ);
    r.sc = c.take<double>(B * P::kSC);
    r.uinv = c.take<double>(B * 21);
    r.info = c.take<int>(B * 2);
    if (w) *w = r;
    return c.at;
}

template <class M>
__global__ __launch_bounds__(kLanes) void cov_evaluate_kernel(CornerPool pl, const int32_t* __restrict__ status,
                                                              const double* __restrict__ pose, const uint8_t* __restrict__ mask,
                                                              CovTheta th, CovWs ws) {
    constexpr int NC = M::NC, NQ = M::NQ;
    __shared__ double sj[2 * kLanes][kLdsStride];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (status[b] != DCX_PNP_OK) return;
    const int n = pl.counts[b], s0 = pl.starts[b];
    if (n < 0 || s0 < 0 || (long long)s0 + n > (long long)pl.pool) {      // its slots are not read
        if (lane == 0) {
            ws.info[2 * (long long)b] = 1;
            ws.info[2 * (long long)b + 1] = 0;
        }
        return;
    }
    const Frame f = pl.frame(n, s0);
    const uint8_t* keep = mask ? mask + s0 : nullptr;
    const typename M::Camera cam = M::camera(th.v);
    double p[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) p[i] = pose[8 * (long long)b + i];
    double R[9], G[2][9];
    pose_basis(p, R, G);
    int ea[NQ], eb[NQ];
    lane_entries<NC, NQ>(lane, ea, eb);
    double acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
    bool behind = false;
    double kept[1] = {0.0};
    accumulate_rows<NC, NQ, kLdsStride>(
        n,
        [&](int i, double* ju, double* jv) {
            if (keep && keep[i] == 0) return true;        // a row of zeros
            kept[0] += 1.0;
            double mx, my, u, v, ru, rv;
            f.load(i, mx, my, u, v);
            if (!project_point<true>(cam, p, R, G, mx, my, u, v, ru, rv, ju, jv)) return false;
            ju[NC - 1] = ru;
            jv[NC - 1] = rv;
            return true;
        },
        sj, ea, eb, acc, behind);
    const bool failed = __any(behind);
    wave_sum(kept);
    double* m = ws.m + (long long)b * M::kEntries;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int e = lane + kLanes * q;
        if (e < M::kEntries) m[e] = acc[q];
    }
    if (lane == 0) {
        ws.info[2 * (long long)b] = failed ? 1 : 0;
        ws.info[2 * (long long)b + 1] = (int)kept[0];
    }
}

template <class M>
__global__ __launch_bounds__(kLanes) void cov_schur_kernel(const int32_t* __restrict__ status, CovWs ws) {
    constexpr int NG = M::NG, NC = M::NC;
    __shared__ double sy[NG + 1][6];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (status[b] != DCX_PNP_OK || ws.info[2 * (long long)b]) return;
    const double* m = ws.m + (long long)b * M::kEntries;
    if (!schur_view<NG>(m, 1.0, lane, sy, ws.yz + (long long)b * M::kYZ, ws.sc + (long long)b * M::kSC)) {
        if (lane == 0) ws.info[2 * (long long)b] = 1;
        return;
    }
    if (lane >= 6) return;
    double u[21], L[21], rhs[6], x[6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) u[pk<6>(i, j)] = m[pk<NC>(NG + i, NG + j)];
    cholesky_factor<6>(u, 1.0, L);                        // positive definite: schur_view has just factored it
#pragma unroll
    for (int k = 0; k < 6; ++k) rhs[k] = k == lane ? 1.0 : 0.0;
    cholesky_substitute<6>(L, rhs, x);
    double* o = ws.uinv + (long long)b * 21;
#pragma unroll
    for (int k = 0; k < 6; ++k)
        if (k <= lane) o[pk<6>(k, lane)] = x[k];          // column `lane` of U^-1, its part on and above the diagonal
}

// thread 0 of reduce_invert: the totals -> the status; with DCX_COV_OK inv (S^-1, NG x NG) and sigma2
template <int NG>
__device__ int cov_invert(const double* tot, double* S, double* L, double* y, double* inv, double& sigma2, double& dof) {
    constexpr int NS = NG * (NG + 1) / 2;
    const double cost = tot[2 * NS], points = tot[2 * NS + 1], views = tot[2 * NS + 2], failed = tot[2 * NS + 3];
    dof = 2.0 * points - NG - 6.0 * views;
    if (views == 0.0) return DCX_COV_NO_VIEWS;
    if (!(dof > 0.0)) return DCX_COV_NO_DOF;
    if (failed != 0.0 || !isfinite(cost)) return DCX_COV_SINGULAR;
    for (int e = 0; e < NS; ++e) S[e] = tot[e] - tot[NS + e];
    for (int i = 0; i < NG; ++i) {
        for (int j = 0; j <= i; ++j) {
            double s = S[pk<NG>(i, j)];
            for (int k = 0; k < j; ++k) s -= L[pk<NG>(i, k)] * L[pk<NG>(j, k)];
            if (i == j) {
                if (!(s > 0) || !isfinite(s)) return DCX_COV_SINGULAR;
                L[pk<NG>(i, i)] = sqrt(s);
            } else {
                L[pk<NG>(i, j)] = s / L[pk<NG>(j, j)];
            }
        }
    }
    sigma2 = cost / dof;
    for (int c = 0; c < NG; ++c) {                        // column c of S^-1; its part on and above the diagonal is kept
        for (int i = 0; i < NG; ++i) {
            double s = i == c ? 1.0 : 0.0;
            for (int k = 0; k < i; ++k) s -= L[pk<NG>(i, k)] * y[k];
            y[i] = s / L[pk<NG>(i, i)];
        }
        for (int i = NG - 1; i >= 0; --i) {
            double s = y[i];
            for (int k = i + 1; k < NG; ++k) s -= L[pk<NG>(k, i)] * y[k];
            y[i] = s / L[pk<NG>(i, i)];
        }
        for (int r = 0; r <= c; ++r) {
            if (!isfinite(sigma2 * y[r]) || (r == c && !(sigma2 * y[r] >= 0))) return DCX_COV_SINGULAR;
            inv[pk<NG>(r, c)] = y[r];
        }
    }
    return DCX_COV_OK;
}

template <class M>
__global__ __launch_bounds__(kRedThreads) void cov_reduce_invert_kernel(int batch, const int32_t* __restrict__ status, CovWs ws,
                                                                        double* __restrict__ global) {
    constexpr int NG = M::NG, NC = M::NC, NS = M::NS, kTot = 2 * NS + 4;   // V, sum S_i, then cost, points, views, failed views
    static_assert(kTot <= 128 && NS + 2 <= kCovHead && NS <= kHeadSigma2 && DCX_COV_STD + NG <= DCX_COV_SIGMA2, "layout");
    __shared__ double part[kSlices][kTot];
    __shared__ double tot[kTot], S[NS], L[NS], y[NG], inv[NS], out[kGlobal];
    const int t = threadIdx.x, e = t % 128, sl = t / 128;
    if (e < kTot) {
        int src = 0;
        if (e < 2 * NS) {
            int a, c;
            unpk<NG>(e < NS ? e : e - NS, a, c);
            src = e < NS ? pk<NC>(a, c) : e - NS;
        }
        double s = 0.0;
        for (int b = sl; b < batch; b += kSlices) {
            if (status[b] != DCX_PNP_OK) continue;
            const bool failed = ws.info[2 * (long long)b] != 0;
            if (e >= 2 * NS + 1) {
                s += e == 2 * NS + 1 ? (double)ws.info[2 * (long long)b + 1] : e == 2 * NS + 2 ? 1.0 : failed ? 1.0 : 0.0;
            } else if (!failed) {                         // (a failed view's entries were not all written)
                s += e < NS ? ws.m[(long long)b * M::kEntries + src]
                     : e < 2 * NS ? ws.sc[(long long)b * M::kSC + src] : ws.m[(long long)b * M::kEntries + M::kCost];
            }
        }
        part[sl][e] = s;
    }
    if (t < kGlobal) out[t] = 0.0;
    __syncthreads();
    if (t == 0) {
        for (int i = 0; i < kTot; ++i) {
            double s = 0.0;
            for (int k = 0; k < kSlices; ++k) s += part[k][i];
            tot[i] = s;
        }
        double sigma2 = 0.0, dof = 0.0;
        const int code = cov_invert<NG>(tot, S, L, y, inv, sigma2, dof);
        if (code == DCX_COV_OK) {
            for (int a = 0; a < NG; ++a) {
                for (int c = 0; c < NG; ++c) out[DCX_COV_COV + a * NG + c] = sigma2 * inv[pk<NG>(a, c)];
                out[DCX_COV_STD + a] = sqrt(sigma2 * inv[pk<NG>(a, a)]);
            }
            out[DCX_COV_SIGMA2] = sigma2;
        }
        out[DCX_COV_DOF] = dof;
        out[DCX_COV_POINTS] = tot[2 * NS + 1];
        out[DCX_COV_VIEWS] = tot[2 * NS + 2];
        out[DCX_COV_STATUS] = (double)code;
        for (int i = 0; i < NS; ++i) ws.head[i] = code == DCX_COV_OK ? inv[i] : 0.0;
        ws.head[kHeadSigma2] = code == DCX_COV_OK ? sigma2 : 0.0;
        ws.head[kHeadStatus] = (double)code;
    }
    __syncthreads();
    if (t < kGlobal) global[t] = out[t];
}

template <class M>
__global__ __launch_bounds__(kLanes) void cov_pose_kernel(const int32_t* __restrict__ status, CovWs ws, double* __restrict__ pose_cov) {
    constexpr int NG = M::NG;
    const int b = blockIdx.x, lane = threadIdx.x;
    if (lane >= kPoseCov) return;
    double v = 0.0;
    if (status[b] == DCX_PNP_OK && ws.head[kHeadStatus] == (double)DCX_COV_OK) {
        // entry (r, c) of the 6x6, or past the 36 the diagonal entry whose root is the standard deviation; both halves of the
        // matrix take the entry on or above the diagonal, so it is symmetric to the bit
        const int r0 = lane < 36 ? lane / 6 : lane - 36, c0 = lane < 36 ? lane % 6 : lane - 36;
        const int r = min(r0, c0), c = max(r0, c0);
        const double* yz = ws.yz + (long long)b * M::kYZ;
        double s = ws.uinv[(long long)b * 21 + pk<6>(r, c)];
        for (int a = 0; a < NG; ++a) {
            double ta = 0.0;
            for (int k = 0; k < NG; ++k) ta += ws.head[pk<NG>(a, k)] * yz[c * NG + k];
            s += yz[r * NG + a] * ta;
        }
        v = ws.head[kHeadSigma2] * s;
        if (lane >= 36) v = sqrt(v);
    }
    pose_cov[(long long)b * kPoseCov + lane] = v;
}

template <class M>
hipError_t cov_run(hipStream_t s, const CornerPool& pl, int batch, const double* h_theta, const int32_t* d_view_status,
                   const double* d_pose, const uint8_t* d_mask, const CovWs& ws, double* d_global, double* d_pose_cov) {
    CovTheta th{};
    for (int i = 0; i < M::NG; ++i) th.v[i] = h_theta[i];
    const dim3 views((unsigned)batch), wave(kLanes), one(1), red(kRedThreads);
    hipLaunchKernelGGL(cov_evaluate_kernel<M>, views, wave, 0, s, pl, d_view_status, d_pose, d_mask, th, ws);
    hipLaunchKernelGGL(cov_schur_kernel<M>, views, wave, 0, s, d_view_status, ws);
    hipLaunchKernelGGL(cov_reduce_invert_kernel<M>, one, red, 0, s, batch, d_view_status, ws, d_global);
    hipLaunchKernelGGL(cov_pose_kernel<M>, views, wave, 0, s, d_view_status, ws, d_pose_cov);
    return hipGetLastError();
}

}  // namespace

extern "C" size_t dcx_calibrate_uncertainty_workspace_bytes(int batch) { return batch > 0 ? cov_layout(nullptr, batch, nullptr) : 0; }

extern "C" int dcx_calibrate_uncertainty_pool(const int32_t* d_counts, const int32_t* d_starts, const int32_t* d_rows, const float* d_xy,
                                              int batch, int pool, int col_count, int row_count, double square_len, int model,
                                              const double* h_theta, const int32_t* d_view_status, const double* d_pose,
                                              const uint8_t* d_mask, void* d_workspace, size_t workspace_bytes, double* d_global,
                                              double* d_pose_cov, void* stream) {
    CornerPool pl;
    if (!corner_pool(d_counts, d_starts, d_rows, d_xy, batch, pool, col_count, row_count, square_len, pl)) return DCX_E_ARG;
    if (model != DCX_CAMERA_PINHOLE && model != DCX_CAMERA_FISHEYE) return DCX_E_ARG;
    if (!h_theta || !d_view_status || !d_pose || !d_workspace || !d_global || !d_pose_cov) return DCX_E_ARG;
    if (workspace_bytes < cov_layout(nullptr, batch, nullptr)) return DCX_E_WS;
    CovWs ws;
    cov_layout(d_workspace, batch, &ws);
    hipStream_t s = (hipStream_t)stream;
    DCX_CHECK_HIP(model == DCX_CAMERA_PINHOLE
                      ? cov_run<PinholeCalib>(s, pl, batch, h_theta, d_view_status, d_pose, d_mask, ws, d_global, d_pose_cov)
                      : cov_run<FisheyeCalib>(s, pl, batch, h_theta, d_view_status, d_pose, d_mask, ws, d_global, d_pose_cov));
    return 0;
}
