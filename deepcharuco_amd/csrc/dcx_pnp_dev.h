// dcx_pnp_dev.h -- the pool reader, the consensus steps and the PnP solver, on top of dcx_camera_dev.h (camera model, rotations) and
// dcx_mat_dev.h (small matrices, reductions): the corner pool as every kernel receives it (CornerPool) and the one host-side check
// that fills it from the C ABI's pool arguments (corner_pool), the frame types (Frame, IndexedFrame), the per-frame checks
// (frame_status, ranges_overlap), the normal equations of a frame at a pose (evaluate), the planar DLT homography, the planar pose
// init and the PnP Levenberg-Marquardt (solve), which dcx_pnp.hip runs per frame, dcx_calib.hip and dcx_stereo.hip per view, and
// dcx_pnp_ransac.hip over an index list of a frame's rows (the frame type is a template parameter).  Also here: what the consensus
// searches (dcx_pnp_ransac.hip, dcx_calib_ransac.hip) and the masked stereo solve share: the slot-range overlap test, the sampler,
// the four-point homography, one row's reprojection error and the first-maximum score search.
// deepcharuco_amd/pnp.py restates every step (its functions of the same names).  Everything is force-inlined and has internal
// linkage, so each translation unit compiles its own copy.
#pragma once
#include "dcx_camera_dev.h"

namespace {

constexpr int kLmMaxIter = 20;
constexpr double kLmEps = 1.1920928955078125e-07;   // FLT_EPSILON

struct Frame {
    const int32_t* rows;     // this frame's rows (x, y, id, cell), n of them
    const float* xy;         // this frame's refined xy, or null
    int n;
    int rm1;                 // row_count - 1
    double square_len;

    // board point (float32-rounded as inference.py:20-26's np.float32 table) and image point (float32, inference.py:27)
    __device__ __forceinline__ void load(int i, double& X, double& Y, double& u, double& v) const {
        const int id = rows[4 * i + 2];
        X = (double)__double2float_rn((double)(1 + id % rm1) * square_len);
        Y = (double)__double2float_rn((double)(1 + id / rm1) * square_len);
        if (xy) {
            u = (double)xy[2 * i];
            v = (double)xy[2 * i + 1];
        } else {
            u = (double)(float)rows[4 * i];
            v = (double)(float)rows[4 * i + 1];
        }
    }
};

// The corner pool dcx_infer_batch writes, with the board its ids refer to: what the five pool entries (dcx_solve_pnp_pool,
// dcx_solve_pnp_ransac_pool, dcx_calibrate_pool, dcx_calibrate_ransac_pool, dcx_stereo_calibrate_pool) pass to their kernels.
struct CornerPool {
    const int32_t* counts;   // rows per frame
    const int32_t* starts;   // a frame's first slot
    const int32_t* rows;     // (x, y, id, cell) per slot
    const float* xy;         // refined xy per slot, or null: the integer rows are the image points
    int pool, n_ids, rm1;    // slots; (col_count - 1) * (row_count - 1); row_count - 1
    double square_len;

    __device__ __forceinline__ Frame frame(int n, long long s0) const {
        return Frame{rows + 4 * s0, xy ? xy + 2 * s0 : nullptr, n, rm1, square_len};
    }
    __device__ __forceinline__ Frame frame(int b) const { return frame(counts[b], starts[b]); }
};

// The C ABI's pool arguments -> the pool, or false: what every pool entry refuses with DCX_E_ARG before it looks at anything else
// of its own (a null pool pointer, no frames, a negative pool, a board without inner corners or with more than 2^31 - 1 of them,
// a non-finite square).  d_xy may be null.
inline bool corner_pool(const int32_t* d_counts, const int32_t* d_starts, const int32_t* d_rows, const float* d_xy, int batch, int pool,
                        int col_count, int row_count, double square_len, CornerPool& pl) {
    if (!d_counts || !d_starts || !d_rows || batch <= 0 || pool < 0 || col_count < 2 || row_count < 2) return false;
    if ((long long)(col_count - 1) * (row_count - 1) > 0x7fffffffLL || !isfinite(square_len)) return false;
    pl = CornerPool{d_counts, d_starts, d_rows, d_xy, pool, (col_count - 1) * (row_count - 1), row_count - 1, square_len};
    return true;
}

// The rows of a frame picked by an index list (the RANSAC refit over the inlier slots): row i of this frame is row idx[i] of base.
struct IndexedFrame {
    Frame base;
    const int32_t* idx;
    int n;

    __device__ __forceinline__ void load(int i, double& X, double& Y, double& u, double& v) const { base.load(idx[i], X, Y, u, v); }
};

// The solver (evaluate, homography, init_pose, solve, row_error2) is a template on the camera class C and touches it through four
// functions only: has_distortion(cam), undistort(cam, dist, u, v, x, y), project<JAC>(cam, q, u, v, ru, rv, du, dv) and
// points_inside(f, cam): does every image point of the frame lie inside the camera's model?  The pinhole (PnpCamera,
// dcx_camera_dev.h) takes every pixel; the fisheye (FisheyeCamera, dcx_fisheye_dev.h) refuses theta >= pi/2.
template <class F>
__device__ __forceinline__ bool points_inside(const F&, const PnpCamera&) { return true; }

// Sum over the frame's points of the squared reprojection error at pose p (+inf if a point is not in front of the camera) and,
// with JAC, of JtJ (21, packed) and Jtr (6).  acc = {cost, JtJ[21], Jtr[6]} on return, identical in every lane.
template <bool JAC, class F, class C>
__device__ __forceinline__ void evaluate(const F& f, const C& cam, const double* p, double (&acc)[28]) {
    double R[9], G[2][9];
    if (JAC) pose_basis(p, R, G);
    else rodrigues(p, R);
#pragma unroll
    for (int i = 0; i < 28; ++i) acc[i] = 0.0;
    for (int i = threadIdx.x; i < f.n; i += kLanes) {
        double mx, my, u, v, q[3], ru, rv, du[3], dv[3];
        f.load(i, mx, my, u, v);
        board_point(R, p + 3, mx, my, q);
        if (!project<JAC>(cam, q, u, v, ru, rv, du, dv)) {
            acc[0] = INFINITY;
            continue;
        }
        acc[0] += ru * ru + rv * rv;
        if (!JAC) continue;
        double ju[6], jv[6];
        pose_columns(du, dv, mx, my, G, ju, jv);
#pragma unroll
        for (int a = 0; a < 6; ++a) {
#pragma unroll
            for (int b = a; b < 6; ++b) acc[1 + pk<6>(a, b)] += ju[a] * ju[b] + jv[a] * jv[b];
            acc[22 + a] += ju[a] * ru + jv[a] * rv;
        }
    }
    wave_sum(acc);
}

// Planar DLT (pnp._homography) of the board points to the (undistorted) image points -> status; H (row major, h33 = 1) maps
// the centred board points (X - mcx, Y - mcy) to the image points.
template <class F, class C>
__device__ __forceinline__ int homography(const F& f, const C& cam, bool dist, double* H, double& mc_x, double& mc_y) {
    const int lane = threadIdx.x;
    const double n = (double)f.n;
    // centroids of the board points and of the normalised image points
    double s1[4] = {0, 0, 0, 0};
    for (int i = lane; i < f.n; i += kLanes) {
        double mx, my, u, v, x, y;
        f.load(i, mx, my, u, v);
        undistort(cam, dist, u, v, x, y);
        s1[0] += mx; s1[1] += my; s1[2] += x; s1[3] += y;
    }
    wave_sum(s1);
    const double mcx = s1[0] / n, mcy = s1[1] / n, icx = s1[2] / n, icy = s1[3] / n;
    // second moments of the centred board points (collinearity) and mean distances (Hartley scales)
    double s2[5] = {0, 0, 0, 0, 0};
    for (int i = lane; i < f.n; i += kLanes) {
        double mx, my, u, v, x, y;
        f.load(i, mx, my, u, v);
        undistort(cam, dist, u, v, x, y);
        const double X = mx - mcx, Y = my - mcy;
        s2[0] += X * X; s2[1] += X * Y; s2[2] += Y * Y;
        s2[3] += sqrt(X * X + Y * Y);
        s2[4] += sqrt((x - icx) * (x - icx) + (y - icy) * (y - icy));
    }
    wave_sum(s2);
    {
        const double tr = s2[0] + s2[2], df = s2[0] - s2[2];
        const double rt = sqrt(df * df + 4.0 * s2[1] * s2[1]);
        const double e1 = 0.5 * (tr + rt), e0 = 0.5 * (tr - rt);
        if (!(e0 > 1e-10 * e1)) return DCX_PNP_DEGENERATE;       // collinear board points
    }
    const double d1 = s2[3] / n, d2 = s2[4] / n;
    const double sc1 = d1 > 0 ? M_SQRT2 / d1 : 0.0, sc2 = d2 > 0 ? M_SQRT2 / d2 : 0.0;
    // DLT normal matrix of the Hartley-normalised correspondences
    double M[45];
#pragma unroll
    for (int i = 0; i < 45; ++i) M[i] = 0.0;
    for (int i = lane; i < f.n; i += kLanes) {
        double mx, my, u, v, x, y;
        f.load(i, mx, my, u, v);
        undistort(cam, dist, u, v, x, y);
        const double X = sc1 * (mx - mcx), Y = sc1 * (my - mcy);
        const double xu = sc2 * (x - icx), yv = sc2 * (y - icy);
        const double r1[9] = {X, Y, 1.0, 0.0, 0.0, 0.0, -xu * X, -xu * Y, -xu};
        const double r2[9] = {0.0, 0.0, 0.0, X, Y, 1.0, -yv * X, -yv * Y, -yv};
#pragma unroll
        for (int a = 0; a < 9; ++a)
#pragma unroll
            for (int b = a; b < 9; ++b) M[pk<9>(a, b)] += r1[a] * r1[b] + r2[a] * r2[b];
    }
    wave_sum(M);
    double vrow[1][9];               // row `lane` of the eigenvector matrix (lanes >= 9 carry a zero row)
#pragma unroll
    for (int c = 0; c < 9; ++c) vrow[0][c] = (c == lane) ? 1.0 : 0.0;
    jacobi<9, 1>(M, vrow);
    // smallest eigenvalue (first on ties), its eigenvector's entry in this lane's row, the next smallest and the largest |w|
    int kmin = 0;
    double wmin = M[pk<9>(0, 0)], wmax = fabs(wmin), e = vrow[0][0];
#pragma unroll
    for (int c = 1; c < 9; ++c) {
        const double w = M[pk<9>(c, c)];
        if (w < wmin) { wmin = w; kmin = c; e = vrow[0][c]; }
        wmax = fmax(wmax, fabs(w));
    }
    double w2 = INFINITY;
#pragma unroll
    for (int c = 0; c < 9; ++c)
        if (c != kmin) w2 = fmin(w2, M[pk<9>(c, c)]);
    if (!(w2 > 1e-12 * wmax)) return DCX_PNP_DEGENERATE;           // two (near) null directions
    double hn[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) hn[i] = __shfl(e, i, kLanes);
    // H = T2^-1 Hn T1, T1 = diag(sc1, sc1, 1) on the centred board points, T2 = Hartley of the image points
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double ri0 = hn[i * 3 + 0] * sc1, ri1 = hn[i * 3 + 1] * sc1, ri2 = hn[i * 3 + 2];
        H[i * 3 + 0] = ri0; H[i * 3 + 1] = ri1; H[i * 3 + 2] = ri2;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double h2 = H[6 + j];
        H[0 + j] = H[0 + j] / sc2 + icx * h2;
        H[3 + j] = H[3 + j] / sc2 + icy * h2;
    }
    double hmax = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) hmax = fmax(hmax, fabs(H[i]));
    if (!(fabs(H[8]) > 1e-12 * hmax)) return DCX_PNP_DEGENERATE;
    const double h22 = H[8];
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] /= h22;
    mc_x = mcx;
    mc_y = mcy;
    return DCX_PNP_OK;
}

// ---- the consensus searches' shared steps (dcx_pnp_ransac.hip, dcx_calib_ransac.hip): the per-frame checks, the slot-range overlap
// test, the counter-hash sampler, the closed-form homography through four rows, one row's reprojection error and the first maximum
// of the scores

constexpr int kMaxIterations = 4096; // hypotheses per frame (pnp.RANSAC_MAX_ITERATIONS)
constexpr int kSampleTries = 8;      // complete 4-samples per hypothesis (pnp.RANSAC_SAMPLE_TRIES)
constexpr int kMaxDraws = 256;       // slot draws per hypothesis, redraws included (pnp.RANSAC_MAX_DRAWS)

// The per-frame checks, in the order of dcx_solve_pnp_kernel (which spells them out itself, see there) -> DCX_PNP_OK if the frame's
// rows can be read and solved.  Wave-wide.
__device__ __forceinline__ int frame_status(const CornerPool& pl, int b, int& n, int& s0) {
    n = pl.counts[b];
    s0 = pl.starts[b];
    if (n <= 0) return DCX_PNP_TOO_FEW;
    if (s0 < 0 || (long long)s0 + n > (long long)pl.pool) return DCX_PNP_TRUNCATED;   // (its slots are not read)
    if (n < 4) return DCX_PNP_TOO_FEW;
    bool bad = false;
    for (int i = threadIdx.x; i < n; i += kLanes) {
        const int id = pl.rows[4 * ((long long)s0 + i) + 2];
        bad |= id < 0 || id >= pl.n_ids;
    }
    return __any(bad) ? DCX_PNP_BAD_ID : DCX_PNP_OK;
}

// One wave per view b of a pool whose views own their slot ranges: does b's range (the part inside the pool) meet another view's?
// The lanes share the other views out.  Wave-wide.
__device__ __forceinline__ bool ranges_overlap(const CornerPool& pl, int batch, int b) {
    const int32_t *counts = pl.counts, *starts = pl.starts;
    const long long n = counts[b], s0 = starts[b], pool = pl.pool;
    if (n <= 0) return false;
    const long long lo = s0 < 0 ? 0 : s0, hi = s0 + n < pool ? s0 + n : pool;
    if (lo >= hi) return false;
    bool hit = false;
    for (int o = threadIdx.x; o < batch; o += kLanes) {
        const long long on = counts[o], os = starts[o];
        if (o == b || on <= 0) continue;
        const long long olo = os < 0 ? 0 : os, ohi = os + on < pool ? os + on : pool;
        hit |= olo < ohi && olo < hi && lo < ohi;
    }
    return __any(hit);
}

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    return x ^ (x >> 16);
}

// draw c of hypothesis h of a frame with n rows -> a slot in [0, n)  (pnp._ransac_draw)
__device__ __forceinline__ int ransac_draw(uint32_t seed, uint32_t n, uint32_t h, uint32_t c) {
    const uint32_t r = mix32(seed ^ mix32(n * 0x9E3779B9u + mix32(h * 0x85EBCA6Bu + c)));
    return (int)(((uint64_t)r * n) >> 32);
}

__device__ __forceinline__ bool on_a_line(const int* gx, const int* gy, int a, int b, int c) {
    return (long long)(gx[b] - gx[a]) * (gy[c] - gy[a]) - (long long)(gy[b] - gy[a]) * (gx[c] - gx[a]) == 0;
}

// pnp._ransac_sample: four distinct slots whose ids are distinct and hold no collinear triple on the id grid; false if none came
__device__ __forceinline__ bool ransac_sample(const int32_t* rows, uint32_t seed, int n, int h, int rm1, int (&s)[4]) {
    uint32_t c = 0;
#pragma unroll 1
    for (int attempt = 0; attempt < kSampleTries; ++attempt) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            while (true) {
                if (c >= (uint32_t)kMaxDraws) return false;
                const int i = ransac_draw(seed, (uint32_t)n, (uint32_t)h, c++);
                bool held = false;
#pragma unroll
                for (int j = 0; j < k; ++j) held |= s[j] == i;
                if (!held) {
                    s[k] = i;
                    break;
                }
            }
        }
        int id[4], gx[4], gy[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            id[k] = rows[4 * s[k] + 2];
            gx[k] = id[k] % rm1;
            gy[k] = id[k] / rm1;
        }
        const bool shared = id[0] == id[1] || id[0] == id[2] || id[0] == id[3] || id[1] == id[2] || id[1] == id[3] || id[2] == id[3];
        if (!shared && !on_a_line(gx, gy, 1, 2, 3) && !on_a_line(gx, gy, 0, 2, 3) && !on_a_line(gx, gy, 0, 1, 3) &&
            !on_a_line(gx, gy, 0, 1, 2))
            return true;
    }
    return false;
}

// pnp._projective_basis: the 3x3 that sends e1, e2, e3, (1,1,1) to the four points, each up to scale
__device__ __forceinline__ void projective_basis(const double* x, const double* y, double* A) {
    const double m[9] = {x[0], x[1], x[2], y[0], y[1], y[2], 1.0, 1.0, 1.0};
    double a[9];
    adjugate(m, a);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double lam = a[j * 3] * x[3] + a[j * 3 + 1] * y[3] + a[j * 3 + 2];
        A[j] = m[j] * lam;
        A[3 + j] = m[3 + j] * lam;
        A[6 + j] = lam;
    }
}

// squared reprojection error (px^2) of one row at the pose (R, t) through the full distortion model; +inf if the point is not in
// front of the camera (evaluate()'s projection, per row)
template <class C>
__device__ __forceinline__ double row_error2(const double* R, const double* t, const C& cam, double mx, double my, double u,
                                             double v) {
    double q[3], ru, rv;
    board_point(R, t, mx, my, q);
    if (!project<false>(cam, q, u, v, ru, rv, nullptr, nullptr)) return INFINITY;
    return ru * ru + rv * rv;
}

// The first maximum of a frame's `iterations` scores: the highest score, the lowest h among equals (ascending h in each lane, then
// a butterfly with the same rule).  best < 0: no hypothesis scored.  Wave-wide; every lane gets the same answer.
__device__ __forceinline__ void best_hypothesis(const int32_t* scores, int iterations, int& best, int& bh) {
    best = -1;
    bh = 0x7fffffff;
    for (int h = threadIdx.x; h < iterations; h += kLanes) {
        const int sc = scores[h];
        if (sc > best) {
            best = sc;
            bh = h;
        }
    }
#pragma unroll
    for (int m = kLanes / 2; m >= 1; m >>= 1) {
        const int ob = __shfl_xor(best, m, kLanes), oh = __shfl_xor(bh, m, kLanes);
        if (ob > best || (ob == best && oh < bh)) {
            best = ob;
            bh = oh;
        }
    }
}

// Four sampled rows of a frame, held by one lane: board points and undistorted image points.
struct Sample {
    double mx[4], my[4], x[4], y[4];
};

// pnp._homography4: the homography through exactly four points in closed form, H = B adj(A) with A, B the projective bases of the
// centred board points and of the image points.  init_pose() picks this overload for a Sample; no cross-lane step.
template <class C>
__device__ __forceinline__ int homography(const Sample& q, const C&, bool, double* H, double& mc_x, double& mc_y) {
    const double mcx = (q.mx[0] + q.mx[1] + q.mx[2] + q.mx[3]) / 4.0, mcy = (q.my[0] + q.my[1] + q.my[2] + q.my[3]) / 4.0;
    double cx[4], cy[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        cx[k] = q.mx[k] - mcx;
        cy[k] = q.my[k] - mcy;
    }
    double A[9], B[9], Aa[9];
    projective_basis(cx, cy, A);
    projective_basis(q.x, q.y, B);
    adjugate(A, Aa);
    double hmax = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            H[i * 3 + j] = B[i * 3] * Aa[j] + B[i * 3 + 1] * Aa[3 + j] + B[i * 3 + 2] * Aa[6 + j];
            hmax = fmax(hmax, fabs(H[i * 3 + j]));
        }
    if (!(fabs(H[8]) > 1e-12 * hmax)) return DCX_PNP_DEGENERATE;
    const double h22 = H[8];
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] /= h22;
    mc_x = mcx;
    mc_y = mcy;
    return DCX_PNP_OK;
}

// Planar initialisation (pnp._init_pose) -> status; p0 = rvec, tvec.  homography() is found by the frame's type: a frame of exactly
// four rows may bring its own (dcx_pnp_ransac.hip); everything after it is per lane.
template <class F, class C>
__device__ __forceinline__ int init_pose(const F& f, const C& cam, bool dist, double* p0) {
    double H[9], mcx, mcy;
    const int st = homography(f, cam, dist, H, mcx, mcy);
    if (st != DCX_PNP_OK) return st;
    const double n1 = sqrt(H[0] * H[0] + H[3] * H[3] + H[6] * H[6]);
    const double n2 = sqrt(H[1] * H[1] + H[4] * H[4] + H[7] * H[7]);
    const double i1 = 1.0 / fmax(n1, 2.2e-16), i2 = 1.0 / fmax(n2, 2.2e-16), it = 2.0 / fmax(n1 + n2, 2.2e-16);
    double Rr[9];
    Rr[0] = H[0] * i1; Rr[3] = H[3] * i1; Rr[6] = H[6] * i1;
    Rr[1] = H[1] * i2; Rr[4] = H[4] * i2; Rr[7] = H[7] * i2;
    Rr[2] = Rr[3] * Rr[7] - Rr[6] * Rr[4];
    Rr[5] = Rr[6] * Rr[1] - Rr[0] * Rr[7];
    Rr[8] = Rr[0] * Rr[4] - Rr[3] * Rr[1];
    double t[3] = {H[2] * it, H[5] * it, H[8] * it};
    double Q[9];
    if (!polar_factor(Rr, Q)) return DCX_PNP_DEGENERATE;
    rvec_of(Q, p0);
    double R[9];
    rodrigues(p0, R);
    p0[3] = t[0] - (R[0] * mcx + R[1] * mcy);
    p0[4] = t[1] - (R[3] * mcx + R[4] * mcy);
    p0[5] = t[2] - (R[6] * mcx + R[7] * mcy);
#pragma unroll
    for (int i = 0; i < 6; ++i)
        if (!isfinite(p0[i])) return DCX_PNP_NONFINITE;
    return DCX_PNP_OK;
}

template <class F, class C>
__device__ __forceinline__ int solve(const F& f, const C& cam, double* pose) {
    if (!points_inside(f, cam)) return DCX_PNP_DEGENERATE;
    const bool dist = has_distortion(cam);
    double p[6];
    int st = init_pose(f, cam, dist, p);
    if (st != DCX_PNP_OK) return st;
    double acc[28];
    evaluate<true>(f, cam, p, acc);
    if (!isfinite(acc[0])) return DCX_PNP_DEGENERATE;
    double jtj[21], jtr[6];
    double prev_cost = acc[0], cost = acc[0];
    int lg = -3, iters = 0;
#pragma unroll 1
    while (true) {
#pragma unroll
        for (int i = 0; i < 21; ++i) jtj[i] = acc[1 + i];
#pragma unroll
        for (int i = 0; i < 6; ++i) jtr[i] = acc[22 + i];
        double prev[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) prev[i] = p[i];
#pragma unroll 1
        while (true) {
            double x[6];
            if (!cholesky_solve(jtj, jtr, 1.0 + pow(10.0, (double)lg), x)) return DCX_PNP_DEGENERATE;
#pragma unroll
            for (int i = 0; i < 6; ++i) p[i] = prev[i] - x[i];
            evaluate<false>(f, cam, p, acc);
            cost = acc[0];
            if (!(cost <= prev_cost)) {
                if (++lg <= 16) continue;
            }
            break;
        }
        lg = max(lg - 1, -16);
        ++iters;
        double dn = 0.0, pn = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            dn += (p[i] - prev[i]) * (p[i] - prev[i]);
            pn += prev[i] * prev[i];
        }
        if (iters >= kLmMaxIter || sqrt(dn) < kLmEps * sqrt(pn)) break;
        prev_cost = cost;
        evaluate<true>(f, cam, p, acc);
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) pose[i] = p[i];
    pose[6] = sqrt(cost / (double)f.n);
    pose[7] = (double)iters;
#pragma unroll
    for (int i = 0; i < 6; ++i)
        if (!isfinite(p[i])) return DCX_PNP_NONFINITE;
    if (isnan(cost)) return DCX_PNP_NONFINITE;
    if (!isfinite(cost)) return DCX_PNP_DEGENERATE;
    return DCX_PNP_OK;
}

}  // namespace
