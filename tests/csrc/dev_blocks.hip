// dev_blocks.hip -- test-only harness: one thin kernel and one extern "C" launcher around each fp64 device building block of
// deepcharuco_amd/csrc (dcx_mat_dev.h, dcx_camera_dev.h, dcx_fisheye_dev.h, dcx_pnp_dev.h), so that tests/test_gpu_dev_blocks.py can
// hold each block by itself to exact math.  The headers give every translation unit its own copy of the blocks; this is one more.
// It pins the blocks' source text, not the instructions inside the library's kernels.
//
// A kernel copies its arguments in, calls the block and copies the results out: no arithmetic of its own.  Per-lane blocks run one
// instance per thread behind an i < n guard.  Wave-wide blocks run one instance per 64-thread workgroup and write every lane's
// result.  Instance i reads in + i * NIN doubles (iin + i * NIIN int32) and writes out + i * NOUT doubles (iout + i * NIOUT int32);
// for a wave-wide block the outputs are per lane: (i * 64 + lane) * NOUT.  What a block leaves unwritten keeps the caller's fill.
// Every launcher refuses (-1) null pointers, n <= 0 and n > DCXT_CAP before it launches; 0 = launched, 1 = the launch failed.
#include "../../deepcharuco_amd/csrc/dcx_calib_dev.h"      // brings the four block headers and dcx_lm_dev.h (kLmThreads)

#define DCXT_CAP 65536

namespace {

constexpr int kBlock = 64;

__device__ __forceinline__ PnpCamera pinhole_of(const double* c) {
    PnpCamera cam;
    cam.fx = c[0]; cam.fy = c[1]; cam.cx = c[2]; cam.cy = c[3];
    for (int i = 0; i < 8; ++i) cam.k[i] = c[4 + i];
    return cam;
}

__device__ __forceinline__ FisheyeCamera fisheye_of(const double* c) {
    FisheyeCamera cam;
    cam.fx = c[0]; cam.fy = c[1]; cam.cx = c[2]; cam.cy = c[3];
    for (int i = 0; i < 4; ++i) cam.k[i] = c[4 + i];
    return cam;
}

template <class C> struct CamOf;
template <> struct CamOf<PnpCamera> { static __device__ __forceinline__ PnpCamera get(const double* c) { return pinhole_of(c); } };
template <> struct CamOf<FisheyeCamera> { static __device__ __forceinline__ FisheyeCamera get(const double* c) { return fisheye_of(c); } };

inline int launched() { return hipGetLastError() == hipSuccess ? 0 : 1; }

}  // namespace

// ------------------------------------------------------------------------------------------------ per-lane blocks
// LANE(name, NIN, NIIN, NOUT, NIOUT) { body }: a, ia = this instance's inputs, o, io = its outputs

#define LANE(name, NIN, NIIN, NOUT, NIOUT)                                                                                       \
    __device__ __forceinline__ void name##_body(const double* a, const int32_t* ia, double* o, int32_t* io);                       \
    __global__ __launch_bounds__(kBlock) void name##_kernel(const double* in, const int32_t* iin, double* out, int32_t* iout,     \
                                                            int n) {                                                               \
        const int i = blockIdx.x * kBlock + threadIdx.x;                                                                           \
        if (i >= n) return;                                                                                                        \
        name##_body(in + (long long)i * NIN, iin + (long long)i * NIIN, out + (long long)i * NOUT, iout + (long long)i * NIOUT);   \
    }                                                                                                                              \
    extern "C" int dcxt_##name(const double* in, const int32_t* iin, double* out, int32_t* iout, int n, hipStream_t stream) {      \
        if (!in || !iin || !out || !iout || n <= 0 || n > DCXT_CAP) return -1;                                                     \
        name##_kernel<<<dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream>>>(in, iin, out, iout, n);            \
        return launched();                                                                                                         \
    }                                                                                                                              \
    __device__ __forceinline__ void name##_body(const double* a, const int32_t* ia, double* o, int32_t* io)

LANE(rodrigues, 3, 1, 9, 1) {
    double r[3] = {a[0], a[1], a[2]}, R[9];
    rodrigues(r, R);
    for (int i = 0; i < 9; ++i) o[i] = R[i];
}

LANE(rvec_of, 9, 1, 3, 1) {
    double R[9], r[3];
    for (int i = 0; i < 9; ++i) R[i] = a[i];
    rvec_of(R, r);
    for (int i = 0; i < 3; ++i) o[i] = r[i];
}

LANE(right_jacobian, 3, 1, 9, 1) {
    double r[3] = {a[0], a[1], a[2]}, J[9];
    right_jacobian(r, J);
    for (int i = 0; i < 9; ++i) o[i] = J[i];
}

// p (3) -> R (9), G[0] (9), G[1] (9)
LANE(pose_basis, 3, 1, 27, 1) {
    double p[3] = {a[0], a[1], a[2]}, R[9], G[2][9];
    pose_basis(p, R, G);
    for (int i = 0; i < 9; ++i) { o[i] = R[i]; o[9 + i] = G[0][i]; o[18 + i] = G[1][i]; }
}

// du (3), dv (3), mx, my, G (18) -> ju (6), jv (6)
LANE(pose_columns, 26, 1, 12, 1) {
    double du[3], dv[3], G[2][9], ju[6], jv[6];
    for (int i = 0; i < 3; ++i) { du[i] = a[i]; dv[i] = a[3 + i]; }
    for (int i = 0; i < 9; ++i) { G[0][i] = a[8 + i]; G[1][i] = a[17 + i]; }
    pose_columns(du, dv, a[6], a[7], G, ju, jv);
    for (int i = 0; i < 6; ++i) { o[i] = ju[i]; o[6 + i] = jv[i]; }
}

// k (8), x, y -> xd, yd, a, b, d
LANE(distort, 10, 1, 5, 1) {
    double k[8], xd, yd, da, db, dd;
    for (int i = 0; i < 8; ++i) k[i] = a[i];
    distort<true>(k, a[8], a[9], xd, yd, da, db, dd);
    o[0] = xd; o[1] = yd; o[2] = da; o[3] = db; o[4] = dd;
}

// camera (12), q (3), u, v -> ok; ru, rv, du (3), dv (3), x, y, xd, yd
LANE(project, 17, 1, 12, 1) {
    const PnpCamera cam = pinhole_of(a);
    double q[3] = {a[12], a[13], a[14]}, ru, rv, du[3], dv[3], x, y, xd, yd;
    const bool ok = project<true>(cam, q, a[15], a[16], ru, rv, du, dv, x, y, xd, yd);
    io[0] = ok;
    if (!ok) return;
    o[0] = ru; o[1] = rv;
    for (int i = 0; i < 3; ++i) { o[2 + i] = du[i]; o[5 + i] = dv[i]; }
    o[8] = x; o[9] = y; o[10] = xd; o[11] = yd;
}

// the same without the derivative -> ok; ru, rv
LANE(project_nojac, 17, 1, 2, 1) {
    const PnpCamera cam = pinhole_of(a);
    double q[3] = {a[12], a[13], a[14]}, ru, rv;
    const bool ok = project<false>(cam, q, a[15], a[16], ru, rv, nullptr, nullptr);
    io[0] = ok;
    if (!ok) return;
    o[0] = ru; o[1] = rv;
}

// camera (12), u, v -> x, y
LANE(undistort, 14, 1, 2, 1) {
    const PnpCamera cam = pinhole_of(a);
    double x, y;
    undistort(cam, has_distortion(cam), a[12], a[13], x, y);
    o[0] = x; o[1] = y;
}

// k (4), a, b -> xd, yd, tt, t2, dxa, dxb, dyb
LANE(fisheye_distort, 6, 1, 7, 1) {
    double k[4] = {a[0], a[1], a[2], a[3]}, xd, yd, tt, t2, dxa, dxb, dyb;
    fisheye_distort<true>(k, a[4], a[5], xd, yd, tt, t2, dxa, dxb, dyb);
    o[0] = xd; o[1] = yd; o[2] = tt; o[3] = t2; o[4] = dxa; o[5] = dxb; o[6] = dyb;
}

// camera (8), q (3), u, v -> ok; ru, rv, du (3), dv (3), a, b, xd, yd, tt, t2
LANE(fisheye_project, 13, 1, 14, 1) {
    const FisheyeCamera cam = fisheye_of(a);
    double q[3] = {a[8], a[9], a[10]}, ru, rv, du[3], dv[3], na, nb, xd, yd, tt, t2;
    const bool ok = project<true>(cam, q, a[11], a[12], ru, rv, du, dv, na, nb, xd, yd, tt, t2);
    io[0] = ok;
    if (!ok) return;
    o[0] = ru; o[1] = rv;
    for (int i = 0; i < 3; ++i) { o[2 + i] = du[i]; o[5 + i] = dv[i]; }
    o[8] = na; o[9] = nb; o[10] = xd; o[11] = yd; o[12] = tt; o[13] = t2;
}

LANE(fisheye_project_nojac, 13, 1, 2, 1) {
    const FisheyeCamera cam = fisheye_of(a);
    double q[3] = {a[8], a[9], a[10]}, ru, rv;
    const bool ok = project<false>(cam, q, a[11], a[12], ru, rv, nullptr, nullptr);
    io[0] = ok;
    if (!ok) return;
    o[0] = ru; o[1] = rv;
}

// camera (8), u, v -> inside; x, y
LANE(fisheye_undistort, 10, 1, 2, 1) {
    const FisheyeCamera cam = fisheye_of(a);
    double x, y;
    io[0] = undistort(cam, a[8], a[9], x, y);
    o[0] = x; o[1] = y;
}

// packed 3x3 (6) -> the rotated packed matrix (6), V row major (9); V starts as the identity, as polar_factor() starts it
LANE(jacobi3, 6, 1, 15, 1) {
    double s[6], v[3][3];
    for (int i = 0; i < 6; ++i) s[i] = a[i];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) v[i][j] = i == j ? 1.0 : 0.0;
    jacobi<3, 3>(s, v);
    for (int i = 0; i < 6; ++i) o[i] = s[i];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) o[6 + i * 3 + j] = v[i][j];
}

LANE(polar_factor, 9, 1, 9, 1) {
    double M[9], Q[9];
    for (int i = 0; i < 9; ++i) M[i] = a[i];
    const bool ok = polar_factor(M, Q);
    io[0] = ok;
    if (!ok) return;
    for (int i = 0; i < 9; ++i) o[i] = Q[i];
}

// packed 6x6 (21), scale -> ok; L (21)
LANE(cholesky_factor, 22, 1, 21, 1) {
    double m[21], L[21];
    for (int i = 0; i < 21; ++i) { m[i] = a[i]; L[i] = 0.0; }
    const bool ok = cholesky_factor<6>(m, a[21], L);
    io[0] = ok;
    if (!ok) return;
    for (int i = 0; i < 21; ++i) o[i] = L[i];
}

// L (21), rhs (6) -> x (6)
LANE(cholesky_substitute, 27, 1, 6, 1) {
    double L[21], rhs[6], x[6];
    for (int i = 0; i < 21; ++i) L[i] = a[i];
    for (int i = 0; i < 6; ++i) rhs[i] = a[21 + i];
    cholesky_substitute<6>(L, rhs, x);
    for (int i = 0; i < 6; ++i) o[i] = x[i];
}

// packed 6x6 (21), rhs (6), scale -> ok; x (6)
LANE(cholesky_solve, 28, 1, 6, 1) {
    double m[21], rhs[6], x[6];
    for (int i = 0; i < 21; ++i) m[i] = a[i];
    for (int i = 0; i < 6; ++i) rhs[i] = a[21 + i];
    const bool ok = cholesky_solve(m, rhs, a[27], x);
    io[0] = ok;
    if (!ok) return;
    for (int i = 0; i < 6; ++i) o[i] = x[i];
}

LANE(adjugate, 9, 1, 9, 1) {
    double m[9], r[9];
    for (int i = 0; i < 9; ++i) m[i] = a[i];
    adjugate(m, r);
    for (int i = 0; i < 9; ++i) o[i] = r[i];
}

// x (4), y (4) -> A (9)
LANE(projective_basis, 8, 1, 9, 1) {
    double x[4], y[4], A[9];
    for (int i = 0; i < 4; ++i) { x[i] = a[i]; y[i] = a[4 + i]; }
    projective_basis(x, y, A);
    for (int i = 0; i < 9; ++i) o[i] = A[i];
}

// Sample: mx (4), my (4), x (4), y (4) -> status; H (9), mcx, mcy
LANE(homography4, 16, 1, 11, 1) {
    Sample q;
    for (int i = 0; i < 4; ++i) { q.mx[i] = a[i]; q.my[i] = a[4 + i]; q.x[i] = a[8 + i]; q.y[i] = a[12 + i]; }
    double H[9], mcx, mcy;
    const int st = homography(q, identity_camera(), false, H, mcx, mcy);
    io[0] = st;
    if (st != DCX_PNP_OK) return;
    for (int i = 0; i < 9; ++i) o[i] = H[i];
    o[9] = mcx; o[10] = mcy;
}

// Sample -> status; p0 (6): init_pose() through the four-point homography
LANE(init_pose4, 16, 1, 6, 1) {
    Sample q;
    for (int i = 0; i < 4; ++i) { q.mx[i] = a[i]; q.my[i] = a[4 + i]; q.x[i] = a[8 + i]; q.y[i] = a[12 + i]; }
    double p0[6];
    const int st = init_pose(q, identity_camera(), false, p0);
    io[0] = st;
    if (st != DCX_PNP_OK) return;
    for (int i = 0; i < 6; ++i) o[i] = p0[i];
}

// x -> mix32(x)
LANE(mix32, 1, 1, 1, 1) { io[0] = (int32_t)mix32((uint32_t)ia[0]); }

// seed, n, h, c -> slot
LANE(ransac_draw, 1, 4, 1, 1) { io[0] = ransac_draw((uint32_t)ia[0], (uint32_t)ia[1], (uint32_t)ia[2], (uint32_t)ia[3]); }

// gx (4), gy (4), a, b, c -> on a line?
LANE(on_a_line, 1, 11, 1, 1) {
    int gx[4], gy[4];
    for (int i = 0; i < 4; ++i) { gx[i] = ia[i]; gy[i] = ia[4 + i]; }
    io[0] = on_a_line(gx, gy, ia[8], ia[9], ia[10]);
}

// e -> (row, column) by unpk<N> for every N in use: 6, 8, 9, 13, 15, 16; -1, -1 where e is past the end of that N
template <int N>
__device__ __forceinline__ void unpk_out(int e, int32_t* io) {
    io[0] = io[1] = -1;
    if (e < 0 || e >= N * (N + 1) / 2) return;
    int r, c;
    unpk<N>(e, r, c);
    io[0] = r; io[1] = c;
}
LANE(unpk, 1, 1, 1, 12) {
    unpk_out<6>(ia[0], io); unpk_out<8>(ia[0], io + 2); unpk_out<9>(ia[0], io + 4);
    unpk_out<13>(ia[0], io + 6); unpk_out<15>(ia[0], io + 8); unpk_out<16>(ia[0], io + 10);
}

// i, j -> pk<N>(i, j) for the same N; -1 where i or j is outside
template <int N>
__device__ __forceinline__ int pk_out(int i, int j) { return (i < 0 || j < 0 || i >= N || j >= N) ? -1 : pk<N>(i, j); }
LANE(pk, 1, 2, 1, 6) {
    io[0] = pk_out<6>(ia[0], ia[1]); io[1] = pk_out<8>(ia[0], ia[1]); io[2] = pk_out<9>(ia[0], ia[1]);
    io[3] = pk_out<13>(ia[0], ia[1]); io[4] = pk_out<15>(ia[0], ia[1]); io[5] = pk_out<16>(ia[0], ia[1]);
}

// ransac_sample over a shared id table: seed, n, h, rm1 -> ok, s (4).  rows = (x, y, id, cell) per slot, n_rows of them; an
// instance whose n is outside [4, n_rows] is not run (ok = -1): the sampler reads rows[4 * slot + 2] for slot < n.
__global__ __launch_bounds__(kBlock) void ransac_sample_kernel(const int32_t* rows, int n_rows, const int32_t* iin, int32_t* iout, int n) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int32_t* ia = iin + (long long)i * 4;
    int32_t* io = iout + (long long)i * 5;
    if (ia[1] < 4 || ia[1] > n_rows || ia[3] < 1) { io[0] = -1; return; }
    int s[4] = {-1, -1, -1, -1};
    io[0] = ransac_sample(rows, (uint32_t)ia[0], ia[1], ia[2], ia[3], s);
    for (int k = 0; k < 4; ++k) io[1 + k] = s[k];
}
extern "C" int dcxt_ransac_sample(const int32_t* rows, int n_rows, const int32_t* iin, int32_t* iout, int n, hipStream_t stream) {
    if (!rows || !iin || !iout || n_rows <= 0 || n <= 0 || n > DCXT_CAP) return -1;
    ransac_sample_kernel<<<dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream>>>(rows, n_rows, iin, iout, n);
    return launched();
}

// ------------------------------------------------------------------------------------------------ wave-wide blocks
// WAVE(name, NIN, NIIN, NOUT, NIOUT) { body }: one 64-lane workgroup per instance b; a, ia = the instance's inputs (shared by its
// lanes), o, io = THIS LANE's outputs

#define WAVE(name, NIN, NIIN, NOUT, NIOUT)                                                                                       \
    __device__ __forceinline__ void name##_body(const double* a, const int32_t* ia, double* o, int32_t* io, int lane);             \
    __global__ __launch_bounds__(kLanes) void name##_kernel(const double* in, const int32_t* iin, double* out, int32_t* iout) {    \
        const long long b = blockIdx.x, l = b * kLanes + threadIdx.x;                                                              \
        name##_body(in + b * NIN, iin + b * NIIN, out + l * NOUT, iout + l * NIOUT, (int)threadIdx.x);                             \
    }                                                                                                                              \
    extern "C" int dcxt_##name(const double* in, const int32_t* iin, double* out, int32_t* iout, int n, hipStream_t stream) {      \
        if (!in || !iin || !out || !iout || n <= 0 || n > DCXT_CAP) return -1;                                                     \
        name##_kernel<<<dim3((unsigned)n), dim3(kLanes), 0, stream>>>(in, iin, out, iout);                                         \
        return launched();                                                                                                         \
    }                                                                                                                              \
    __device__ __forceinline__ void name##_body(const double* a, const int32_t* ia, double* o, int32_t* io, int lane)

// 64 lanes x 5 values -> every lane's 5 sums (homography()'s second pass)
WAVE(wave_sum5, 64 * 5, 1, 5, 1) {
    double v[5];
    for (int i = 0; i < 5; ++i) v[i] = a[lane * 5 + i];
    wave_sum(v);
    for (int i = 0; i < 5; ++i) o[i] = v[i];
}

// 64 lanes x 28 values (evaluate()'s accumulator)
WAVE(wave_sum28, 64 * 28, 1, 28, 1) {
    double v[28];
    for (int i = 0; i < 28; ++i) v[i] = a[lane * 28 + i];
    wave_sum(v);
    for (int i = 0; i < 28; ++i) o[i] = v[i];
}

// mask (64 ints), count -> this lane's place, the count after
WAVE(append_kept, 1, 65, 1, 2) {
    int count = ia[64];
    io[0] = append_kept(ia[lane] != 0, lane, count);
    io[1] = count;
}

// packed 9x9 (45) -> this lane's copy of the rotated matrix (45) and its row of V (9): homography()'s use, rows >= 9 start at zero
WAVE(jacobi9, 45, 1, 54, 1) {
    double M[45], vrow[1][9];
    for (int i = 0; i < 45; ++i) M[i] = a[i];
    for (int c = 0; c < 9; ++c) vrow[0][c] = (c == lane) ? 1.0 : 0.0;
    jacobi<9, 1>(M, vrow);
    for (int i = 0; i < 45; ++i) o[i] = M[i];
    for (int c = 0; c < 9; ++c) o[45 + c] = vrow[0][c];
}

// scores of every instance in one table, `stride` apart; an instance's iterations in [1, stride] or it is not run (best = -2)
__global__ __launch_bounds__(kLanes) void best_hypothesis_kernel(const int32_t* scores, int stride, const int32_t* iterations, int32_t* iout) {
    const long long b = blockIdx.x, l = b * kLanes + threadIdx.x;
    const int it = iterations[b];
    if (it < 1 || it > stride) { iout[2 * l] = -2; return; }
    int best, bh;
    best_hypothesis(scores + b * stride, it, best, bh);
    iout[2 * l] = best;
    iout[2 * l + 1] = bh;
}
extern "C" int dcxt_best_hypothesis(const int32_t* scores, int stride, const int32_t* iterations, int32_t* iout, int n, hipStream_t stream) {
    if (!scores || !iterations || !iout || stride <= 0 || n <= 0 || n > DCXT_CAP) return -1;
    best_hypothesis_kernel<<<dim3((unsigned)n), dim3(kLanes), 0, stream>>>(scores, stride, iterations, iout);
    return launched();
}

// block_tree at the two shapes in use: THREADS x NV partials per instance -> the NV totals (s[0][..])
template <int THREADS, int NV>
__global__ __launch_bounds__(THREADS) void block_tree_kernel(const double* in, double* out) {
    __shared__ double s[THREADS][NV];
    const long long b = blockIdx.x;
    const int t = threadIdx.x;
    for (int j = 0; j < NV; ++j) s[t][j] = in[(b * THREADS + t) * NV + j];
    block_tree<THREADS, NV>(s);
    if (t < NV) out[b * NV + t] = s[0][t];
}
extern "C" int dcxt_block_tree6(const double* in, double* out, int n, hipStream_t stream) {
    if (!in || !out || n <= 0 || n > DCXT_CAP) return -1;
    block_tree_kernel<kLmThreads, 6><<<dim3((unsigned)n), dim3(kLmThreads), 0, stream>>>(in, out);
    return launched();
}
extern "C" int dcxt_block_tree7(const double* in, double* out, int n, hipStream_t stream) {
    if (!in || !out || n <= 0 || n > DCXT_CAP) return -1;
    block_tree_kernel<kRedThreads, 7><<<dim3((unsigned)n), dim3(kRedThreads), 0, stream>>>(in, out);
    return launched();
}
extern "C" int dcxt_block_tree_threads() { return kLmThreads; }

// ---- the joint solves' per-view steps

// accumulate_rows<13, 2, 13> and lane_entries<13, 2> (the stereo and rig solves' shape; 13 = dcx_stereo_dev.h's kLdsStride, which
// cannot be included beside dcx_calib_dev.h's constant of the same name).  rows: n x (ju[13], jv[13]); front: n ints, 0 = the row
// is behind the camera.  Instance b owns rows starts[b] .. starts[b] + counts[b], checked against n_rows.
// -> per lane: acc (2), and ea (2), eb (2), behind
__global__ __launch_bounds__(kLanes) void accumulate_rows_kernel(const double* rows, const int32_t* front, int n_rows, const int32_t* counts,
                                                                 const int32_t* starts, double* out, int32_t* iout) {
    __shared__ double sj[2 * kLanes][13];
    const long long b = blockIdx.x, l = b * kLanes + threadIdx.x;
    const int lane = threadIdx.x, n = counts[b], s0 = starts[b];
    if (n < 0 || s0 < 0 || (long long)s0 + n > n_rows) { iout[5 * l + 4] = -1; return; }
    int ea[2], eb[2];
    lane_entries<13, 2>(lane, ea, eb);
    double acc[2] = {0.0, 0.0};
    bool behind = false;
    const double* base = rows + (long long)s0 * 26;
    const int32_t* fr = front + s0;
    accumulate_rows<13, 2, 13>(n, [&](int i, double* ju, double* jv) {
        for (int j = 0; j < 13; ++j) { ju[j] = base[(long long)i * 26 + j]; jv[j] = base[(long long)i * 26 + 13 + j]; }
        return fr[i] != 0;
    }, sj, ea, eb, acc, behind);
    out[2 * l] = acc[0]; out[2 * l + 1] = acc[1];
    iout[5 * l] = ea[0]; iout[5 * l + 1] = ea[1]; iout[5 * l + 2] = eb[0]; iout[5 * l + 3] = eb[1]; iout[5 * l + 4] = behind;
}
extern "C" int dcxt_accumulate_rows(const double* rows, const int32_t* front, int n_rows, const int32_t* counts, const int32_t* starts,
                                    double* out, int32_t* iout, int n, hipStream_t stream) {
    if (!rows || !front || !counts || !starts || !out || !iout || n_rows <= 0 || n <= 0 || n > DCXT_CAP) return -1;
    accumulate_rows_kernel<<<dim3((unsigned)n), dim3(kLanes), 0, stream>>>(rows, front, n_rows, counts, starts, out, iout);
    return launched();
}

// schur_view<NA>: m (packed NC x NC, NC = NA + 7), scale -> sc (NS + NA, written by its lanes), yz (6 NA + 6), this lane's verdict
template <int NA>
__global__ __launch_bounds__(kLanes) void schur_view_kernel(const double* m, const double* scale, double* sc, double* yz, int32_t* iout) {
    constexpr int NC = NA + 7, kEntries = NC * (NC + 1) / 2, kSC = NA * (NA + 1) / 2 + NA, kYZ = 6 * NA + 6;
    __shared__ double sy[NA + 1][6];
    const long long b = blockIdx.x;
    const int lane = threadIdx.x;
    iout[b * kLanes + lane] = schur_view<NA>(m + b * kEntries, scale[b], lane, sy, yz + b * kYZ, sc + b * kSC);
}
#define SCHUR(NA)                                                                                                                 \
    extern "C" int dcxt_schur_view##NA(const double* m, const double* scale, double* sc, double* yz, int32_t* iout, int n,        \
                                       hipStream_t stream) {                                                                      \
        if (!m || !scale || !sc || !yz || !iout || n <= 0 || n > DCXT_CAP) return -1;                                             \
        schur_view_kernel<NA><<<dim3((unsigned)n), dim3(kLanes), 0, stream>>>(m, scale, sc, yz, iout);                            \
        return launched();                                                                                                        \
    }
SCHUR(6)
SCHUR(8)
SCHUR(9)

// ---- blocks over frames of a corner pool.  The pool is the library's CornerPool; camera = fx fy cx cy k[8] (pinhole) or k[4]
// (fisheye), shared by the instances; instance b is frame b.  A frame is run only if its slots lie inside the pool, it has at
// least one row and its ids are inside the board (else status -100 and nothing else written): the blocks read without checking,
// as in the library, where frame_status() has gone before them.

namespace {

struct PoolArgs {
    CornerPool pl;
    int batch;
};

__device__ __forceinline__ bool frame_readable(const CornerPool& pl, int b) {
    const long long n = pl.counts[b], s0 = pl.starts[b];
    if (n < 1 || s0 < 0 || s0 + n > (long long)pl.pool) return false;
    bool bad = false;
    for (long long i = threadIdx.x; i < n; i += kLanes) {
        const int id = pl.rows[4 * (s0 + i) + 2];
        bad |= id < 0 || id >= pl.n_ids;
    }
    return !__any(bad);
}

inline bool pool_args(const int32_t* counts, const int32_t* starts, const int32_t* rows, const float* xy, int batch, int pool, int col_count,
                      int row_count, double square_len, PoolArgs& pa) {
    pa.batch = batch;
    return batch <= DCXT_CAP && corner_pool(counts, starts, rows, xy, batch, pool, col_count, row_count, square_len, pa.pl);
}

}  // namespace

#define POOL_PARAMS const int32_t *counts, const int32_t *starts, const int32_t *rows, const float *xy, int batch, int pool,      \
                    int col_count, int row_count, double square_len
#define POOL_ARGS counts, starts, rows, xy, batch, pool, col_count, row_count, square_len

// frame_status and ranges_overlap -> per lane: status, n, s0, overlap
__global__ __launch_bounds__(kLanes) void frame_checks_kernel(PoolArgs pa, int32_t* iout) {
    const int b = blockIdx.x;
    int32_t* io = iout + ((long long)b * kLanes + threadIdx.x) * 4;
    int n, s0;
    io[0] = frame_status(pa.pl, b, n, s0);
    io[1] = n;
    io[2] = s0;
    io[3] = ranges_overlap(pa.pl, pa.batch, b);
}
extern "C" int dcxt_frame_checks(POOL_PARAMS, int32_t* iout, hipStream_t stream) {
    PoolArgs pa;
    if (!iout || !pool_args(POOL_ARGS, pa)) return -1;
    frame_checks_kernel<<<dim3((unsigned)batch), dim3(kLanes), 0, stream>>>(pa, iout);
    return launched();
}

// per frame b, at the pose in[b * 6 ..]: evaluate<true> -> acc (28) per lane; evaluate<false> -> cost per lane; and the frame's
// homography (status; H, mcx, mcy), init_pose (status; p0), solve (status; pose[8]), points_inside
// out per lane: acc[28] | cost | H[9] mcx mcy | p0[6] | pose[8] = 54;  iout per lane: readable, st_H, st_init, st_solve, inside
template <class C>
__global__ __launch_bounds__(kLanes) void frame_blocks_kernel(PoolArgs pa, const double* camera, const double* in, double* out, int32_t* iout) {
    const int b = blockIdx.x;
    double* o = out + ((long long)b * kLanes + threadIdx.x) * 54;
    int32_t* io = iout + ((long long)b * kLanes + threadIdx.x) * 5;
    if (!frame_readable(pa.pl, b)) { io[0] = -100; return; }
    io[0] = 1;
    const Frame f = pa.pl.frame(b);
    const C cam = CamOf<C>::get(camera);
    double p[6], acc[28];
    for (int i = 0; i < 6; ++i) p[i] = in[(long long)b * 6 + i];
    evaluate<true>(f, cam, p, acc);
    for (int i = 0; i < 28; ++i) o[i] = acc[i];
    evaluate<false>(f, cam, p, acc);
    o[28] = acc[0];
    io[4] = points_inside(f, cam);
    if (!io[4]) return;                     // the library's solve() stops here too: undistort() would leave NaN
    double H[9], mcx, mcy;
    io[1] = homography(f, cam, has_distortion(cam), H, mcx, mcy);
    if (io[1] == DCX_PNP_OK) {
        for (int i = 0; i < 9; ++i) o[29 + i] = H[i];
        o[38] = mcx; o[39] = mcy;
    }
    double p0[6];
    io[2] = init_pose(f, cam, has_distortion(cam), p0);
    if (io[2] == DCX_PNP_OK)
        for (int i = 0; i < 6; ++i) o[40 + i] = p0[i];
    double pose[8];
    io[3] = solve(f, cam, pose);
    if (io[3] == DCX_PNP_OK)
        for (int i = 0; i < 8; ++i) o[46 + i] = pose[i];
}
#define FRAME_BLOCKS(name, C)                                                                                                     \
    extern "C" int dcxt_frame_blocks_##name(POOL_PARAMS, const double* camera, const double* in, double* out, int32_t* iout,      \
                                            hipStream_t stream) {                                                                 \
        PoolArgs pa;                                                                                                              \
        if (!camera || !in || !out || !iout || !pool_args(POOL_ARGS, pa)) return -1;                                              \
        frame_blocks_kernel<C><<<dim3((unsigned)batch), dim3(kLanes), 0, stream>>>(pa, camera, in, out, iout);                    \
        return launched();                                                                                                        \
    }
FRAME_BLOCKS(pinhole, PnpCamera)
FRAME_BLOCKS(fisheye, FisheyeCamera)

extern "C" int dcxt_cap() { return DCXT_CAP; }
