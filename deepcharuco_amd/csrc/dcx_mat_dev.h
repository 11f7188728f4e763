// dcx_mat_dev.h -- the small fp64 matrix steps and fixed-order reductions of the pose and calibration kernels, one copy each:
// packed symmetric storage (pk, unpk), the wave butterfly, the one-workgroup tree, the ballot compaction, cyclic Jacobi, the polar
// factor, the packed Cholesky (factor, substitute, both), the 3x3 adjugate, and what the joint solves (dcx_calib_dev.h,
// dcx_stereo.hip) run per view: the LDS-staged Gram accumulation of [J | r] and the view's Schur part.  Also the workspace carver of
// their hosts.  No camera and no pool in here: those are dcx_camera_dev.h and dcx_pnp_dev.h.
// Everything is force-inlined and has internal linkage, so each translation unit compiles its own copy.
#pragma once
#include "dcx_common.h"

#include <math.h>

namespace {

constexpr int kLanes = 64;
constexpr int kJacobiMaxSweeps = 16;

// packed upper triangle of a symmetric N x N matrix, row major
template <int N>
__device__ constexpr int pk(int i, int j) {
    return i <= j ? i * N - i * (i - 1) / 2 + (j - i) : j * N - j * (j - 1) / 2 + (i - j);
}

// the inverse: packed index e -> its row a and column b >= a
template <int N>
__device__ __forceinline__ void unpk(int e, int& a, int& b) {
    int r = 0, first = 0;
    while (first + (N - r) <= e) { first += N - r; ++r; }
    a = r;
    b = r + (e - first);
}

template <int N>
__device__ __forceinline__ void wave_sum(double (&a)[N]) {
#pragma unroll
    for (int m = kLanes / 2; m >= 1; m >>= 1) {
#pragma unroll
        for (int i = 0; i < N; ++i) a[i] += __shfl_xor(a[i], m, kLanes);
    }
}

// Fixed-order tree over the THREADS partials in s (LDS), NV values per thread; the totals end in s[0][0..NV).
template <int THREADS, int NV>
__device__ __forceinline__ void block_tree(double (*s)[NV]) {
    const int t = threadIdx.x;
    for (int h = THREADS / 2; h >= 1; h >>= 1) {
        __syncthreads();
        if (t < h) {
#pragma unroll
            for (int j = 0; j < NV; ++j) s[t][j] += s[t + h][j];
        }
    }
    __syncthreads();
}

// Ordered compaction, 64 candidates at a time: the lanes with `in` take consecutive places from `count` on, in lane order.
// -> this lane's place (meaningful where `in`); count moves past the kept ones.  Wave-wide.
__device__ __forceinline__ int append_kept(bool in, int lane, int& count) {
    const unsigned long long m = __ballot(in);
    const int at = count + __popcll(m & ((1ull << lane) - 1ull));
    count += __popcll(m);
    return at;
}

// Cyclic Jacobi on the packed symmetric a (eigenvalues end on its diagonal).  v holds NR rows of V (a = V diag V^T); the caller
// initialises them.  Same rotation formulas and order as pnp._jacobi.
template <int N, int NR>
__device__ __forceinline__ void jacobi(double (&a)[N * (N + 1) / 2], double (&v)[NR][N]) {
#pragma unroll 1
    for (int sweep = 0; sweep < kJacobiMaxSweeps; ++sweep) {
        double off = 0.0, dia = 0.0;
#pragma unroll
        for (int p = 0; p < N; ++p) {
            dia += a[pk<N>(p, p)] * a[pk<N>(p, p)];
#pragma unroll
            for (int q = p + 1; q < N; ++q) off += a[pk<N>(p, q)] * a[pk<N>(p, q)];
        }
        if (!(off > 1e-30 * dia)) break;
#pragma unroll
        for (int p = 0; p < N; ++p) {
#pragma unroll
            for (int q = p + 1; q < N; ++q) {
                const double apq = a[pk<N>(p, q)], app = a[pk<N>(p, p)], aqq = a[pk<N>(q, q)];
                double t = 0.0;
                if (apq != 0.0) {
                    const double theta = (aqq - app) / (2.0 * apq);
                    t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                    if (theta < 0) t = -t;
                }
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                // columns p, q, then rows p, q (the 2x2 block in two steps, as the host does on the full matrix)
                const double bpp = c * app - s * apq, bpq = s * app + c * apq;
                const double bqp = c * apq - s * aqq, bqq = s * apq + c * aqq;
#pragma unroll
                for (int r = 0; r < N; ++r) {
                    if (r == p || r == q) continue;
                    const double arp = a[pk<N>(r, p)], arq = a[pk<N>(r, q)];
                    a[pk<N>(r, p)] = c * arp - s * arq;
                    a[pk<N>(r, q)] = s * arp + c * arq;
                }
                a[pk<N>(p, p)] = c * bpp - s * bqp;
                a[pk<N>(q, q)] = s * bpq + c * bqq;
                a[pk<N>(p, q)] = 0.0;
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    const double vp = v[r][p], vq = v[r][q];
                    v[r][p] = c * vp - s * vq;
                    v[r][q] = s * vp + c * vq;
                }
            }
        }
    }
}

// polar factor Q = M (M^T M)^-1/2 of a row-major 3x3 by the 3x3 Jacobi; false if M^T M has a non-positive eigenvalue
__device__ __forceinline__ bool polar_factor(const double* M, double* Q) {
    double S[6], W[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) S[pk<3>(a, b)] = M[a] * M[b] + M[3 + a] * M[3 + b] + M[6 + a] * M[6 + b];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) W[a][b] = a == b ? 1.0 : 0.0;
    jacobi<3, 3>(S, W);
    double iw[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double w = S[pk<3>(c, c)];
        if (!(w > 0)) return false;
        iw[c] = 1.0 / sqrt(w);
    }
    double P[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) P[a * 3 + b] = W[a][0] * iw[0] * W[b][0] + W[a][1] * iw[1] * W[b][1] + W[a][2] * iw[2] * W[b][2];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) Q[a * 3 + b] = M[a * 3 + 0] * P[b] + M[a * 3 + 1] * P[3 + b] + M[a * 3 + 2] * P[6 + b];
    return true;
}

// Cholesky of the packed symmetric N x N a with its diagonal scaled by `scale` -> L (packed); false if not positive definite
template <int N>
__device__ __forceinline__ bool cholesky_factor(const double* a, double scale, double* L) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double s = a[pk<N>(i, j)] * (i == j ? scale : 1.0);
#pragma unroll
            for (int k = 0; k < j; ++k) s -= L[pk<N>(i, k)] * L[pk<N>(j, k)];
            if (i == j) {
                if (!(s > 0)) return false;
                L[pk<N>(i, i)] = sqrt(s);
            } else {
                L[pk<N>(i, j)] = s / L[pk<N>(j, j)];
            }
        }
    }
    return true;
}

// L L^T x = rhs by the two substitutions
template <int N>
__device__ __forceinline__ void cholesky_substitute(const double* L, const double* rhs, double* x) {
    double y[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double s = rhs[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= L[pk<N>(i, k)] * y[k];
        y[i] = s / L[pk<N>(i, i)];
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < N; ++k) s -= L[pk<N>(k, i)] * x[k];
        x[i] = s / L[pk<N>(i, i)];
    }
}

// (the 6x6 JtJ with its diagonal scaled by 1 + lambda) x = Jtr by Cholesky; false if not positive definite
__device__ __forceinline__ bool cholesky_solve(const double* jtj, const double* jtr, double scale, double* x) {
    double L[21];
    if (!cholesky_factor<6>(jtj, scale, L)) return false;
    cholesky_substitute<6>(L, jtr, x);
    return true;
}

// adjugate of a row-major 3x3
__device__ __forceinline__ void adjugate(const double* m, double* a) {
    a[0] = m[4] * m[8] - m[5] * m[7]; a[1] = m[2] * m[7] - m[1] * m[8]; a[2] = m[1] * m[5] - m[2] * m[4];
    a[3] = m[5] * m[6] - m[3] * m[8]; a[4] = m[0] * m[8] - m[2] * m[6]; a[5] = m[2] * m[3] - m[0] * m[5];
    a[6] = m[3] * m[7] - m[4] * m[6]; a[7] = m[1] * m[6] - m[0] * m[7]; a[8] = m[0] * m[4] - m[1] * m[3];
}

// ---- the joint solves' per-view steps (dcx_calib_dev.h, dcx_stereo.hip).  A view's rows of [J | r] (NC columns, the residual last)
// give a packed symmetric NC x NC; one 64-lane wave per view, lane l owns its entries l, l + 64, ... (NQ of them at the most).

// the entries this lane owns: e = lane + 64 q, (ea, eb) its row and column in the packed NC x NC, -1 past the end
template <int NC, int NQ>
__device__ __forceinline__ void lane_entries(int lane, int* ea, int* eb) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        ea[q] = eb[q] = -1;
        const int e = lane + kLanes * q;
        if (e >= NC * (NC + 1) / 2) continue;
        unpk<NC>(e, ea[q], eb[q]);
    }
}

// n rows added to the lane's entries: 64 rows at a time through LDS (sj, 128 x STRIDE), every lane its entries in row order.
// row_fn(i, ju, jv) fills the u and v lines of row i (zero on entry) and answers whether the point is in front of the camera; a
// row that is not counts as zero and sets `behind`.  Wave-wide.
template <int NC, int NQ, int STRIDE, class RowFn>
__device__ __forceinline__ void accumulate_rows(int n, const RowFn& row_fn, double (*sj)[STRIDE], const int* ea, const int* eb,
                                                double* acc, bool& behind) {
    const int lane = threadIdx.x;
    for (int c0 = 0; c0 < n; c0 += kLanes) {
        const int i = c0 + lane;
        double ju[NC], jv[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) ju[j] = jv[j] = 0.0;
        if (i < n && !row_fn(i, ju, jv)) {
            behind = true;
#pragma unroll
            for (int j = 0; j < NC; ++j) ju[j] = jv[j] = 0.0;
        }
        __syncthreads();                     // the previous chunk's rows have been read
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            sj[2 * lane][j] = ju[j];
            sj[2 * lane + 1][j] = jv[j];
        }
        __syncthreads();
        const int rows = 2 * min(kLanes, n - c0);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            if (ea[q] < 0) continue;
            double s = acc[q];
            for (int r = 0; r < rows; ++r) s += sj[r][ea[q]] * sj[r][eb[q]];
            acc[q] = s;
        }
    }
}

// The view's Schur part.  m is its packed symmetric [V W g_a; W^T U g_b; . . cost] over NA shared parameters, 6 pose parameters
// and the residual.  Every lane factors U* (U, diagonal scaled) itself; lane j < NA solves column j of U*^-1 W^T (rhs = row j of
// W), lane NA solves U*^-1 g_b: both to sy (LDS, NA + 1 rows) and to yz (U*^-1 W^T as 6 x NA row major, then U*^-1 g_b); then the
// lanes < NA (NA + 1) / 2 + NA form sc: W U*^-1 W^T (packed NA x NA), then W U*^-1 g_b (where there are more than 64 of them, the
// lanes take a second one each).  false (sc zeroed) if U* is not positive definite.  Wave-wide.
template <int NA>
__device__ __forceinline__ bool schur_view(const double* m, double scale, int lane, double (*sy)[6], double* yz, double* sc) {
    constexpr int NC = NA + 7, NS = NA * (NA + 1) / 2;
    double u[21], L[21];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) u[pk<6>(i, j)] = m[pk<NC>(NA + i, NA + j)];
    if (!cholesky_factor<6>(u, scale, L)) {
        if (lane < NS + NA) sc[lane] = 0.0;
        if constexpr (NS + NA > kLanes)
            if (lane + kLanes < NS + NA) sc[lane + kLanes] = 0.0;
        return false;
    }
    if (lane < NA + 1) {
        double rhs[6], x[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) rhs[k] = lane < NA ? m[pk<NC>(lane, NA + k)] : m[pk<NC>(NA + k, NC - 1)];
        cholesky_substitute<6>(L, rhs, x);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            sy[lane][k] = x[k];
            if (lane < NA) yz[k * NA + lane] = x[k];
            else yz[6 * NA + k] = x[k];
        }
    }
    __syncthreads();
    if (lane < NS + NA) {
        int a = lane - NS, c = NA;
        if (lane < NS) unpk<NA>(lane, a, c);
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) s += m[pk<NC>(a, NA + k)] * sy[c][k];
        sc[lane] = s;
    }
    if constexpr (NS + NA > kLanes) {        // a second round of entries (NA = 12: 90 of them)
        static_assert(NS + NA <= 2 * kLanes, "rounds");
        const int e = lane + kLanes;
        if (e < NS + NA) {
            int a = e - NS, c = NA;
            if (e < NS) unpk<NA>(e, a, c);
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) s += m[pk<NC>(a, NA + k)] * sy[c][k];
            sc[e] = s;
        }
    }
    return true;
}

// ---- the hosts' workspace carver: parts of a caller's buffer handed out in order, each rounded up to 8 bytes

__host__ __device__ inline size_t up8(size_t n) { return (n + 7) & ~(size_t)7; }

struct Carver {
    char* base;                          // may be null: then only `at`, the bytes needed, means anything
    size_t at;

    template <class T>
    T* take(size_t count) {
        T* q = (T*)(base + at);
        at += up8(count * sizeof(T));
        return q;
    }
};

}  // namespace
