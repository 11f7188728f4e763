// dcx_pnp_dev.h -- the fp64 device steps of the PnP solver (dcx_pnp.hip) that the camera calibration (dcx_calib.hip) reuses:
// packed symmetric storage, the wave butterfly, cyclic Jacobi, Rodrigues both ways, the SO(3) right Jacobian, the pool reader
// (Frame), undistortPoints, the 6x6 Cholesky, the planar DLT homography, the planar pose init and the PnP Levenberg-Marquardt; dcx_pnp_ransac.hip runs the
// last three over an index list of a frame's rows (the frame type is a template parameter).  Also here: what the two consensus
// searches (dcx_pnp_ransac.hip, dcx_calib_ransac.hip) share: the per-frame checks, the sampler, the four-point homography and one
// row's reprojection error.
// deepcharuco_amd/pnp.py restates every step (its functions of the same names).  Everything is force-inlined and has internal
// linkage, so each translation unit compiles its own copy.
#pragma once
#include "dcx_common.h"

#include <math.h>

namespace {

constexpr int kLanes = 64;
constexpr int kLmMaxIter = 20;
constexpr double kLmEps = 1.1920928955078125e-07;   // FLT_EPSILON
constexpr int kUndistortIters = 5;
constexpr int kJacobiMaxSweeps = 16;

struct PnpCamera {
    double fx, fy, cx, cy;
    double k[8];            // k1 k2 p1 p2 k3 k4 k5 k6, zero padded
};

// K (row major, no skew) and 0 / 4 / 5 / 8 distortion coefficients from the host -> the kernel argument; false if refused
inline bool pnp_camera(const double* h_camera9, const double* h_dist, int n_dist, PnpCamera& cam) {
    if (!h_camera9 || !(n_dist == 0 || n_dist == 4 || n_dist == 5 || n_dist == 8) || (n_dist > 0 && !h_dist)) return false;
    if (h_camera9[1] != 0.0) return false;                         // skew is not supported
    cam.fx = h_camera9[0];
    cam.fy = h_camera9[4];
    cam.cx = h_camera9[2];
    cam.cy = h_camera9[5];
    if (!(isfinite(cam.fx) && isfinite(cam.fy) && isfinite(cam.cx) && isfinite(cam.cy)) || cam.fx == 0.0 || cam.fy == 0.0)
        return false;
    for (int i = 0; i < 8; ++i) {
        cam.k[i] = i < n_dist ? h_dist[i] : 0.0;
        if (!isfinite(cam.k[i])) return false;
    }
    return true;
}

// packed upper triangle of a symmetric N x N matrix, row major
template <int N>
__device__ constexpr int pk(int i, int j) {
    return i <= j ? i * N - i * (i - 1) / 2 + (j - i) : j * N - j * (j - 1) / 2 + (i - j);
}

template <int N>
__device__ __forceinline__ void wave_sum(double (&a)[N]) {
#pragma unroll
    for (int m = kLanes / 2; m >= 1; m >>= 1) {
#pragma unroll
        for (int i = 0; i < N; ++i) a[i] += __shfl_xor(a[i], m, kLanes);
    }
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

__device__ __forceinline__ void rodrigues(const double* r, double* R) {
    const double th = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    if (!(th >= 1e-300)) {
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    const double kx = r[0] / th, ky = r[1] / th, kz = r[2] / th;
    const double sn = sin(th), cs = 1.0 - cos(th);
    // I + sin K + (1 - cos) K^2,  K^2 = k k^T - I
    R[0] = 1.0 + cs * (kx * kx - 1.0); R[1] = -sn * kz + cs * kx * ky; R[2] = sn * ky + cs * kx * kz;
    R[3] = sn * kz + cs * kx * ky;     R[4] = 1.0 + cs * (ky * ky - 1.0); R[5] = -sn * kx + cs * ky * kz;
    R[6] = -sn * ky + cs * kx * kz;    R[7] = sn * kx + cs * ky * kz;     R[8] = 1.0 + cs * (kz * kz - 1.0);
}

// rotation vector of an orthonormal matrix: cvRodrigues2's matrix -> vector branch after its SVD
__device__ __forceinline__ void rvec_of(const double* R, double* r) {
    const double rx = R[7] - R[5], ry = R[2] - R[6], rz = R[3] - R[1];
    const double s = sqrt((rx * rx + ry * ry + rz * rz) * 0.25);
    const double c = fmin(fmax((R[0] + R[4] + R[8] - 1.0) * 0.5, -1.0), 1.0);
    const double theta = acos(c);
    if (s < 1e-5) {
        if (c > 0) { r[0] = r[1] = r[2] = 0.0; return; }
        double x = sqrt(fmax((R[0] + 1.0) * 0.5, 0.0));
        double y = sqrt(fmax((R[4] + 1.0) * 0.5, 0.0)) * (R[1] < 0 ? -1.0 : 1.0);
        double z = sqrt(fmax((R[8] + 1.0) * 0.5, 0.0)) * (R[2] < 0 ? -1.0 : 1.0);
        if (fabs(x) < fabs(y) && fabs(x) < fabs(z) && ((R[5] > 0) != (y * z > 0))) z = -z;
        const double f = M_PI / sqrt(x * x + y * y + z * z);
        r[0] = x * f; r[1] = y * f; r[2] = z * f;
        return;
    }
    const double f = theta / (2.0 * s);
    r[0] = rx * f; r[1] = ry * f; r[2] = rz * f;
}

// right Jacobian of SO(3): d(R(r) u)/dr = -R [u]x Jr(r)
__device__ __forceinline__ void right_jacobian(const double* r, double* J) {
    const double th2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
    double a, b;
    if (th2 < 1e-8) {
        a = 0.5 - th2 / 24.0;
        b = 1.0 / 6.0 - th2 / 120.0;
    } else {
        const double th = sqrt(th2);
        a = (1.0 - cos(th)) / th2;
        b = (th - sin(th)) / (th2 * th);
    }
    const double S[9] = {0.0, -r[2], r[1], r[2], 0.0, -r[0], -r[1], r[0], 0.0};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double s2 = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) s2 += S[i * 3 + k] * S[k * 3 + j];
            J[i * 3 + j] = (i == j ? 1.0 : 0.0) - a * S[i * 3 + j] + b * s2;
        }
}

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

// The rows of a frame picked by an index list (the RANSAC refit over the inlier slots): row i of this frame is row idx[i] of base.
struct IndexedFrame {
    Frame base;
    const int32_t* idx;
    int n;

    __device__ __forceinline__ void load(int i, double& X, double& Y, double& u, double& v) const { base.load(idx[i], X, Y, u, v); }
};

__device__ __forceinline__ void undistort(const PnpCamera& cam, bool dist, double u, double v, double& x, double& y) {
    const double x0 = (u - cam.cx) / cam.fx, y0 = (v - cam.cy) / cam.fy;
    x = x0;
    y = y0;
    if (!dist) return;
    const double* k = cam.k;
    for (int it = 0; it < kUndistortIters; ++it) {
        const double r2 = x * x + y * y;
        const double icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
        if (icdist < 0) {
            x = x0;
            y = y0;
            break;
        }
        const double dx = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x);
        const double dy = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y;
        x = (x0 - dx) * icdist;
        y = (y0 - dy) * icdist;
    }
}

// Sum over the frame's points of the squared reprojection error at pose p (+inf if a point is not in front of the camera) and,
// with JAC, of JtJ (21, packed) and Jtr (6).  acc = {cost, JtJ[21], Jtr[6]} on return, identical in every lane.
template <bool JAC, class F>
__device__ __forceinline__ void evaluate(const F& f, const PnpCamera& cam, const double* p, double (&acc)[28]) {
    double R[9], G[2][9];           // G[c] = -R [e_c]x Jr: d(R m)/dr for the board point m = e_c (the board has z = 0)
    rodrigues(p, R);
    if (JAC) {
        double Jr[9];
        right_jacobian(p, Jr);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            double E[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};      // [e_c]x
            if (c == 0) { E[5] = -1.0; E[7] = 1.0; } else { E[2] = 1.0; E[6] = -1.0; }
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    double s = 0.0;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        double ej = 0.0;
#pragma unroll
                        for (int l = 0; l < 3; ++l) ej += E[k * 3 + l] * Jr[l * 3 + j];
                        s += R[i * 3 + k] * ej;
                    }
                    G[c][i * 3 + j] = -s;
                }
        }
    }
#pragma unroll
    for (int i = 0; i < 28; ++i) acc[i] = 0.0;
    const double* k = cam.k;
    for (int i = threadIdx.x; i < f.n; i += kLanes) {
        double mx, my, u, v;
        f.load(i, mx, my, u, v);
        const double X = R[0] * mx + R[1] * my + p[3];
        const double Y = R[3] * mx + R[4] * my + p[4];
        const double Z = R[6] * mx + R[7] * my + p[5];
        if (!(Z > 0)) {
            acc[0] = INFINITY;
            continue;
        }
        const double iz = 1.0 / Z, x = X * iz, y = Y * iz;
        const double r2 = x * x + y * y;
        const double num = 1 + r2 * (k[0] + r2 * (k[1] + r2 * k[4]));
        const double den = 1 + r2 * (k[5] + r2 * (k[6] + r2 * k[7]));
        const double g = num / den;
        const double xd = x * g + 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x);
        const double yd = y * g + k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y;
        const double ru = cam.fx * xd + cam.cx - u, rv = cam.fy * yd + cam.cy - v;
        acc[0] += ru * ru + rv * rv;
        if (!JAC) continue;
        const double dg = ((k[0] + r2 * (2 * k[1] + 3 * k[4] * r2)) * den - num * (k[5] + r2 * (2 * k[6] + 3 * k[7] * r2))) / (den * den);
        const double dxd_dx = g + 2 * x * x * dg + 2 * k[2] * y + 6 * k[3] * x;
        const double dxd_dy = 2 * x * y * dg + 2 * k[2] * x + 2 * k[3] * y;
        const double dyd_dx = dxd_dy;
        const double dyd_dy = g + 2 * y * y * dg + 6 * k[2] * y + 2 * k[3] * x;
        // d(u, v)/d(X, Y, Z)
        const double a0 = cam.fx * dxd_dx, a1 = cam.fx * dxd_dy, b0 = cam.fy * dyd_dx, b1 = cam.fy * dyd_dy;
        const double du[3] = {a0 * iz, a1 * iz, -(a0 * x + a1 * y) * iz};
        const double dv[3] = {b0 * iz, b1 * iz, -(b0 * x + b1 * y) * iz};
        double ju[6], jv[6];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double su = 0.0, sv = 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double dX = mx * G[0][c * 3 + j] + my * G[1][c * 3 + j];
                su += du[c] * dX;
                sv += dv[c] * dX;
            }
            ju[j] = su;
            jv[j] = sv;
            ju[3 + j] = du[j];
            jv[3 + j] = dv[j];
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) {
#pragma unroll
            for (int b = a; b < 6; ++b) acc[1 + pk<6>(a, b)] += ju[a] * ju[b] + jv[a] * jv[b];
            acc[22 + a] += ju[a] * ru + jv[a] * rv;
        }
    }
    wave_sum(acc);
}

// (JtJ with its diagonal scaled by 1 + lambda) x = Jtr by Cholesky; false if not positive definite
__device__ __forceinline__ bool cholesky_solve(const double* jtj, const double* jtr, double scale, double* x) {
    double L[21];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double s = jtj[pk<6>(i, j)] * (i == j ? scale : 1.0);
#pragma unroll
            for (int k = 0; k < j; ++k) s -= L[pk<6>(i, k)] * L[pk<6>(j, k)];
            if (i == j) {
                if (!(s > 0)) return false;
                L[pk<6>(i, i)] = sqrt(s);
            } else {
                L[pk<6>(i, j)] = s / L[pk<6>(j, j)];
            }
        }
    }
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double s = jtr[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= L[pk<6>(i, k)] * y[k];
        y[i] = s / L[pk<6>(i, i)];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) s -= L[pk<6>(k, i)] * x[k];
        x[i] = s / L[pk<6>(i, i)];
    }
    return true;
}

// Planar DLT (pnp._homography) of the board points to the (undistorted) image points -> status; H (row major, h33 = 1) maps
// the centred board points (X - mcx, Y - mcy) to the image points.
template <class F>
__device__ __forceinline__ int homography(const F& f, const PnpCamera& cam, bool dist, double* H, double& mc_x, double& mc_y) {
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

// ---- the consensus searches' shared steps (dcx_pnp_ransac.hip, dcx_calib_ransac.hip): the per-frame checks, the counter-hash
// sampler, the closed-form homography through four rows and one row's reprojection error

constexpr int kMaxIterations = 4096; // hypotheses per frame (pnp.RANSAC_MAX_ITERATIONS)
constexpr int kSampleTries = 8;      // complete 4-samples per hypothesis (pnp.RANSAC_SAMPLE_TRIES)
constexpr int kMaxDraws = 256;       // slot draws per hypothesis, redraws included (pnp.RANSAC_MAX_DRAWS)

// The per-frame checks of dcx_solve_pnp_kernel, in its order -> DCX_PNP_OK if the frame's rows can be read and solved.  Wave-wide.
__device__ __forceinline__ int frame_status(const int32_t* counts, const int32_t* starts, const int32_t* rows, int b, int pool,
                                            int n_ids, int& n, int& s0) {
    n = counts[b];
    s0 = starts[b];
    if (n <= 0) return DCX_PNP_TOO_FEW;
    if (s0 < 0 || (long long)s0 + n > (long long)pool) return DCX_PNP_TRUNCATED;      // (its slots are not read)
    if (n < 4) return DCX_PNP_TOO_FEW;
    bool bad = false;
    for (int i = threadIdx.x; i < n; i += kLanes) {
        const int id = rows[4 * ((long long)s0 + i) + 2];
        bad |= id < 0 || id >= n_ids;
    }
    return __any(bad) ? DCX_PNP_BAD_ID : DCX_PNP_OK;
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

// adjugate of a row-major 3x3
__device__ __forceinline__ void adjugate(const double* m, double* a) {
    a[0] = m[4] * m[8] - m[5] * m[7]; a[1] = m[2] * m[7] - m[1] * m[8]; a[2] = m[1] * m[5] - m[2] * m[4];
    a[3] = m[5] * m[6] - m[3] * m[8]; a[4] = m[0] * m[8] - m[2] * m[6]; a[5] = m[2] * m[3] - m[0] * m[5];
    a[6] = m[3] * m[7] - m[4] * m[6]; a[7] = m[1] * m[6] - m[0] * m[7]; a[8] = m[0] * m[4] - m[1] * m[3];
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
__device__ __forceinline__ double row_error2(const double* R, const double* t, const PnpCamera& cam, double mx, double my, double u,
                                             double v) {
    const double X = R[0] * mx + R[1] * my + t[0];
    const double Y = R[3] * mx + R[4] * my + t[1];
    const double Z = R[6] * mx + R[7] * my + t[2];
    if (!(Z > 0)) return INFINITY;
    const double* k = cam.k;
    const double iz = 1.0 / Z, x = X * iz, y = Y * iz;
    const double r2 = x * x + y * y;
    const double num = 1 + r2 * (k[0] + r2 * (k[1] + r2 * k[4]));
    const double den = 1 + r2 * (k[5] + r2 * (k[6] + r2 * k[7]));
    const double g = num / den;
    const double xd = x * g + 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x);
    const double yd = y * g + k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y;
    const double ru = cam.fx * xd + cam.cx - u, rv = cam.fy * yd + cam.cy - v;
    return ru * ru + rv * rv;
}

// Four sampled rows of a frame, held by one lane: board points and undistorted image points.
struct Sample {
    double mx[4], my[4], x[4], y[4];
};

// pnp._homography4: the homography through exactly four points in closed form, H = B adj(A) with A, B the projective bases of the
// centred board points and of the image points.  init_pose() picks this overload for a Sample; no cross-lane step.
__device__ __forceinline__ int homography(const Sample& q, const PnpCamera&, bool, double* H, double& mc_x, double& mc_y) {
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
template <class F>
__device__ __forceinline__ int init_pose(const F& f, const PnpCamera& cam, bool dist, double* p0) {
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
    // polar factor Rr (Rr^T Rr)^-1/2
    double S[6], W[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) S[pk<3>(a, b)] = Rr[a] * Rr[b] + Rr[3 + a] * Rr[3 + b] + Rr[6 + a] * Rr[6 + b];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) W[a][b] = a == b ? 1.0 : 0.0;
    jacobi<3, 3>(S, W);
    double iw[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double w = S[pk<3>(c, c)];
        if (!(w > 0)) return DCX_PNP_DEGENERATE;
        iw[c] = 1.0 / sqrt(w);
    }
    double P[9], Q[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) P[a * 3 + b] = W[a][0] * iw[0] * W[b][0] + W[a][1] * iw[1] * W[b][1] + W[a][2] * iw[2] * W[b][2];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) Q[a * 3 + b] = Rr[a * 3 + 0] * P[b] + Rr[a * 3 + 1] * P[3 + b] + Rr[a * 3 + 2] * P[6 + b];
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

template <class F>
__device__ __forceinline__ int solve(const F& f, const PnpCamera& cam, double* pose) {
    bool dist = false;
#pragma unroll
    for (int i = 0; i < 8; ++i) dist |= cam.k[i] != 0.0;
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
