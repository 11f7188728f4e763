// dcx_camera_dev.h -- the camera model and the rotations of the pose, calibration and rectification kernels, one copy each (all
// fp64): the camera as a kernel argument, Rodrigues both ways, the SO(3) right Jacobian, undistortPoints, the pinhole +
// rational/tangential distortion with its derivative (distort, project), and the pose part of a row's Jacobian (pose_basis,
// pose_columns).  deepcharuco_amd/pnp.py restates every step (its functions of the same names; _project holds the model).
// dcx_rectify.hip needs no more than this header; the pool reader and the solvers on top are dcx_pnp_dev.h.
// Everything is force-inlined and has internal linkage, so each translation unit compiles its own copy.
#pragma once
#include "dcx_mat_dev.h"

namespace {

constexpr int kUndistortIters = 5;

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

// calibration's theta = (fx, fy, cx, cy, k1, k2, p1, p2, k3) as a camera
__host__ __device__ __forceinline__ PnpCamera camera_of(const double* th) {
    PnpCamera c;
    c.fx = th[0]; c.fy = th[1]; c.cx = th[2]; c.cy = th[3];
#pragma unroll
    for (int i = 0; i < 8; ++i) c.k[i] = i < 5 ? th[4 + i] : 0.0;
    return c;
}

// fx = fy = 1, cx = cy = 0, no distortion: undistort() through it is the identity, the pixels are taken as they are
__device__ __forceinline__ PnpCamera identity_camera() {
    PnpCamera c;
    c.fx = c.fy = 1.0;
    c.cx = c.cy = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) c.k[i] = 0.0;
    return c;
}

__device__ __forceinline__ bool has_distortion(const PnpCamera& cam) {
    bool dist = false;
#pragma unroll
    for (int i = 0; i < 8; ++i) dist |= cam.k[i] != 0.0;
    return dist;
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

// normalised (x, y) -> distorted normalised (xd, yd) and, with JAC, a = dxd/dx, b = dxd/dy (= dyd/dx), d = dyd/dy
template <bool JAC>
__device__ __forceinline__ void distort(const double* k, double x, double y, double& xd, double& yd, double& a, double& b, double& d) {
    const double r2 = x * x + y * y;
    const double num = 1 + r2 * (k[0] + r2 * (k[1] + r2 * k[4]));
    const double den = 1 + r2 * (k[5] + r2 * (k[6] + r2 * k[7]));
    const double g = num / den;
    xd = x * g + 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x);
    yd = y * g + k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y;
    if (!JAC) return;
    const double dg = ((k[0] + r2 * (2 * k[1] + 3 * k[4] * r2)) * den - num * (k[5] + r2 * (2 * k[6] + 3 * k[7] * r2))) / (den * den);
    a = g + 2 * x * x * dg + 2 * k[2] * y + 6 * k[3] * x;
    b = 2 * x * y * dg + 2 * k[2] * x + 2 * k[3] * y;
    d = g + 2 * y * y * dg + 6 * k[2] * y + 2 * k[3] * x;
}

// The camera-frame point q through the pinhole and distort() -> its residual (ru, rv) against the image point (u, v) and, with
// JAC, du = du/dq, dv = dv/dq; false (nothing written) if q is not in front of the camera.  Also out: the normalised point
// (x, y) and the distorted one (xd, yd), which calibration's intrinsic columns are made of.
template <bool JAC>
__device__ __forceinline__ bool project(const PnpCamera& cam, const double* q, double u, double v, double& ru, double& rv, double* du,
                                        double* dv, double& x, double& y, double& xd, double& yd) {
    if (!(q[2] > 0)) return false;
    const double iz = 1.0 / q[2];
    x = q[0] * iz;
    y = q[1] * iz;
    double dxd_dx, dxd_dy, dyd_dy;
    distort<JAC>(cam.k, x, y, xd, yd, dxd_dx, dxd_dy, dyd_dy);
    ru = cam.fx * xd + cam.cx - u;
    rv = cam.fy * yd + cam.cy - v;
    if (!JAC) return true;
    const double dyd_dx = dxd_dy;
    const double a0 = cam.fx * dxd_dx, a1 = cam.fx * dxd_dy, b0 = cam.fy * dyd_dx, b1 = cam.fy * dyd_dy;
    du[0] = a0 * iz; du[1] = a1 * iz; du[2] = -(a0 * x + a1 * y) * iz;
    dv[0] = b0 * iz; dv[1] = b1 * iz; dv[2] = -(b0 * x + b1 * y) * iz;
    return true;
}

template <bool JAC>
__device__ __forceinline__ bool project(const PnpCamera& cam, const double* q, double u, double v, double& ru, double& rv, double* du,
                                        double* dv) {
    double x, y, xd, yd;
    return project<JAC>(cam, q, u, v, ru, rv, du, dv, x, y, xd, yd);
}

// the board point (mx, my, 0) at the pose (R, t) in the camera's frame
__device__ __forceinline__ void board_point(const double* R, const double* t, double mx, double my, double* q) {
    q[0] = R[0] * mx + R[1] * my + t[0];
    q[1] = R[3] * mx + R[4] * my + t[1];
    q[2] = R[6] * mx + R[7] * my + t[2];
}

// R(p) and G[c] = -R [e_c]x Jr(p): d(R m)/dr for the board point m = e_c (the board has z = 0)
__device__ __forceinline__ void pose_basis(const double* p, double* R, double (*G)[9]) {
    double Jr[9];
    rodrigues(p, R);
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

// The six pose columns of a row's Jacobian, rotation first, from du = du/dq0, dv = dv/dq0 (q0 = R m + t, m = (mx, my, 0)) and
// pose_basis()'s G
__device__ __forceinline__ void pose_columns(const double* du, const double* dv, double mx, double my, const double (*G)[9], double* ju,
                                             double* jv) {
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
}

}  // namespace
