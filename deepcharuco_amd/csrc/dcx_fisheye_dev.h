// dcx_fisheye_dev.h -- the fisheye camera model (OpenCV's documented cv2.fisheye, skew 0) for the pose, calibration and
// rectification kernels of dcx_fisheye.hip, all fp64, beside the pinhole of dcx_camera_dev.h and with the same contracts, so that
// the PnP solver of dcx_pnp_dev.h (a template on the camera class) runs through either.  For a camera-frame point (X, Y, Z):
//   a = X / Z, b = Y / Z, r = sqrt(a^2 + b^2), theta = atan r, theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8),
//   x' = (theta_d / r) a, y' = (theta_d / r) b, u = fx x' + cx, v = fy y' + cy.
// As everywhere in this project a point must have Z > 0: the field of view is under 180 degrees (theta in [0, pi/2)).
// s = theta_d / r and w = (ds/dr) / r are taken by their series in r^2 below r = kFisheyeSmallR (no division by r; a point on the
// optical axis is a valid input).  The inverse is Newton on theta (1 + k1 theta^2 + ...) - theta_d from theta = theta_d, to
// convergence (kFisheyeNewtonMaxIter, kFisheyeNewtonEps: rectify.py's NEWTON_*); a pixel is OUTSIDE if Newton does not converge or
// theta is not in [0, pi/2).  deepcharuco_amd/fisheye.py restates every step (its functions of the same names).
// Everything is force-inlined and has internal linkage, so each translation unit compiles its own copy.
#pragma once
#include "dcx_camera_dev.h"

namespace {

constexpr double kFisheyeSmallR = 1e-4;          // below it s and w come from their series (truncation: r^6 / 7 and O(r^4))
constexpr double kFisheyeSmallThetaD = 1e-8;     // below it tan(theta) / theta_d = 1 to the last bit
constexpr int kFisheyeNewtonMaxIter = 20;        // rectify.NEWTON_MAX_ITER
constexpr double kFisheyeNewtonEps = 1e-15;      // rectify.NEWTON_EPS

struct FisheyeCamera {
    double fx, fy, cx, cy;
    double k[4];            // k1 k2 k3 k4
};

// K (row major, no skew) and the four coefficients (NULL: zeros) from the host -> the kernel argument; false if refused, as
// pnp_camera() refuses (skew, a non-finite entry, a zero focal length)
inline bool fisheye_camera(const double* h_camera9, const double* h_dist4, FisheyeCamera& cam) {
    if (!h_camera9 || h_camera9[1] != 0.0) return false;
    cam.fx = h_camera9[0];
    cam.fy = h_camera9[4];
    cam.cx = h_camera9[2];
    cam.cy = h_camera9[5];
    if (!(isfinite(cam.fx) && isfinite(cam.fy) && isfinite(cam.cx) && isfinite(cam.cy)) || cam.fx == 0.0 || cam.fy == 0.0)
        return false;
    for (int i = 0; i < 4; ++i) {
        cam.k[i] = h_dist4 ? h_dist4[i] : 0.0;
        if (!isfinite(cam.k[i])) return false;
    }
    return true;
}

// calibration's theta = (fx, fy, cx, cy, k1, k2, k3, k4) as a camera
__host__ __device__ __forceinline__ FisheyeCamera fisheye_camera_of(const double* th) {
    FisheyeCamera c;
    c.fx = th[0]; c.fy = th[1]; c.cx = th[2]; c.cy = th[3];
#pragma unroll
    for (int i = 0; i < 4; ++i) c.k[i] = th[4 + i];
    return c;
}

// the solver's question "is there anything to undistort": always, theta_d is not tan(theta) even with k = 0
__device__ __forceinline__ bool has_distortion(const FisheyeCamera&) { return true; }

// Pixel -> the pinhole-normalised point (tan(theta) along the pixel's direction); false (x = y = NaN) if the pixel is outside
__device__ __forceinline__ bool undistort(const FisheyeCamera& cam, double u, double v, double& x, double& y) {
    const double xp = (u - cam.cx) / cam.fx, yp = (v - cam.cy) / cam.fy;
    const double thd = sqrt(xp * xp + yp * yp);
    const double* k = cam.k;
    double th = thd;
    bool done = false;
#pragma unroll 1
    for (int it = 0; it < kFisheyeNewtonMaxIter && !done; ++it) {
        const double t2 = th * th;
        const double f = th * (1 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3])))) - thd;
        const double df = 1 + t2 * (3 * k[0] + t2 * (5 * k[1] + t2 * (7 * k[2] + t2 * 9 * k[3])));
        const double s = f / df;
        th -= s;
        done = fabs(s) < kFisheyeNewtonEps;
    }
    if (!(done && th >= 0.0 && th < M_PI_2)) {       // (NaN compares false)
        x = y = NAN;
        return false;
    }
    const double sc = thd < kFisheyeSmallThetaD ? 1.0 : tan(th) / thd;
    x = xp * sc;
    y = yp * sc;
    return true;
}

// the solver's form of it (the flag of the pinhole's is not needed: see has_distortion): an outside pixel leaves NaN, which
// solve() never meets, points_inside() having refused the frame before
__device__ __forceinline__ void undistort(const FisheyeCamera& cam, bool, double u, double v, double& x, double& y) {
    undistort(cam, u, v, x, y);
}

// solve()'s check in front of everything else: does every image point of the frame undistort?  Wave-wide.
template <class F>
__device__ __forceinline__ bool points_inside(const F& f, const FisheyeCamera& cam) {
    bool bad = false;
    for (int i = threadIdx.x; i < f.n; i += kLanes) {
        double mx, my, u, v, x, y;
        f.load(i, mx, my, u, v);
        bad |= !undistort(cam, u, v, x, y);
    }
    return !__any(bad);
}

// Normalised (a, b) -> the model's (x', y'); tt = theta / r and t2 = theta^2, which the k columns are made of
// (dx'/dk_j = a tt theta^(2j)); with JAC dxa = dx'/da, dxb = dx'/db (= dy'/da), dyb = dy'/db.
template <bool JAC>
__device__ __forceinline__ void fisheye_distort(const double* k, double a, double b, double& xd, double& yd, double& tt, double& t2,
                                                double& dxa, double& dxb, double& dyb) {
    const double r2 = a * a + b * b;
    const double r = sqrt(r2);
    const double th = atan(r);
    const bool small = r < kFisheyeSmallR;
    tt = small ? 1.0 + r2 * (-1.0 / 3.0 + r2 * (1.0 / 5.0)) : th / r;
    t2 = th * th;
    const double s = tt * (1 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))));
    xd = s * a;
    yd = s * b;
    if (!JAC) return;
    const double dthd = 1 + t2 * (3 * k[0] + t2 * (5 * k[1] + t2 * (7 * k[2] + t2 * 9 * k[3])));
    // w = (ds/dr) / r: s = 1 + (k1 - 1/3) r^2 + (1/5 - k1 + k2) r^4 + ..., so w = 2 (k1 - 1/3) + 4 (1/5 - k1 + k2) r^2 + ...
    const double w = small ? 2.0 * (k[0] - 1.0 / 3.0) + 4.0 * (1.0 / 5.0 - k[0] + k[1]) * r2 : (dthd / (1.0 + r2) - s) / r2;
    dxa = s + a * a * w;
    dxb = a * b * w;
    dyb = s + b * b * w;
}

// The camera-frame point q through the model -> its residual (ru, rv) against the image point (u, v) and, with JAC, du = du/dq,
// dv = dv/dq; false (nothing written) if q is not in front of the camera: the pinhole project()'s contract.  Also out: the
// normalised point (a, b), the model's (xd, yd) and fisheye_distort()'s tt, t2, which calibration's intrinsic columns are made of.
template <bool JAC>
__device__ __forceinline__ bool project(const FisheyeCamera& cam, const double* q, double u, double v, double& ru, double& rv, double* du,
                                        double* dv, double& a, double& b, double& xd, double& yd, double& tt, double& t2) {
    if (!(q[2] > 0)) return false;
    const double iz = 1.0 / q[2];
    a = q[0] * iz;
    b = q[1] * iz;
    double dxa, dxb, dyb;
    fisheye_distort<JAC>(cam.k, a, b, xd, yd, tt, t2, dxa, dxb, dyb);
    ru = cam.fx * xd + cam.cx - u;
    rv = cam.fy * yd + cam.cy - v;
    if (!JAC) return true;
    const double a0 = cam.fx * dxa, a1 = cam.fx * dxb, b0 = cam.fy * dxb, b1 = cam.fy * dyb;
    du[0] = a0 * iz; du[1] = a1 * iz; du[2] = -(a0 * a + a1 * b) * iz;
    dv[0] = b0 * iz; dv[1] = b1 * iz; dv[2] = -(b0 * a + b1 * b) * iz;
    return true;
}

template <bool JAC>
__device__ __forceinline__ bool project(const FisheyeCamera& cam, const double* q, double u, double v, double& ru, double& rv, double* du,
                                        double* dv) {
    double a, b, xd, yd, tt, t2;
    return project<JAC>(cam, q, u, v, ru, rv, du, dv, a, b, xd, yd, tt, t2);
}

}  // namespace
