// dcx_rectify_dev.h -- the undistort + rectify map and the rectified points, one text for both camera models: dcx_rectify.hip
// instantiates the two kernels below on PnpCamera, dcx_fisheye.hip on FisheyeCamera.  Both fp64, no allocation, no
// synchronisation, no atomics, no LDS; K, the coefficients, R and P are kernel arguments (a captured hipGraph keeps them).  The
// map kernel reaches its model through model_point (the normalised point through the distortion), one overload per camera; the
// points kernel inverts it from a pixel: the fisheye by dcx_fisheye_dev.h's undistort(), the pinhole by a Newton loop that
// stands in the kernel (why: there).
#pragma once
#include "dcx_fisheye_dev.h"

#include <type_traits>

namespace {

constexpr int kMapShift = 5;                 // fractional bits of a map entry
constexpr double kMapLimit = 32768.0;        // a source position beyond this many px is outside
constexpr int kNewtonMaxIter = 20;           // rectify.NEWTON_MAX_ITER
constexpr double kNewtonEps = 1e-15;         // rectify.NEWTON_EPS

struct RectXform {
    double R[9];                             // row major
    double fx, fy, cx, cy;                   // the left 3x3 of P
};

// R (NULL: identity) and P (3x4 row major, NULL: K) from the host -> the kernel argument; false if refused
template <class Camera>
inline bool rect_xform(const double* h_R9, const double* h_P12, const Camera& cam, RectXform& x) {
    for (int i = 0; i < 9; ++i) {
        x.R[i] = h_R9 ? h_R9[i] : (i % 4 == 0 ? 1.0 : 0.0);
        if (!isfinite(x.R[i])) return false;
    }
    if (h_P12) {
        if (h_P12[1] != 0.0) return false;
        x.fx = h_P12[0]; x.cx = h_P12[2]; x.fy = h_P12[5]; x.cy = h_P12[6];
    } else {
        x.fx = cam.fx; x.fy = cam.fy; x.cx = cam.cx; x.cy = cam.cy;
    }
    return isfinite(x.fx) && isfinite(x.fy) && isfinite(x.cx) && isfinite(x.cy) && x.fx != 0.0 && x.fy != 0.0;
}

// ---- the models: normalised (x, y) -> the model's (xd, yd)

__device__ __forceinline__ void model_point(const PnpCamera& cam, double x, double y, double& xd, double& yd) {
    double a, b, d;
    distort<false>(cam.k, x, y, xd, yd, a, b, d);
}

__device__ __forceinline__ void model_point(const FisheyeCamera& cam, double x, double y, double& xd, double& yd) {
    double tt, t2, a, b, d;
    fisheye_distort<false>(cam.k, x, y, xd, yd, tt, t2, a, b, d);
}

// ---- the map: one thread per output pixel

template <class Camera>
__global__ __launch_bounds__(256) void dcx_rectify_map_kernel(Camera cam, RectXform xf, int width, int height,
                                                                int32_t* __restrict__ map) {
    const int u = blockIdx.x * 64 + (threadIdx.x & 63), v = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (u >= width || v >= height) return;
    const double x = ((double)u - xf.cx) / xf.fx, y = ((double)v - xf.cy) / xf.fy;
    const double qx = xf.R[0] * x + xf.R[3] * y + xf.R[6];          // R^T (x, y, 1)
    const double qy = xf.R[1] * x + xf.R[4] * y + xf.R[7];
    const double qz = xf.R[2] * x + xf.R[5] * y + xf.R[8];
    double xd, yd;
    model_point(cam, qx / qz, qy / qz, xd, yd);
    const double mx = cam.fx * xd + cam.cx, my = cam.fy * yd + cam.cy;
    int2 e = make_int2(INT32_MIN, INT32_MIN);
    if (qz > 0 && fabs(mx) <= kMapLimit && fabs(my) <= kMapLimit)    // (NaN and inf compare false)
        e = make_int2((int)rint((double)(1 << kMapShift) * mx), (int)rint((double)(1 << kMapShift) * my));
    reinterpret_cast<int2*>(map)[(size_t)v * width + u] = e;
}

// ---- the points: one lane per slot of the pool

template <class Camera>
__global__ __launch_bounds__(kLanes) void dcx_rectify_points_kernel(const int32_t* __restrict__ rows, const float* __restrict__ xy,
                                                                      int pool, Camera cam, RectXform xf,
                                                                      double* __restrict__ out) {
    const int i = blockIdx.x * kLanes + threadIdx.x;
    if (i >= pool) return;
    double u, v;
    if (xy) {
        u = (double)xy[2 * (size_t)i];
        v = (double)xy[2 * (size_t)i + 1];
    } else {
        u = (double)rows[4 * (size_t)i];
        v = (double)rows[4 * (size_t)i + 1];
    }
    // pixel -> normalised (x, y), and whether the pixel is inside the model
    double x, y;
    bool inside;
    if constexpr (std::is_same_v<Camera, PnpCamera>) {
        // Newton on distort<true>'s analytic 2x2 Jacobian from the normalised pixel, to convergence (PnP's undistort() keeps cv2's
        // five rounds).  Not an overload beside undistort(): inlined from a function, the compiler contracts x * x + y * y in
        // distort and the two products of each row of R below the other way round (which product is rounded before the add):
        // the same instruction counts and other last bits in the output.
        const double x0 = (u - cam.cx) / cam.fx, y0 = (v - cam.cy) / cam.fy;
        x = x0;
        y = y0;
        inside = false;
#pragma unroll 1
        for (int it = 0; it < kNewtonMaxIter && !inside; ++it) {
            double xd, yd, a, b, d;
            distort<true>(cam.k, x, y, xd, yd, a, b, d);
            const double ex = xd - x0, ey = yd - y0;
            const double det = a * d - b * b;
            const double sx = (d * ex - b * ey) / det, sy = (a * ey - b * ex) / det;
            x -= sx;
            y -= sy;
            inside = fabs(sx) < kNewtonEps && fabs(sy) < kNewtonEps;
        }
    } else {
        inside = undistort(cam, u, v, x, y);
    }
    const double X = xf.R[0] * x + xf.R[1] * y + xf.R[2];
    const double Y = xf.R[3] * x + xf.R[4] * y + xf.R[5];
    const double Z = xf.R[6] * x + xf.R[7] * y + xf.R[8];
    double ou = NAN, ov = NAN;
    if (inside && Z > 0) {
        ou = xf.fx * (X / Z) + xf.cx;
        ov = xf.fy * (Y / Z) + xf.cy;
    }
    out[2 * (size_t)i] = ou;
    out[2 * (size_t)i + 1] = ov;
}

}  // namespace
