// dcx_rectify.hip -- stereo rectification on the device: the undistort + rectify map (cv2.initUndistortRectifyMap in 1/32 px fixed
// point), the remap of u8 frames through it (cv2.remap INTER_LINEAR / BORDER_CONSTANT, the per-frame hot path) and the corner pool
// in rectified coordinates (cv2.undistortPoints with R and P).  deepcharuco_amd/rectify.py restates every step
// (undistort_rectify_map_host, remap_host, rectify_points_host) and is the pin of these kernels; the rectifying transforms
// themselves (stereo_rectify_host) run once per rig over 18 numbers and stay on the host.
//
// Map and points are fp64 and agree with the host to rounding; the remap is integer and agrees bit for bit.  K, the distortion
// coefficients, R and P are kernel arguments (a captured hipGraph keeps them).  No allocation, no synchronisation, no atomics, no
// LDS in any of the three.  The map and points kernels are dcx_rectify_dev.h's, one text for this unit's pinhole and
// dcx_fisheye.hip's fisheye; the distortion model and its derivative (distort<>) are dcx_camera_dev.h's, the one copy the pose and
// calibration kernels project through.  The remap reads a map whichever model made it.
#include "dcx_rectify_dev.h"

namespace {

constexpr int kFrameGroup = 8;               // rectify.REMAP_FRAME_GROUP: frames one remap thread serves with its map entries held
constexpr int kPix = 4;                      // output pixels of one remap thread: 32 B of map (two 16-B loads), one dword of gray

// ---- the remap
//
// One map serves every frame of the batch, and a map entry (8 B) outweighs the 1 - 3 B of the pixel it places, so a thread takes
// kPix consecutive output pixels (the output and the map are dense, so the pixels of a frame are one flat run: consecutive means
// horizontally adjacent but for a row's end), decodes their map entries ONCE into tap offsets, weights and inside-flags, and loops
// over the kFrameGroup frames of its group (grid z) with those in registers.  Map loads are 16 B and gray / BGR stores whole
// dwords where the frame's pixel count and the pointers allow (VEC); the flat run's last thread and unaligned calls store bytes.
// The taps are byte gathers that the caches serve: every tap address is clamped into the source, loaded unconditionally and
// replaced by `border` where the tap is outside, so no lane branches and no address leaves the frame.
struct Taps {
    int off[4];                 // byte offsets of the (clamped) taps 00, 10, 01, 11 of channel 0 in a frame
    unsigned w[4];              // their weights, summing to 1024
    bool in[4];
};

__device__ __forceinline__ Taps decode(int mx, int my, int src_h, int src_w, int pitch, int ch) {
    Taps t;
    const int x0 = mx >> kMapShift, y0 = my >> kMapShift;            // arithmetic shifts: floor
    const unsigned fx = mx & 31, fy = my & 31;
    const bool ix0 = x0 >= 0 && x0 < src_w, ix1 = x0 >= -1 && x0 < src_w - 1;
    const bool iy0 = y0 >= 0 && y0 < src_h, iy1 = y0 >= -1 && y0 < src_h - 1;
    const int cx0 = min(max(x0, 0), src_w - 1) * ch, cx1 = min(max(x0, -1) + 1, src_w - 1) * ch;
    const int cy0 = min(max(y0, 0), src_h - 1) * pitch, cy1 = min(max(y0, -1) + 1, src_h - 1) * pitch;
    t.off[0] = cy0 + cx0; t.off[1] = cy0 + cx1; t.off[2] = cy1 + cx0; t.off[3] = cy1 + cx1;
    t.w[0] = (32 - fx) * (32 - fy); t.w[1] = fx * (32 - fy); t.w[2] = (32 - fx) * fy; t.w[3] = fx * fy;
    t.in[0] = iy0 && ix0; t.in[1] = iy0 && ix1; t.in[2] = iy1 && ix0; t.in[3] = iy1 && ix1;
    return t;
}

template <int CH, bool VEC>
__global__ __launch_bounds__(256) void dcx_remap_u8_kernel(const uint8_t* __restrict__ src, long frame_stride, int pitch, int src_h,
                                                             int src_w, const int32_t* __restrict__ map, int n_pix, int batch,
                                                             unsigned border, uint8_t* __restrict__ out) {
    const int p0 = (blockIdx.x * 256 + threadIdx.x) * kPix;
    if (p0 >= n_pix) return;
    const int n = min(kPix, n_pix - p0);
    int m[2 * kPix];
    if (VEC && n == kPix) {
        const int4 lo = reinterpret_cast<const int4*>(map + 2 * (size_t)p0)[0], hi = reinterpret_cast<const int4*>(map + 2 * (size_t)p0)[1];
        m[0] = lo.x; m[1] = lo.y; m[2] = lo.z; m[3] = lo.w; m[4] = hi.x; m[5] = hi.y; m[6] = hi.z; m[7] = hi.w;
    } else {
#pragma unroll
        for (int i = 0; i < kPix; ++i) {
            const int2 e = i < n ? reinterpret_cast<const int2*>(map)[(size_t)p0 + i] : make_int2(INT32_MIN, INT32_MIN);
            m[2 * i] = e.x;
            m[2 * i + 1] = e.y;
        }
    }
    Taps t[kPix];
#pragma unroll
    for (int i = 0; i < kPix; ++i) t[i] = decode(m[2 * i], m[2 * i + 1], src_h, src_w, pitch, CH);
    const int f0 = blockIdx.z * kFrameGroup, f1 = min(f0 + kFrameGroup, batch);
#pragma unroll 2
    for (int f = f0; f < f1; ++f) {
        const uint8_t* s = src + (size_t)f * frame_stride;
        uint8_t* o = out + ((size_t)f * n_pix + p0) * CH;
        unsigned char r[kPix * CH];
#pragma unroll
        for (int i = 0; i < kPix; ++i) {
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                unsigned acc = 512;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned p = s[t[i].off[k] + c];
                    acc += t[i].w[k] * (t[i].in[k] ? p : border);
                }
                r[i * CH + c] = (unsigned char)(acc >> 10);
            }
        }
        if (VEC && n == kPix) {
#pragma unroll
            for (int j = 0; j < CH; ++j)
                reinterpret_cast<unsigned*>(o)[j] = (unsigned)r[4 * j] | (unsigned)r[4 * j + 1] << 8 | (unsigned)r[4 * j + 2] << 16 |
                                                    (unsigned)r[4 * j + 3] << 24;
        } else {
#pragma unroll
            for (int j = 0; j < kPix * CH; ++j)
                if (j < n * CH) o[j] = r[j];
        }
    }
}

}  // namespace

extern "C" int dcx_undistort_rectify_map(const double* h_camera9, const double* h_dist, int n_dist, const double* h_R9,
                                         const double* h_P12, int width, int height, int32_t* d_map, void* stream) {
    if (!d_map || ((uintptr_t)d_map & 7) || width <= 0 || height <= 0 || (long long)width * height > 0x7fffffffLL / 2) return DCX_E_ARG;
    PnpCamera cam;
    RectXform xf;
    if (!pnp_camera(h_camera9, h_dist, n_dist, cam) || !rect_xform(h_R9, h_P12, cam, xf)) return DCX_E_ARG;
    const dim3 grid((unsigned)((width + 63) / 64), (unsigned)((height + 3) / 4));
    if (grid.y > 65535u) return DCX_E_ARG;
    hipLaunchKernelGGL(dcx_rectify_map_kernel<PnpCamera>, grid, dim3(256), 0, (hipStream_t)stream, cam, xf, width, height, d_map);
    return (int)hipGetLastError();
}

extern "C" int dcx_rectify_points_pool(const int32_t* d_rows, const float* d_xy, int pool, const double* h_camera9,
                                       const double* h_dist, int n_dist, const double* h_R9, const double* h_P12, double* d_out,
                                       void* stream) {
    if (pool < 0 || (pool > 0 && (!d_out || (!d_rows && !d_xy)))) return DCX_E_ARG;
    PnpCamera cam;
    RectXform xf;
    if (!pnp_camera(h_camera9, h_dist, n_dist, cam) || !rect_xform(h_R9, h_P12, cam, xf)) return DCX_E_ARG;
    if (pool == 0) return 0;
    hipLaunchKernelGGL(dcx_rectify_points_kernel<PnpCamera>, dim3((unsigned)((pool + kLanes - 1) / kLanes)), dim3(kLanes), 0,
                       (hipStream_t)stream, d_rows, d_xy, pool, cam, xf, d_out);
    return (int)hipGetLastError();
}

extern "C" int dcx_remap_u8(const uint8_t* d_src, long frame_stride, int pitch, int src_h, int src_w, int channels,
                            const int32_t* d_map, int out_h, int out_w, int batch, int border, uint8_t* d_out, void* stream) {
    if (!d_src || !d_map || ((uintptr_t)d_map & 7) || !d_out || border < 0 || border > 255 || frame_stride < 0) return DCX_E_ARG;
    if (channels != 1 && channels != 3) return DCX_E_ARG;
    if (batch <= 0 || src_h <= 0 || src_w <= 0 || out_h <= 0 || out_w <= 0) return DCX_E_SHAPE;
    if ((long long)pitch < (long long)src_w * channels || (long long)pitch * src_h > 0x7fffffffLL) return DCX_E_SHAPE;
    const long long n_pix = (long long)out_h * out_w;
    if (n_pix * channels > 0x7fffffffLL / 4) return DCX_E_SHAPE;
    const unsigned groups = (unsigned)((batch + kFrameGroup - 1) / kFrameGroup);
    if (groups > 65535u) return DCX_E_SHAPE;
    const dim3 grid((unsigned)((n_pix + 256 * kPix - 1) / (256 * kPix)), 1, groups);
    // whole-dword stores need every frame of the dense output to start on a dword; 16-B map loads a 16-B aligned map
    const bool vec = ((n_pix * channels) & 3) == 0 && ((uintptr_t)d_out & 3) == 0 && ((uintptr_t)d_map & 15) == 0;
#define DCX_REMAP(CH, VEC)                                                                                                        \
    hipLaunchKernelGGL((dcx_remap_u8_kernel<CH, VEC>), grid, dim3(256), 0, (hipStream_t)stream, d_src, frame_stride, pitch, src_h, \
                       src_w, d_map, (int)n_pix, batch, (unsigned)border, d_out)
    if (channels == 1) {
        if (vec) DCX_REMAP(1, true); else DCX_REMAP(1, false);
    } else {
        if (vec) DCX_REMAP(3, true); else DCX_REMAP(3, false);
    }
#undef DCX_REMAP
    return (int)hipGetLastError();
}
