// dcx_first_dev.h -- the steps every Cin = 1 first-layer kernel of dcx_misc.hip takes (conv1a of both nets: dcx_conv1_kernel,
// dcx_conv1_tile_kernel, dcx_conv1_patches_kernel) and the pixel formats they and dcx_gather_kernel / dcx_bgr2gray_kernel load.
// The bits of a first-layer output are defined HERE, once: dcx_px_padded for the value of a tap, dcx_conv1_quad for the
// arithmetic on nine taps.  Which kernel a launch size selects decides who calls them, never what they compute.
#pragma once
#include "dcx_common.h"

// pre_bgr_image model_utils.py:46-50: (float(g) - 128) / 255, IEEE division
// (hipcc's default f32 division is correctly rounded; tests check all 256 inputs bit-for-bit).
__device__ __forceinline__ float dcx_norm_u8(uint8_t g) { return ((float)g - 128.0f) / 255.0f; }

// cv2.cvtColor(img, COLOR_BGR2GRAY) on 8-bit pixels, one generation of OpenCV's fixed-point constants (dcx_bgr2gray_kernel's
// comment in dcx_misc.hip has their history): gray = (CB B + CG G + CR R + half) >> SHIFT.
template <unsigned B, unsigned G, unsigned R, int S>
struct DcxBgrGray {
    static constexpr unsigned CB = B, CG = G, CR = R;
    static constexpr int SHIFT = S;
    static_assert(CB + CG + CR == (1u << SHIFT), "the weights of a gray conversion sum to one");
    static __device__ __forceinline__ uint8_t gray(unsigned bb, unsigned gg, unsigned rr) {
        return (uint8_t)((bb * CB + gg * CG + rr * CR + (1u << (SHIFT - 1))) >> SHIFT);
    }
};
using DcxGray15 = DcxBgrGray<3735u, 19235u, 9798u, 15>;      // OpenCV 4.x, 8-bit images
using DcxGray14 = DcxBgrGray<1868u, 9617u, 4899u, 14>;       // older generations

// Pixel formats of the u8 frames (DCX_PIX_*): gray, or interleaved BGR converted in the load -- the gray frame of inference.py:40
// is never materialised.  BPP = bytes per pixel.  DcxPixF32: an image that is normalised already.
template <int PIX>
struct DcxPix {
    static_assert(dcx_pix_valid(PIX), "DCX_PIX_*");
    static constexpr int BPP = dcx_pix_bpp(PIX);
    static __device__ __forceinline__ float load(const uint8_t* p) {
        if constexpr (PIX == DCX_PIX_GRAY8) return dcx_norm_u8(*p);
        else if constexpr (PIX == DCX_PIX_BGR8) return dcx_norm_u8(DcxGray15::gray(p[0], p[1], p[2]));
        else return dcx_norm_u8(DcxGray14::gray(p[0], p[1], p[2]));
    }
};
struct DcxPixF32 {
    static constexpr int BPP = 4;
    static __device__ __forceinline__ float load(const uint8_t* p) { return *reinterpret_cast<const float*>(p); }
};

// f(DcxPix<pix>()) for a run-time pix; DCX_E_ARG for a value that is no DCX_PIX_*
template <typename F>
static int dcx_with_pix(int pix, F&& f) {
    switch (pix) {
        case DCX_PIX_GRAY8: return f(DcxPix<DCX_PIX_GRAY8>());
        case DCX_PIX_BGR8: return f(DcxPix<DCX_PIX_BGR8>());
        case DCX_PIX_BGR8_LEGACY14: return f(DcxPix<DCX_PIX_BGR8_LEGACY14>());
        default: return DCX_E_ARG;
    }
}

// pixel (iy, ix) of an h x w image of the NORMALISED, zero-padded plane (net.py pads the normalised image; model_utils.py:19-36
// pads a patch with 0): the load is clamped into the image and its value dropped outside.  pitch in BYTES.
template <class PX>
__device__ __forceinline__ float dcx_px_padded(const uint8_t* img, int pitch, int h, int w, int iy, int ix) {
    const bool inb = (unsigned)iy < (unsigned)h && (unsigned)ix < (unsigned)w;
    const int cy = min(max(iy, 0), h - 1), cx = min(max(ix, 0), w - 1);
    const float v = PX::load(img + (size_t)cy * pitch + (size_t)cx * PX::BPP);
    return inb ? v : 0.0f;
}

// LDS image of a first layer's parameters: [tap][64] | bias | alpha | beta, read as float4 per channel quad.
// All 256 threads of the workgroup call it; the caller's barrier follows.
constexpr int kConv1LdsFloats = 9 * 64 + 3 * 64;
__device__ __forceinline__ void dcx_conv1_stage(float* sw, const float* __restrict__ w9x64, const float* __restrict__ bias,
                                                const float* __restrict__ alpha, const float* __restrict__ beta) {
    const int tid = threadIdx.x;
    for (int i = tid; i < 9 * 64; i += 256) sw[i] = w9x64[i];
    if (tid < 64) {
        sw[576 + tid] = bias[tid];
        sw[640 + tid] = alpha[tid];
        sw[704 + tid] = beta[tid];
    }
}

// channel quad cq of one output pixel from its nine taps x (dy-major): acc = fmaf(w[tap], x[tap], acc) for tap = 0..8, then
// + bias, BN affine (one fmaf), ReLU -- net.py:23-24,60 / refinenet.py:21-22,56
__device__ __forceinline__ float4 dcx_conv1_quad(const float4* sw4, const float (&x)[9], int cq) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const float4 wv = sw4[t * 16 + cq];
        acc.x = fmaf(wv.x, x[t], acc.x);
        acc.y = fmaf(wv.y, x[t], acc.y);
        acc.z = fmaf(wv.z, x[t], acc.z);
        acc.w = fmaf(wv.w, x[t], acc.w);
    }
    const float4 bi = sw4[144 + cq], al = sw4[160 + cq], be = sw4[176 + cq];
    float4 y;
    y.x = fmaxf(fmaf(acc.x + bi.x, al.x, be.x), 0.f);
    y.y = fmaxf(fmaf(acc.y + bi.y, al.y, be.y), 0.f);
    y.z = fmaxf(fmaf(acc.z + bi.z, al.z, be.z), 0.f);
    y.w = fmaxf(fmaf(acc.w + bi.w, al.w, be.w), 0.f);
    return y;
}

// the pipeline's control words (pool cursor, frame tickets), cleared by the first workgroup of the detector's conv1a
__device__ __forceinline__ void dcx_zero_words(int32_t* __restrict__ zero_words, int n_zero) {
    if (zero_words != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0)
        for (int i = threadIdx.x; i < n_zero; i += 256) zero_words[i] = 0;
}
