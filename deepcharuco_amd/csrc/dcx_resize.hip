// dcx_resize.hip -- cv2.resize of a batch of u8 gray or interleaved BGR frames: INTER_NEAREST, INTER_LINEAR (cv2's 11-bit fixed
// point scheme, with its rule that an exact 2 x 2 reduction is INTER_AREA's), INTER_AREA by integer factors and, through an entry
// of its own, INTER_AREA for shrinking by any factor.  The step in front of the detector: camera frames -> the 320 x 240 the
// networks are trained on.  deepcharuco_amd/resize.py:resize_host states every formula and is the pin of this file, bit for bit;
// the formulas are cv2's as published and are not pinned against cv2.
//
// Shape.  The work is memory bound: a 6 x 6 reduction reads 36 source bytes per byte it writes.  One workgroup makes `tw`
// consecutive pixels of ONE output row of one frame (grid: tiles of a row, output rows, frames).  The source bytes these pixels
// need are, per source row, one contiguous span, and the rows are few: fy rows for "area", the two tap rows for "linear" (one
// where both taps clip to the same row; the rows in between are never read), one for "nearest".
//
//   stage     the spans go to LDS in 16-byte chunks cut at the multiples of 16 of the GLOBAL address, so a chunk that lies wholly
//             inside a span is one global_load_dwordx4 whatever the base address and the pitch are; the two chunks that a span's
//             ends cut are put together from byte loads of the bytes inside the span only.  No byte outside a row's span is read,
//             and each byte of a span is read once.
//   compute   a thread per output byte (pixel, channel), consecutive lanes consecutive bytes of the dense output row, so the byte
//             stores of a wave are one contiguous run.  The taps come from LDS; interleaved BGR is read as it stands.
//
// Two kernels.  dcx_resize_u8_kernel stages the bytes themselves (LDS byte r * lrow + (address & 15) + j is byte j of row r's
// span) and serves every mode at every pitch.  Where the pitch is a multiple of 16 the fy rows of an "area" span are cut at the
// same places, and dcx_resize_area_kernel adds them up in registers as they arrive (a thread keeps one chunk's sixteen column sums
// as u16 pairs: fy <= 64 rows of at most 255) and stages the SUMS: fy times fewer LDS writes, fx LDS reads per output byte instead
// of fx fy, and two rows' worth of LDS instead of fy.  Integer sums, so both paths give the same bits.
//
// The coefficients of "linear" and the source index of "nearest" are evaluated per thread in the roundings of the host
// definition: every fp64 / fp32 step through an _rn intrinsic, so nothing contracts into a fused multiply-add.  The scales
// 1.0 / (dn / sn) are computed by the host entry in double and are kernel arguments.
//
// "area_any" (dcx_resize_area_u8: cv2's general INTER_AREA, a box filter with fractional end taps) routes integer factors on both
// axes to the "area" kernels above and takes everything else through dcx_resize_u8_kernel<CH, kAreaAny>: the rows of the output
// row's y-taps (at most 66) and the span from the first x-tap of the tile's first pixel to the last x-tap of its last one are
// staged as bytes; a thread evaluates the tap table of its own pixel in x and of the output row in y (area_taps: a first tap, a
// run of whole pixels of one weight, a last tap) and then, per staged row, the float32 sum over its x-taps in order, weighted
// and added in row order, every product and sum rounded on its own (compiled with contraction off).  The u16 column sums of
// dcx_resize_area_kernel do not carry over: the definition rounds every row's horizontal sum before it is weighted.
//
// No workspace, no atomics, no allocation, no synchronisation: one launch on the stream, capturable in a hipGraph.
#include "dcx_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxSide = 32768;              // every dimension and the batch: 1 .. kMaxSide
constexpr int kMaxFactor = 64;               // "area": integer factors 1 .. kMaxFactor
constexpr int kMaxElems = 1024;              // output bytes of one workgroup: at most four per thread
constexpr int kLdsBytes = 40960;             // staged spans of one workgroup: four workgroups share a CU's 160 KiB
constexpr int kInFlight = 4;                 // 16-byte chunks a thread loads before it stores them
constexpr int kCoefBits = 11;                // INTER_RESIZE_COEF_BITS: the coefficients are rint(w * 2048)

enum { kNearest = 0, kLinear = 1, kArea = 2 };  // dcx_resize_u8's codes
constexpr int kAreaAny = 3;                  // the general path of dcx_resize_area_u8: a kernel mode, no code of dcx_resize_u8
constexpr double kAreaEps = 1e-3;            // "area_any": an end tap that covers no more of its pixel is dropped

struct ResizeArgs {
    const uint8_t* src;
    uint8_t* out;
    long frame_stride;
    int pitch, src_h, src_w, out_h, out_w;
    int tw;                                  // output pixels of one workgroup
    int lrow;                                // chunks of one staged row * 16: at least 16 more than the longest span
    int fx, fy;                              // "area"
    int rows;                                // "area_any": the staged rows of one workgroup (the y-taps of an output row are fewer)
    float inv_area;                          // "area": float32(1.0 / (fx fy))
    double scale_x, scale_y;                 // 1.0 / (dn / sn)
};

// "nearest": min(floor(d * scale), sn - 1), fp64
__device__ __forceinline__ int nearest_index(int d, double scale, int sn) {
    return min((int)floor(__dmul_rn((double)d, scale)), sn - 1);
}

// "linear" along one axis: the two taps and their 11-bit coefficients (resize_host's roundings, step by step)
template <bool X>
__device__ __forceinline__ void linear_taps(int d, double scale, int sn, int& s0, int& s1, int& c0, int& c1) {
    float f = (float)__dadd_rn(__dmul_rn((double)d + 0.5, scale), -0.5);         // (d + 0.5 is exact)
    int s = (int)floorf(f);
    f = __fsub_rn(f, (float)s);
    if (X) {
        if (s < 0) { f = 0.f; s = 0; }
        if (s >= sn - 1) { f = 0.f; s = sn - 1; }
        s0 = s;
        s1 = min(s + 1, sn - 1);
    } else {
        s0 = min(max(s, 0), sn - 1);
        s1 = min(max(s + 1, 0), sn - 1);
    }
    const float one = (float)(1 << kCoefBits);
    c0 = (int)rintf(__fmul_rn(__fsub_rn(1.f, f), one));
    c1 = (int)rintf(__fmul_rn(f, one));
}

// "area_any" along one axis (resize_host's roundings, step by step): the taps of output index d are the n source pixels s0,
// s0 + 1, ...: the fractional first one if there is one, the whole ones, the fractional last one if there is one.  Held as the
// loops take them (no weight is looked up by position): tap 0 has weight w0, taps 1 .. body - 1 are whole pixels of weight w_mid,
// and where n > max(body, 1) tap n - 1 is the last one, of weight w_last.
struct AreaTaps {
    int s0, n, body;
    float w0, w_mid, w_last;
    __device__ __forceinline__ bool has_last() const { return n > max(body, 1); }
};

__device__ __forceinline__ AreaTaps area_taps(int d, double scale, int sn) {
    // Plain operators with contraction off: the _rn intrinsics are plain operators compiled with contraction allowed, and once
    // they are inlined a product and the sum behind it do fuse (f1 + scale became fma(d, scale, scale)).
#pragma clang fp contract(off)
    const double f1 = (double)d * scale, f2 = f1 + scale;
    const double cell = fmin(scale, (double)sn - f1);
    const int s2 = min((int)floor(f2), sn - 1), s1 = min((int)ceil(f1), s2);
    const double head = (double)s1 - f1, tail = f2 - (double)s2;
    const int first = head > kAreaEps, last = tail > kAreaEps;
    AreaTaps t;
    t.s0 = s1 - first;
    t.body = first + (s2 - s1);
    t.n = t.body + last;
    t.w_mid = (float)(1.0 / cell);
    t.w_last = (float)(fmin(fmin(tail, 1.0), cell) / cell);
    t.w0 = first ? (float)(head / cell) : (t.body ? t.w_mid : t.w_last);
    return t;
}

// Bytes [lo, lo + 16) of the span that begins at g (g + lo is a multiple of 16), of which only [0, span) exist (a chunk that an end
// of the span cuts): the existing ones byte by byte (sixteen independent predicated loads, no loop), zeros for the others.
__device__ __forceinline__ uint4 load_cut_chunk(const uint8_t* g, int lo, int span) {
    unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int k = lo + j;
        if (k >= 0 && k < span) w[j >> 2] |= (unsigned)g[k] << (8 * (j & 3));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ bool whole_chunk(int lo, int span) { return lo >= 0 && lo + 16 <= span; }

__device__ __forceinline__ unsigned area_value(unsigned sum, const ResizeArgs& a) {
    return (a.fx == 2 && a.fy == 2) ? (sum + 2) >> 2 : (unsigned)(int)rintf(__fmul_rn((float)sum, a.inv_area));
}

template <int CH, int MODE>
__global__ __launch_bounds__(kThreads) void dcx_resize_u8_kernel(ResizeArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x;
    const int px0 = blockIdx.x * a.tw, npx = min(a.tw, a.out_w - px0), oy = blockIdx.y;
    const uint8_t* frame = a.src + (size_t)blockIdx.z * a.frame_stride;

    // the source rows this output row needs, and the pixels [xlo, xhi] of them that its npx pixels need
    int nr, y0 = 0, y1 = 0, b0 = 0, b1 = 0, xlo, xhi;
    AreaTaps ty{};
    if (MODE == kAreaAny) {
        ty = area_taps(oy, a.scale_y, a.src_h);                                 // (the same for every thread)
        nr = min(ty.n, a.rows);
        y0 = ty.s0;
        xlo = area_taps(px0, a.scale_x, a.src_w).s0;                            // the taps never decrease along the row
        const AreaTaps t = area_taps(px0 + npx - 1, a.scale_x, a.src_w);
        xhi = t.s0 + t.n - 1;
    } else if (MODE == kArea) {
        nr = a.fy;
        y0 = oy * a.fy;
        xlo = px0 * a.fx;
        xhi = (px0 + npx) * a.fx - 1;
    } else if (MODE == kLinear) {
        linear_taps<false>(oy, a.scale_y, a.src_h, y0, y1, b0, b1);
        nr = y1 != y0 ? 2 : 1;
        int t0, t1, t2, t3;
        linear_taps<true>(px0, a.scale_x, a.src_w, xlo, t0, t1, t2);            // the taps never decrease along the row
        linear_taps<true>(px0 + npx - 1, a.scale_x, a.src_w, t0, xhi, t1, t3);
    } else {
        nr = 1;
        y0 = nearest_index(oy, a.scale_y, a.src_h);
        xlo = nearest_index(px0, a.scale_x, a.src_w);
        xhi = nearest_index(px0 + npx - 1, a.scale_x, a.src_w);
    }
    const int span = min((xhi - xlo + 1) * CH, a.lrow - 16);                    // (the host sized lrow for the longest span)
    const int nchunk = a.lrow >> 4;
    auto row_start = [&](int r) -> const uint8_t* {
        const int y = MODE == kArea || MODE == kAreaAny ? y0 + r : (r ? y1 : y0);
        return frame + (size_t)y * a.pitch + (size_t)xlo * CH;
    };

    // ---- stage: kInFlight chunks per thread are loaded before the first is stored
    const int total = nr * nchunk;
    for (int i0 = tid; i0 < total; i0 += kThreads * kInFlight) {
        uint4 v[kInFlight];
        int at[kInFlight];
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
            const int i = i0 + u * kThreads;
            const int r = i / nchunk, c = i - r * nchunk;
            const uint8_t* g = row_start(min(r, nr - 1));
            const int lo = c * 16 - (int)((uintptr_t)g & 15);                    // the chunk's first byte within the span
            at[u] = -1;
            if (i < total && lo < span && lo + 16 > 0) {
                at[u] = r * a.lrow + c * 16;
                v[u] = whole_chunk(lo, span) ? *reinterpret_cast<const uint4*>(g + lo) : load_cut_chunk(g, lo, span);
            }
        }
#pragma unroll
        for (int u = 0; u < kInFlight; ++u)
            if (at[u] >= 0) *reinterpret_cast<uint4*>(lds + at[u]) = v[u];
    }
    __syncthreads();

    // ---- compute: one output byte per thread and round
    uint8_t* orow = a.out + (((size_t)blockIdx.z * a.out_h + oy) * a.out_w + px0) * CH;
    const int off0 = (int)((uintptr_t)row_start(0) & 15);
    for (int e = tid; e < npx * CH; e += kThreads) {
        const int p = e / CH, c = e - p * CH;
        unsigned o;
        if (MODE == kAreaAny) {
#pragma clang fp contract(off)                                                   // (as in area_taps: every product and sum on its own)
            const AreaTaps tx = area_taps(px0 + p, a.scale_x, a.src_w);
            const int i0 = (tx.s0 - xlo) * CH + c;
            auto hsum = [&](int r) -> float {                                   // staged row r over the x-taps in order
#pragma clang fp contract(off)
                const uint8_t* row = lds + r * a.lrow + (int)((uintptr_t)row_start(r) & 15) + i0;
                float h = (float)row[0] * tx.w0;
                for (int k = 1; k < tx.body; ++k) h = h + (float)row[k * CH] * tx.w_mid;
                if (tx.has_last()) h = h + (float)row[(tx.n - 1) * CH] * tx.w_last;
                return h;
            };
            float v = ty.w0 * hsum(0);                                          // horizontal first, then vertical: the host's order
            for (int r = 1; r < ty.body; ++r) v = v + ty.w_mid * hsum(r);
            if (ty.has_last()) v = v + ty.w_last * hsum(ty.n - 1);
            o = (unsigned)(int)fminf(fmaxf(rintf(v), 0.f), 255.f);
        } else if (MODE == kArea) {
            unsigned sum = 0;
            for (int r = 0; r < a.fy; ++r) {
                const uint8_t* row = lds + r * a.lrow + (int)((uintptr_t)row_start(r) & 15) + p * a.fx * CH + c;
                for (int k = 0; k < a.fx; ++k) sum += row[k * CH];
            }
            o = area_value(sum, a);
        } else if (MODE == kLinear) {
            int x0, x1, a0, a1;
            linear_taps<true>(px0 + p, a.scale_x, a.src_w, x0, x1, a0, a1);
            const uint8_t* r0 = lds + off0 + c;
            const uint8_t* r1 = nr == 2 ? lds + a.lrow + (int)((uintptr_t)row_start(1) & 15) + c : r0;
            const int i0 = (x0 - xlo) * CH, i1 = (x1 - xlo) * CH;
            const int h0 = (int)r0[i0] * a0 + (int)r0[i1] * a1;
            const int h1 = (int)r1[i0] * a0 + (int)r1[i1] * a1;
            o = (unsigned)((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2);
        } else {
            o = lds[off0 + (nearest_index(px0 + p, a.scale_x, a.src_w) - xlo) * CH + c];
        }
        orow[e] = (uint8_t)o;
    }
}

// "area" where the pitch is a multiple of 16: every row of the span is cut into the same chunks, and a thread adds its chunk up
// over the fy rows.  A dword of a chunk holds bytes 0..3; its bytes 0 and 2 are summed in the halves of one u32 (`even`) and its
// bytes 1 and 3 in those of another (`odd`), and the four sums are stored as u16 in the bytes' order: LDS u16 (address & 15) + j
// is the sum of column j of the span.
template <int CH>
__global__ __launch_bounds__(kThreads) void dcx_resize_area_kernel(ResizeArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x;
    const int px0 = blockIdx.x * a.tw, npx = min(a.tw, a.out_w - px0), oy = blockIdx.y;
    const uint8_t* g0 = a.src + (size_t)blockIdx.z * a.frame_stride + (size_t)(oy * a.fy) * a.pitch + (size_t)px0 * a.fx * CH;
    const int off = (int)((uintptr_t)g0 & 15);
    const int span = min(npx * a.fx * CH, a.lrow - 16);
    const int nchunk = a.lrow >> 4;

    for (int c = tid; c < nchunk; c += kThreads) {
        const int lo = c * 16 - off;
        if (lo >= span || lo + 16 <= 0) continue;
        unsigned even[4] = {0u, 0u, 0u, 0u}, odd[4] = {0u, 0u, 0u, 0u};
        auto add = [&](const uint4& v) {
            const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                even[k] += w[k] & 0x00ff00ffu;
                odd[k] += (w[k] >> 8) & 0x00ff00ffu;
            }
        };
        if (whole_chunk(lo, span)) {
#pragma unroll 4
            for (int r = 0; r < a.fy; ++r) add(*reinterpret_cast<const uint4*>(g0 + (size_t)r * a.pitch + lo));
        } else {
#pragma unroll 1
            for (int r = 0; r < a.fy; ++r) add(load_cut_chunk(g0 + (size_t)r * a.pitch, lo, span));
        }
        unsigned lo2[4], hi2[4];                                                  // sums of bytes (0, 1) and (2, 3) of each dword
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lo2[k] = (even[k] & 0xffffu) | (odd[k] << 16);
            hi2[k] = (even[k] >> 16) | (odd[k] & 0xffff0000u);
        }
        reinterpret_cast<uint4*>(lds)[2 * c] = make_uint4(lo2[0], hi2[0], lo2[1], hi2[1]);
        reinterpret_cast<uint4*>(lds)[2 * c + 1] = make_uint4(lo2[2], hi2[2], lo2[3], hi2[3]);
    }
    __syncthreads();

    const unsigned short* sums = reinterpret_cast<const unsigned short*>(lds);
    uint8_t* orow = a.out + (((size_t)blockIdx.z * a.out_h + oy) * a.out_w + px0) * CH;
    for (int e = tid; e < npx * CH; e += kThreads) {
        const int p = e / CH, c = e - p * CH;
        const unsigned short* col = sums + off + p * a.fx * CH + c;
        unsigned sum = 0;
        for (int k = 0; k < a.fx; ++k) sum += col[k * CH];
        orow[e] = (uint8_t)area_value(sum, a);
    }
}

// LDS bytes of one staged row that holds up to `pixels` pixels at any alignment
inline int lds_row(long long pixels, int ch) { return (int)((pixels * ch + 15 + 15) & ~15LL) + 16; }

// both entries: `mode` is a code of dcx_resize_u8 or kAreaAny
int resize_u8(const uint8_t* d_src, long frame_stride, int pitch, int src_h, int src_w, int channels, int out_h, int out_w, int batch,
              int mode, uint8_t* d_out, void* stream) {
    if (!d_src || !d_out || frame_stride < 0) return DCX_E_ARG;
    if (channels != 1 && channels != 3) return DCX_E_ARG;
    if (mode != kNearest && mode != kLinear && mode != kArea && mode != kAreaAny) return DCX_E_ARG;
    for (int v : {src_h, src_w, out_h, out_w, batch})
        if (v < 1 || v > kMaxSide) return DCX_E_SHAPE;
    if ((long long)pitch < (long long)src_w * channels || (long long)pitch * src_h > 0x7fffffffLL) return DCX_E_SHAPE;
    if (mode == kLinear && src_w == 2 * out_w && src_h == 2 * out_h) mode = kArea;           // cv2's rule
    if (mode == kAreaAny) {
        if (out_h > src_h || out_w > src_w) return DCX_E_SHAPE;                               // area does not enlarge
        if (src_h > kMaxFactor * out_h || src_w > kMaxFactor * out_w) return DCX_E_SHAPE;
        if (src_w % out_w == 0 && src_h % out_h == 0) mode = kArea;                           // cv2's fast-path rule
    }
    ResizeArgs a{};
    a.src = d_src; a.out = d_out; a.frame_stride = frame_stride;
    a.pitch = pitch; a.src_h = src_h; a.src_w = src_w; a.out_h = out_h; a.out_w = out_w;
    a.scale_x = 1.0 / ((double)out_w / (double)src_w);
    a.scale_y = 1.0 / ((double)out_h / (double)src_h);
    int rows;                                                                                 // staged rows, in units of lrow bytes
    bool sums = false;
    if (mode == kArea) {
        a.fx = src_w / out_w;
        a.fy = src_h / out_h;
        if (a.fx * out_w != src_w || a.fy * out_h != src_h || a.fx > kMaxFactor || a.fy > kMaxFactor) return DCX_E_SHAPE;
        a.inv_area = (float)(1.0 / (double)(a.fx * a.fy));
        sums = pitch % 16 == 0;
        rows = sums ? 2 : a.fy;                                                               // (u16 sums: two bytes per column)
    } else if (mode == kAreaAny) {
        // the rows s1 - 1 .. s2 of a cell: s2 - s1 <= f2 - f1, and ceil() covers a scale within an ulp of the integer above it
        rows = (int)ceil(a.scale_y) + 2;
        if (rows > src_h) rows = src_h;
        a.rows = rows;
    } else {
        rows = mode == kLinear ? 2 : 1;
    }
    // the widest tile whose staged rows fit: (tw - 1) * scale + 4 bounds the pixels between the first tap of a tile's first pixel
    // and the last tap of its last one ("linear": floor(f_last) + 1 - floor(f_first) + 1, and one more for f's float rounding;
    // "area_any": floor(f2_last) - floor(f1_first) + 1 with f2_last - f1_first = tw * scale, and one more for their roundings)
    auto span_px = [&](int tw) -> long long {
        if (mode == kArea) return (long long)tw * a.fx;
        const long long n = (long long)ceil((double)(mode == kAreaAny ? tw : tw - 1) * a.scale_x) + (mode == kAreaAny ? 3 : 4);
        return n < src_w ? n : src_w;
    };
    int tw = out_w < kMaxElems / channels ? out_w : kMaxElems / channels;
    while (tw > 1 && (long long)rows * lds_row(span_px(tw), channels) > kLdsBytes) tw = (tw + 1) / 2;
    a.tw = tw;
    a.lrow = lds_row(span_px(tw), channels);
    const size_t lds_bytes = (size_t)rows * a.lrow;
    if (lds_bytes > 65536) return DCX_E_SHAPE;                                                // (cannot happen within the limits above)
    const dim3 grid((unsigned)((out_w + tw - 1) / tw), (unsigned)out_h, (unsigned)batch);
    if ((unsigned long long)grid.x * grid.y * grid.z * kThreads > 0xffffffffULL) return DCX_E_SHAPE;
#define DCX_RESIZE(KERNEL) hipLaunchKernelGGL(KERNEL, grid, dim3(kThreads), lds_bytes, (hipStream_t)stream, a)
    if (channels == 1) {
        if (sums) DCX_RESIZE((dcx_resize_area_kernel<1>));
        else if (mode == kArea) DCX_RESIZE((dcx_resize_u8_kernel<1, kArea>));
        else if (mode == kAreaAny) DCX_RESIZE((dcx_resize_u8_kernel<1, kAreaAny>));
        else if (mode == kLinear) DCX_RESIZE((dcx_resize_u8_kernel<1, kLinear>));
        else DCX_RESIZE((dcx_resize_u8_kernel<1, kNearest>));
    } else {
        if (sums) DCX_RESIZE((dcx_resize_area_kernel<3>));
        else if (mode == kArea) DCX_RESIZE((dcx_resize_u8_kernel<3, kArea>));
        else if (mode == kAreaAny) DCX_RESIZE((dcx_resize_u8_kernel<3, kAreaAny>));
        else if (mode == kLinear) DCX_RESIZE((dcx_resize_u8_kernel<3, kLinear>));
        else DCX_RESIZE((dcx_resize_u8_kernel<3, kNearest>));
    }
#undef DCX_RESIZE
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int dcx_resize_u8(const uint8_t* d_src, long frame_stride, int pitch, int src_h, int src_w, int channels, int out_h,
                             int out_w, int batch, int interpolation, uint8_t* d_out, void* stream) {
    if (interpolation == kAreaAny) return DCX_E_ARG;                                          // (the other entry's mode)
    return resize_u8(d_src, frame_stride, pitch, src_h, src_w, channels, out_h, out_w, batch, interpolation, d_out, stream);
}

extern "C" int dcx_resize_area_u8(const uint8_t* d_src, long frame_stride, int pitch, int src_h, int src_w, int channels, int out_h,
                                  int out_w, int batch, uint8_t* d_out, void* stream) {
    return resize_u8(d_src, frame_stride, pitch, src_h, src_w, channels, out_h, out_w, batch, kAreaAny, d_out, stream);
}
