// dcx_sgm.hip -- dense stereo matching on rectified u8 pairs: semi-global matching over 9 x 7 census costs (four paths, or
// eight with the diagonals; cv2's uniqueness rule, a left-right check made from the same summed costs, a parabola's sub-pixel
// step in sixteenths), and the disparity map as 3-D points.  deepcharuco_amd/disparity.py restates every step (sgm_host,
// disparity_to_points_host) and is the pin of these kernels: the matcher is integer throughout and agrees with it bit for bit.
//
// Shape.  A candidate disparity is a lane: a wave owns one path line (a row of a frame for the two horizontal paths, a column for
// the two vertical ones) and walks it pixel by pixel with the line's L_r(., d) in its lanes, D / 64 consecutive disparities to a
// lane.  One step of the recursion is then two cross-lane shifts by one (the d - 1 and d + 1 neighbours: only a lane's first and
// last disparity need them), one wave minimum (M) and, for the cost, two 32-bit popcounts of an XOR of census words.  No LDS and
// no barrier on that chain.  The cost volume never exists: a step reads the left census word of its pixel (wave-uniform) and the
// right census words at x - m - d (64 * NPL consecutive words, clamped to the row, served by the caches).  Only S (u16,
// H W D 2 B per frame) lives in the workspace:
//
//   census kernel      both frames -> two u64 census images                                    (one thread per pixel)
//   path kernel, rows  left -> right writes S = L; right -> left by the same wave adds its L   (S: one write, one update that the
//                                                                                               wave's own lanes wrote and L2 holds)
//   path kernel, cols  top -> bottom adds, bottom -> top adds                                  (S: two updates)
//   diagonal kernel    paths == 8 only, one launch per family: "\" (+1, +1) adds, (-1, -1) adds;   (S: two updates per launch)
//                      "/" (+1, -1) adds, (-1, +1) adds
//   select kernel      one workgroup per row reads S once: a wave per pixel finds the winner (one wave minimum of S << 16 | d,
//                      so ties take the lowest d), the uniqueness verdict (a ballot) and the sub-pixel step, and every lane
//                      folds its S into the right view's winner of ITS right pixel, x - m - d, by an LDS minimum of the same
//                      packed word (order-free, so deterministic); after a barrier a thread per pixel makes the left-right
//                      check against that row of right-view winners and stores the int16.
//
// A step's loads (census words, and S where it is updated) do not depend on the recursion, so each pass loads pixel p + 1's
// before it computes pixel p.  What is left on the chain is the shifts, the wave minimum and a handful of integer operations;
// throughput comes from the lines in flight (B H or B W waves).
//
// The diagonal paths.  A wave per START COLUMN c, not per diagonal: at row y the wave stands on column (c + slope y) mod W, slope
// +1 for the "\" family and -1 for "/", so it walks all H rows like a column wave and every launch is B W waves of H steps,
// whatever the lengths (1 ... min(H, W)) of the frame's H + W - 1 diagonals are.  Where the column wraps across the frame edge
// the previous pixel of the path lies outside the frame, and the recursion starts again (L = C) as it does on a line's first
// pixel: the wave carries one diagonal after another, end to end.  The reverse pass walks the same pixels from the last row up
// and starts again where it wraps the other way.  W = 1 wraps at every step (every diagonal has one pixel), H = 1 is one step,
// and a tall frame wraps several times: none needs a launch of its own.  The waves of a workgroup stand on adjacent pixels of
// S at every step, as in the column pass.
//
// Updating S in place is safe because, WITHIN ONE LAUNCH, EVERY ELEMENT OF S IS READ AND WRITTEN BY EXACTLY ONE WAVE, and by
// the same lane of it in both passes: rows and columns partition a frame, and c -> (c + slope y) mod W is a bijection of the
// columns at every row y, so the start-column lines do too.  A wave's reverse pass touches only what its own lanes stored in its
// forward pass (program order; nothing else in the launch reads or writes those addresses).  The two diagonal families visit the
// same pixels from different lines, as rows and columns do, which is why each is a launch of its own and the stream orders them.
//
// No allocation, no synchronisation, no global atomics; every call is a fixed sequence of launches on the stream.
#include <cmath>

#include "dcx_common.h"

namespace {

constexpr int kCensusRX = 4, kCensusRY = 3;      // the census window is 9 wide, 7 tall
constexpr int kMaxWidth = 4096;                  // the select kernel keeps 8 B of LDS per pixel of a row
constexpr int kMaxHeight = 32768;
constexpr int kMaxChunk = 16384;                 // frames of one chunk (the census grid's z is 2 per frame)
constexpr int kBig = 1 << 20;                    // stands for a neighbour d +- 1 outside [0, D): never the minimum

// ---- cross-lane

// One step of a wave minimum: v against the lane that the DPP control names.  A lane whose source is disabled or out of range
// keeps its own value (old = v), which a minimum ignores.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned min_dpp(unsigned v) {
    return min(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, ROW_MASK, 0xf, false));
}

// The minimum over the 64 lanes, in every lane (all 64 must be active): within quads, within rows of 16 by rotation, then row 0
// into row 1 and row 2 into row 3 (row_bcast:15), rows 0-1 into rows 2-3 (row_bcast:31); lane 63 holds the result.
__device__ __forceinline__ unsigned wave_min(unsigned v) {
    v = min_dpp<0xb1, 0xf>(v);       // quad_perm:[1,0,3,2]
    v = min_dpp<0x4e, 0xf>(v);       // quad_perm:[2,3,0,1]
    v = min_dpp<0x124, 0xf>(v);      // row_ror:4
    v = min_dpp<0x128, 0xf>(v);      // row_ror:8
    v = min_dpp<0x142, 0xa>(v);      // row_bcast:15 into rows 1 and 3
    v = min_dpp<0x143, 0xc>(v);      // row_bcast:31 into rows 2 and 3
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

// ---- a lane's NPL consecutive u16 of S as one access

template <int NPL>
__device__ __forceinline__ void load_s(const uint16_t* p, int (&v)[NPL]) {
    if constexpr (NPL == 1) {
        v[0] = *p;
    } else if constexpr (NPL == 2) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
        v[0] = w & 0xffff; v[1] = w >> 16;
    } else {
        const uint2 w = *reinterpret_cast<const uint2*>(p);
        v[0] = w.x & 0xffff; v[1] = w.x >> 16; v[2] = w.y & 0xffff; v[3] = w.y >> 16;
    }
}

template <int NPL>
__device__ __forceinline__ void store_s(uint16_t* p, const int (&v)[NPL]) {
    if constexpr (NPL == 1) {
        *p = (uint16_t)v[0];
    } else if constexpr (NPL == 2) {
        *reinterpret_cast<uint32_t*>(p) = (uint32_t)v[0] | (uint32_t)v[1] << 16;
    } else {
        *reinterpret_cast<uint2*>(p) = make_uint2((uint32_t)v[0] | (uint32_t)v[1] << 16, (uint32_t)v[2] | (uint32_t)v[3] << 16);
    }
}

// ---- census: one thread per pixel of either frame (grid z = 2 * frame + side)

__global__ __launch_bounds__(256) void dcx_sgm_census_kernel(const uint8_t* __restrict__ left, long frame_stride_l, int pitch_l,
                                                               const uint8_t* __restrict__ right, long frame_stride_r, int pitch_r,
                                                               int height, int width, uint64_t* __restrict__ cen_l,
                                                               uint64_t* __restrict__ cen_r) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= width || y >= height) return;
    const int f = blockIdx.z >> 1, side = blockIdx.z & 1;
    const uint8_t* img = side ? right + (size_t)f * frame_stride_r : left + (size_t)f * frame_stride_l;
    const int pitch = side ? pitch_r : pitch_l;
    const unsigned c = img[(size_t)y * pitch + x];
    uint64_t w = 0;
#pragma unroll
    for (int dy = -kCensusRY; dy <= kCensusRY; ++dy) {
        const uint8_t* row = img + (size_t)min(max(y + dy, 0), height - 1) * pitch;           // edge replication: clamped taps
#pragma unroll
        for (int dx = -kCensusRX; dx <= kCensusRX; ++dx) {
            if (dy == 0 && dx == 0) continue;
            w = (w << 1) | (uint64_t)(row[min(max(x + dx, 0), width - 1)] < c);
        }
    }
    (side ? cen_r : cen_l)[((size_t)f * height + y) * width + x] = w;
}

// ---- the paths

// One line's geometry: pixel p of the line is pixel `base + p * step` of the chunk; its image column is x0 + p * dx and its row
// starts at pixel row0 + p * drow of the chunk.  A wrapped line (sgm_pass<..., WRAP>) has the column (x0 + p * dx) mod width and
// its pixel at row start + column; base and step are not read.
struct Line {
    size_t base, step, row0, drow;
    int x0, dx, n;
};

template <int NPL>
struct Fetch {                       // what a step reads from memory: nothing of it depends on the recursion
    uint64_t cl;
    uint64_t cr[NPL];
    int s[NPL];
};

template <int NPL, bool ACC>
__device__ __forceinline__ Fetch<NPL> fetch(const Line& ln, int p, int lane, const uint64_t* __restrict__ cen_l,
                                            const uint64_t* __restrict__ cen_r, const uint16_t* S, int width, int m) {
    Fetch<NPL> f = {};
    const size_t row = ln.row0 + (size_t)p * ln.drow;
    const int x = ln.x0 + p * ln.dx;
    f.cl = cen_l[row + x];
#pragma unroll
    for (int k = 0; k < NPL; ++k) f.cr[k] = cen_r[row + min(max(x - m - lane * NPL - k, 0), width - 1)];
    if (ACC) load_s<NPL>(S + (ln.base + (size_t)p * ln.step) * (64 * NPL) + lane * NPL, f.s);
    return f;
}

// Pixel p of a wrapped line, whose column x the caller keeps: the same reads as fetch's.
template <int NPL, bool ACC>
__device__ __forceinline__ Fetch<NPL> fetch_wrapped(const Line& ln, int p, int x, int lane, const uint64_t* __restrict__ cen_l,
                                                    const uint64_t* __restrict__ cen_r, const uint16_t* S, int width, int m) {
    Fetch<NPL> f = {};
    const size_t row = ln.row0 + (size_t)p * ln.drow;
    f.cl = cen_l[row + x];
#pragma unroll
    for (int k = 0; k < NPL; ++k) f.cr[k] = cen_r[row + min(max(x - m - lane * NPL - k, 0), width - 1)];
    if (ACC) load_s<NPL>(S + (row + x) * (64 * NPL) + lane * NPL, f.s);
    return f;
}

// One path along the line: REVERSE walks it from its last pixel; ACC adds L to S (else S = L).  WRAP: the line is wrapped (Line),
// and the path starts again, L = C, at every pixel that the walk reaches by wrapping across the frame edge (a select after the
// step, not a branch around it: in one block the next step's loads stay ahead of the step, past a branch they sink below it).
// The line's geometry should be wave-uniform in scalar registers: the columns, the wraps and the row addresses are then scalar.
template <int NPL, bool REVERSE, bool ACC, bool WRAP = false>
__device__ __forceinline__ void sgm_pass(const Line& ln, int lane, const uint64_t* __restrict__ cen_l,
                                         const uint64_t* __restrict__ cen_r, uint16_t* S, int width, int m, int p1, int p2) {
    int L[NPL];
    int p = REVERSE ? ln.n - 1 : 0;
    int x = 0, xn = 0;                                                          // WRAP: the columns of pixel p and of the next one,
    bool restart = true, restart_next = false;                                  // and whether the walk wrapped to reach them
    if constexpr (WRAP) {
#pragma unroll
        for (int k = 0; k < NPL; ++k) L[k] = 0;                                 // (a restart is a select, so the first step reads L)
        x = (ln.x0 + p * ln.dx) % width;                                        // (once per pass; the steps add and compare)
        x += x < 0 ? width : 0;
    }
    Fetch<NPL> next = WRAP ? fetch_wrapped<NPL, ACC>(ln, p, x, lane, cen_l, cen_r, S, width, m)
                           : fetch<NPL, ACC>(ln, p, lane, cen_l, cen_r, S, width, m);
#pragma unroll 1
    for (int t = 0; t < ln.n; ++t) {
        const Fetch<NPL> cur = next;
        const int pn = REVERSE ? max(p - 1, 0) : min(p + 1, ln.n - 1);          // (the last step fetches its own pixel again, unused)
        if constexpr (WRAP) {
            xn = x + (REVERSE ? -ln.dx : ln.dx);
            restart_next = xn < 0 || xn >= width;
            xn = pn == p ? x : xn < 0 ? width - 1 : xn >= width ? 0 : xn;       // (the last step stays on its own pixel here too)
        }
        next = WRAP ? fetch_wrapped<NPL, ACC>(ln, pn, xn, lane, cen_l, cen_r, S, width, m)
                    : fetch<NPL, ACC>(ln, pn, lane, cen_l, cen_r, S, width, m);
        int C[NPL];
#pragma unroll
        for (int k = 0; k < NPL; ++k) C[k] = __popcll(cur.cl ^ cur.cr[k]);
        if (!WRAP && t == 0) {
#pragma unroll
            for (int k = 0; k < NPL; ++k) L[k] = C[k];
        } else {
            int lmin = L[0];
#pragma unroll
            for (int k = 1; k < NPL; ++k) lmin = min(lmin, L[k]);
            const int M = (int)wave_min((unsigned)lmin);
            int below = __shfl_up(L[NPL - 1], 1), above = __shfl_down(L[0], 1);
            below = lane == 0 ? kBig : below;                                   // d - 1 < 0 and d + 1 >= D: the term is left out
            above = lane == 63 ? kBig : above;
            int nl[NPL];
#pragma unroll
            for (int k = 0; k < NPL; ++k) {
                const int lo = k ? L[k - 1] : below, hi = k < NPL - 1 ? L[k + 1] : above;
                nl[k] = C[k] + min(min(L[k], min(lo, hi) + p1), M + p2) - M;
            }
#pragma unroll
            for (int k = 0; k < NPL; ++k) L[k] = WRAP && restart ? C[k] : nl[k];    // (one block with no branch: the loads stay ahead of it)
        }
        int o[NPL];
#pragma unroll
        for (int k = 0; k < NPL; ++k) o[k] = ACC ? cur.s[k] + L[k] : L[k];
        store_s<NPL>(S + (WRAP ? ln.row0 + (size_t)p * ln.drow + x : ln.base + (size_t)p * ln.step) * (64 * NPL) + lane * NPL, o);
        p = pn;
        if constexpr (WRAP) {
            x = xn;
            restart = restart_next;
        }
    }
}

// VERT = false: a wave per row, both horizontal paths (S is written, then updated); true: a wave per column, both vertical
// paths (S is updated twice).  In its second pass a lane reads only what it stored itself in the first.
template <int NPL, bool VERT>
__global__ __launch_bounds__(256) void dcx_sgm_path_kernel(const uint64_t* __restrict__ cen_l, const uint64_t* __restrict__ cen_r,
                                                             uint16_t* S, int frames, int height, int width, int m, int p1, int p2) {
    const int lane = threadIdx.x & 63;
    const int per_frame = VERT ? width : height;
    const long long line = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (line >= (long long)frames * per_frame) return;                          // (wave-uniform)
    const int f = (int)(line / per_frame), i = (int)(line - (long long)f * per_frame);
    const size_t frame0 = (size_t)f * height * width;
    Line ln;
    if (VERT) {
        ln.base = frame0 + i; ln.step = (size_t)width; ln.row0 = frame0; ln.drow = (size_t)width; ln.x0 = i; ln.dx = 0; ln.n = height;
    } else {
        ln.base = frame0 + (size_t)i * width; ln.step = 1; ln.row0 = ln.base; ln.drow = 0; ln.x0 = 0; ln.dx = 1; ln.n = width;
    }
    sgm_pass<NPL, false, VERT>(ln, lane, cen_l, cen_r, S, width, m, p1, p2);
    sgm_pass<NPL, true, true>(ln, lane, cen_l, cen_r, S, width, m, p1, p2);
}

// The two diagonal paths of one family, SLOPE = +1: (+1, +1) then (-1, -1); SLOPE = -1: (+1, -1) then (-1, +1).  A wave per start
// column c walks every row y at column (c + SLOPE y) mod width (the file's head has the reasons and the in-place invariant).  The
// wave's index is made a scalar, so the columns, the wraps and the addresses of a step are scalar arithmetic.
template <int NPL, int SLOPE>
__global__ __launch_bounds__(256) void dcx_sgm_diag_kernel(const uint64_t* __restrict__ cen_l, const uint64_t* __restrict__ cen_r,
                                                             uint16_t* S, int frames, int height, int width, int m, int p1, int p2) {
    const int lane = threadIdx.x & 63;
    const long long line = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (line >= (long long)frames * width) return;                              // (wave-uniform)
    const int f = (int)(line / width), c = (int)(line - (long long)f * width);
    Line ln;
    ln.base = 0; ln.step = 0; ln.row0 = (size_t)f * height * width; ln.drow = (size_t)width; ln.x0 = c; ln.dx = SLOPE; ln.n = height;
    sgm_pass<NPL, false, true, true>(ln, lane, cen_l, cen_r, S, width, m, p1, p2);
    sgm_pass<NPL, true, true, true>(ln, lane, cen_l, cen_r, S, width, m, p1, p2);
}

// ---- winner, invalidation, sub-pixel: one workgroup per row

template <int NPL>
__global__ __launch_bounds__(256) void dcx_sgm_select_kernel(const uint16_t* __restrict__ S, int width, int m, int uniqueness,
                                                               int lr_max_diff, int16_t* __restrict__ out) {
    constexpr int D = 64 * NPL;
    extern __shared__ unsigned lds[];
    unsigned* right_best = lds;                    // [width]: min over d of S(y, xr + m + d, d) << 16 | d
    unsigned* res = lds + width;                   // [width]: valid << 31 | d* << 16 | the int16 value
    const size_t row = blockIdx.x;
    const uint16_t* s = S + row * width * D;
    const int lane = threadIdx.x & 63, d0 = lane * NPL;
    for (int x = threadIdx.x; x < width; x += 256) right_best[x] = 0xffffffffu;
    __syncthreads();
    for (int x = threadIdx.x >> 6; x < width; x += 4) {                          // a wave per pixel (x is wave-uniform)
        int v[NPL];
        load_s<NPL>(s + (size_t)x * D + d0, v);
        unsigned best = 0xffffffffu;
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
            const unsigned packed = (unsigned)v[k] << 16 | (unsigned)(d0 + k);
            best = min(best, packed);
            const int xr = x - m - d0 - k;
            if (xr >= 0 && xr < width) atomicMin(&right_best[xr], packed);
        }
        best = wave_min(best);
        const int sb = (int)(best >> 16), ds = (int)(best & 0xffff);
        int not_unique = 0;
        unsigned lo = 0xffffffffu, hi = 0xffffffffu;
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
            const int d = d0 + k;
            not_unique |= (d < ds - 1 || d > ds + 1) && v[k] * (100 - uniqueness) < sb * 100;
            lo = d == ds - 1 ? (unsigned)v[k] : lo;
            hi = d == ds + 1 ? (unsigned)v[k] : hi;
        }
        const bool ambiguous = __any(not_unique) != 0;
        lo = wave_min(lo);
        hi = wave_min(hi);
        if (lane == 0) {
            const int xr = x - m - ds;
            const bool valid = !ambiguous && xr >= 0 && xr < width;
            int off = 0;
            if (ds > 0 && ds < D - 1) {
                const int num = (int)lo - (int)hi, den = (int)lo + (int)hi - 2 * sb;
                if (den > 0) {
                    const int a = 16 * num + den, b = 2 * den;
                    off = a / b - ((a % b != 0 && a < 0) ? 1 : 0);               // floor division (b > 0)
                }
            }
            res[x] = (valid ? 0x80000000u : 0u) | (unsigned)ds << 16 | (unsigned)((16 * (m + ds) + off) & 0xffff);
        }
    }
    __syncthreads();
    const int invalid = 16 * (m - 1);
    for (int x = threadIdx.x; x < width; x += 256) {
        const unsigned r = res[x];
        bool valid = (r >> 31) != 0;
        const int ds = (int)((r >> 16) & 0x7fff);
        if (valid && lr_max_diff >= 0) {
            const int dr = (int)(right_best[x - m - ds] & 0xffff);                // (valid: x - m - ds lies in [0, width))
            valid = abs(dr - ds) <= lr_max_diff;
        }
        out[row * width + x] = (int16_t)(valid ? (int)(int16_t)(r & 0xffff) : invalid);
    }
}

// ---- the disparity map as 3-D points: one thread per pixel

struct Q44 {
    double q[16];
};

__global__ __launch_bounds__(256) void dcx_disparity_points_kernel(const int16_t* __restrict__ disp, long long n, int height, int width,
                                                                     int m, Q44 Q, float* __restrict__ xyz) {
#pragma clang fp contract(off)
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int v = disp[idx];
    const double x = (double)(int)(idx % width), y = (double)(int)((idx / width) % height), d = (double)v / 16.0;
    double h[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) h[i] = ((Q.q[4 * i] * x + Q.q[4 * i + 1] * y) + Q.q[4 * i + 2] * d) + Q.q[4 * i + 3];
    const bool ok = v >= 16 * m && v != 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) xyz[3 * idx + i] = ok ? (float)(h[i] / h[3]) : NAN;
}

template <int NPL>
int sgm_launch(const uint8_t* d_left, long frame_stride_l, int pitch_l, const uint8_t* d_right, long frame_stride_r, int pitch_r,
               int batch, int height, int width, int m, int p1, int p2, int uniqueness, int lr_max_diff, int paths,
               int16_t* d_disp16, void* d_workspace, int chunk, hipStream_t stream) {
    const size_t px = (size_t)height * width;
    uint64_t* cen_l = static_cast<uint64_t*>(d_workspace);
    uint64_t* cen_r = cen_l + (size_t)chunk * px;
    uint16_t* S = reinterpret_cast<uint16_t*>(cen_r + (size_t)chunk * px);
    for (int f0 = 0; f0 < batch; f0 += chunk) {
        const int frames = min(chunk, batch - f0);
        hipLaunchKernelGGL(dcx_sgm_census_kernel, dim3((unsigned)((width + 63) / 64), (unsigned)((height + 3) / 4), (unsigned)(2 * frames)),
                           dim3(256), 0, stream, d_left + (size_t)f0 * frame_stride_l, frame_stride_l, pitch_l,
                           d_right + (size_t)f0 * frame_stride_r, frame_stride_r, pitch_r, height, width, cen_l, cen_r);
        hipLaunchKernelGGL((dcx_sgm_path_kernel<NPL, false>), dim3((unsigned)(((long long)frames * height + 3) / 4)), dim3(256), 0, stream,
                           cen_l, cen_r, S, frames, height, width, m, p1, p2);
        hipLaunchKernelGGL((dcx_sgm_path_kernel<NPL, true>), dim3((unsigned)(((long long)frames * width + 3) / 4)), dim3(256), 0, stream,
                           cen_l, cen_r, S, frames, height, width, m, p1, p2);
        if (paths == 8) {
            const dim3 grid((unsigned)(((long long)frames * width + 3) / 4));
            hipLaunchKernelGGL((dcx_sgm_diag_kernel<NPL, 1>), grid, dim3(256), 0, stream, cen_l, cen_r, S, frames, height, width, m, p1, p2);
            hipLaunchKernelGGL((dcx_sgm_diag_kernel<NPL, -1>), grid, dim3(256), 0, stream, cen_l, cen_r, S, frames, height, width, m, p1, p2);
        }
        hipLaunchKernelGGL((dcx_sgm_select_kernel<NPL>), dim3((unsigned)((long long)frames * height)), dim3(256),
                           2 * (size_t)width * sizeof(unsigned), stream, S, width, m, uniqueness, lr_max_diff, d_disp16 + (size_t)f0 * px);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

inline bool sgm_shape_ok(int batch, int height, int width, int num_disparities) {
    return batch >= 1 && height >= 1 && height <= kMaxHeight && width >= 1 && width <= kMaxWidth &&
           (num_disparities == 64 || num_disparities == 128 || num_disparities == 256);
}

inline size_t sgm_frame_bytes(int height, int width, int num_disparities) {
    return (size_t)height * width * (16 + 2 * (size_t)num_disparities);
}

}  // namespace

extern "C" size_t dcx_sgm_workspace_bytes(int batch, int height, int width, int num_disparities) {
    if (!sgm_shape_ok(batch, height, width, num_disparities)) return 0;
    return (size_t)batch * sgm_frame_bytes(height, width, num_disparities);
}

extern "C" int dcx_sgm_u8_paths(const uint8_t* d_left, long frame_stride_l, int pitch_l, const uint8_t* d_right, long frame_stride_r,
                                int pitch_r, int batch, int height, int width, int min_disparity, int num_disparities, int p1, int p2,
                                int uniqueness, int lr_max_diff, int paths, int16_t* d_disp16, void* d_workspace,
                                size_t workspace_bytes, void* stream) {
    if (paths != 4 && paths != 8) return DCX_E_ARG;
    if (!d_left || !d_right || !d_disp16 || ((uintptr_t)d_disp16 & 1) || !d_workspace || ((uintptr_t)d_workspace & 7)) return DCX_E_ARG;
    if (frame_stride_l < 0 || frame_stride_r < 0 || p1 < 0 || p1 > p2 || p2 > 255 || uniqueness < 0 || uniqueness >= 100) return DCX_E_ARG;
    if (!sgm_shape_ok(batch, height, width, num_disparities) || pitch_l < width || pitch_r < width) return DCX_E_SHAPE;
    if (min_disparity < -2047 || min_disparity + num_disparities > 2047) return DCX_E_ARG;        // the int16 output's range
    const size_t fit = workspace_bytes / sgm_frame_bytes(height, width, num_disparities);
    if (fit < 1) return DCX_E_WS;
    size_t chunk = fit < (size_t)batch ? fit : (size_t)batch;                  // frames that one pass takes: the batch, or as many as fit
    if (chunk > (size_t)kMaxChunk) chunk = kMaxChunk;
    const int lr = lr_max_diff < 0 ? -1 : lr_max_diff;
#define DCX_SGM(NPL)                                                                                                             \
    sgm_launch<NPL>(d_left, frame_stride_l, pitch_l, d_right, frame_stride_r, pitch_r, batch, height, width, min_disparity, p1, p2, \
                    uniqueness, lr, paths, d_disp16, d_workspace, (int)chunk, (hipStream_t)stream)
    return num_disparities == 64 ? DCX_SGM(1) : num_disparities == 128 ? DCX_SGM(2) : DCX_SGM(4);
#undef DCX_SGM
}

extern "C" int dcx_sgm_u8(const uint8_t* d_left, long frame_stride_l, int pitch_l, const uint8_t* d_right, long frame_stride_r,
                          int pitch_r, int batch, int height, int width, int min_disparity, int num_disparities, int p1, int p2,
                          int uniqueness, int lr_max_diff, int16_t* d_disp16, void* d_workspace, size_t workspace_bytes,
                          void* stream) {
    return dcx_sgm_u8_paths(d_left, frame_stride_l, pitch_l, d_right, frame_stride_r, pitch_r, batch, height, width, min_disparity,
                            num_disparities, p1, p2, uniqueness, lr_max_diff, 4, d_disp16, d_workspace, workspace_bytes, stream);
}

extern "C" int dcx_disparity_to_points(const int16_t* d_disp16, int batch, int height, int width, int min_disparity,
                                       const double* h_Q16, float* d_xyz, void* stream) {
    if (!d_disp16 || !h_Q16 || !d_xyz || ((uintptr_t)d_disp16 & 1) || ((uintptr_t)d_xyz & 3)) return DCX_E_ARG;
    if (batch < 1 || height < 1 || width < 1) return DCX_E_SHAPE;
    const long long n = (long long)batch * height * width;
    if (n > 0x7fffffffLL * 64) return DCX_E_SHAPE;
    Q44 Q;
    for (int i = 0; i < 16; ++i) {
        Q.q[i] = h_Q16[i];
        if (!std::isfinite(Q.q[i])) return DCX_E_ARG;
    }
    hipLaunchKernelGGL(dcx_disparity_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_disp16, n,
                       height, width, min_disparity, Q, d_xyz);
    return (int)hipGetLastError();
}
