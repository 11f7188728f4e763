// dcx_speckle.hip -- the speckle filter for int16 disparity maps (cv2.filterSpeckles): every pixel of a connected component of at
// most max_speckle_size pixels becomes new_val.  Pixels equal to new_val belong to no component; two 4-neighbours of one frame are
// joined when their values differ by at most max_diff.  deepcharuco_amd/disparity.py:filter_speckles_host states it and is the pin
// of these kernels: all integer, and the result depends on the components' sizes only, so whatever order the unions below happen
// in, the bits are the host's.
//
// Shape.  Connected-component labelling by union-find.  A pixel's label is a pixel index of its frame that never exceeds its own
// (a root holds its own index), so every chain of labels descends to the smallest index that the unions made so far have reached.
// Per frame the workspace holds a 32-bit label and a 32-bit size per pixel:
//
//   tile kernel     a workgroup labels one 32 x 32 tile in LDS: each pixel starts as its own root, is united with its right and
//                   lower neighbour inside the tile (LDS atomicMin), and stores the frame index of its tile root; new_val pixels
//                   store kNone.  It also clears the tile's sizes.
//   border kernel   a thread per pixel pair that straddles a tile edge: the same predicate, a lock-free union on the global labels.
//   count kernel    a thread per pixel: finds its root, stores it as its label and adds 1 to the root's size (one add per wave
//                   and root).
//   apply kernel    out[p] = size[label[p]] <= max_speckle_size ? new_val : in[p]; it reads in[p] before it writes out[p], so
//                   out may be in.
//
// Visibility.  What one phase hands to the next crosses a kernel boundary.  The one phase in which workgroups act on each other's
// words is the border kernel, and there every access to the labels is an agent-scope atomic (a load that bypasses the L1, or an
// atomicMin at the L2) and every decision is taken on the value such an access returned.  In the count kernel a thread following a
// chain may read a label that another thread is replacing by its root: old or new, both lie on the chain to that root.
//
// No waiting.  No kernel waits for another workgroup or thread: no flags, no tickets, no cooperative launch.  Every loop of a find
// or a union ends because the index it holds strictly decreases (commented at each loop).
//
// No allocation, no synchronisation; every call is a fixed sequence of launches on the stream (four per chunk of frames).
#include "dcx_common.h"

namespace {

constexpr int kTile = 32, kTilePx = kTile * kTile;      // tests/test_gpu_speckle.py sizes its cases by kTile
constexpr int kThreads = 256;
constexpr unsigned kNone = 0xffffffffu;                 // the label of a new_val pixel
constexpr long long kMaxPixels = 1LL << 30;             // a frame's pixel indices fit 32 bits with room for kNone
constexpr int kMaxSide = 1 << 20;                       // keeps a frame's tile count (grid x) below 2^21
constexpr int kMaxChunk = 32768;                        // frames of one chunk (grid y)

__device__ __forceinline__ bool joined(int a, int b, int new_val, int max_diff) {
    return a != new_val && b != new_val && abs(a - b) <= max_diff;              // (int16 values: the difference fits an int)
}

// ---- the tile, in LDS

__device__ __forceinline__ unsigned lds_find(unsigned* lab, unsigned a) {
    // ends: a label never exceeds its index, so a strictly decreases until it reaches a root
    for (unsigned p; (p = __hip_atomic_load(&lab[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != a;) a = p;
    return a;
}

__device__ __forceinline__ void lds_unite(unsigned* lab, unsigned a, unsigned b) {
    // ends: max(a, b) strictly decreases from one round to the next (the finds never raise a or b, and `was` < hi)
    for (;;) {
        a = lds_find(lab, a);
        b = lds_find(lab, b);
        if (a == b) return;
        const unsigned hi = max(a, b), lo = min(a, b);
        const unsigned was = __hip_atomic_fetch_min(&lab[hi], lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (was == hi) return;                   // hi was a root and now hangs under lo
        a = was;                                 // hi had been hooked under `was` meanwhile; whichever of `was` and lo the slot
        b = lo;                                  // holds now, the two must still be made one
    }
}

__global__ __launch_bounds__(kThreads) void dcx_speckle_tile_kernel(const int16_t* __restrict__ in, int height, int width, int tiles_x,
                                                                     int new_val, int max_diff, unsigned* __restrict__ labels,
                                                                     unsigned* __restrict__ sizes) {
    __shared__ int val[kTilePx];                 // new_val outside the frame: never joined
    __shared__ unsigned lab[kTilePx];
    const size_t frame0 = (size_t)blockIdx.y * height * width;
    const int x0 = (int)(blockIdx.x % tiles_x) * kTile, y0 = (int)(blockIdx.x / tiles_x) * kTile;
    for (int i = threadIdx.x; i < kTilePx; i += kThreads) {
        const int x = x0 + (i & (kTile - 1)), y = y0 + i / kTile;
        const bool inside = x < width && y < height;
        const size_t p = frame0 + (size_t)y * width + x;
        val[i] = inside ? (int)in[p] : new_val;
        lab[i] = (unsigned)i;
        if (inside) sizes[p] = 0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kTilePx; i += kThreads) {
        const int v = val[i];
        if ((i & (kTile - 1)) < kTile - 1 && joined(v, val[i + 1], new_val, max_diff)) lds_unite(lab, i, i + 1);
        if (i < kTilePx - kTile && joined(v, val[i + kTile], new_val, max_diff)) lds_unite(lab, i, i + kTile);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kTilePx; i += kThreads) {
        const int x = x0 + (i & (kTile - 1)), y = y0 + i / kTile;
        if (x >= width || y >= height) continue;
        unsigned l = kNone;
        if (val[i] != new_val) {
            const unsigned r = lds_find(lab, (unsigned)i);                      // (a root lies inside the frame: only such pixels are joined)
            l = (unsigned)(y0 + (int)(r / kTile)) * (unsigned)width + (unsigned)(x0 + (int)(r & (kTile - 1)));
        }
        labels[frame0 + (size_t)y * width + x] = l;
    }
}

// ---- across tile edges, on the global labels

__device__ __forceinline__ unsigned label_load(unsigned* lab, unsigned a) {
    return __hip_atomic_load(&lab[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ unsigned global_find(unsigned* lab, unsigned a) {
    // ends: a label never exceeds its index, so a strictly decreases until it reaches a root
    for (unsigned p; (p = label_load(lab, a)) != a;) a = p;
    return a;
}

__device__ __forceinline__ void global_unite(unsigned* lab, unsigned a, unsigned b) {
    // ends: max(a, b) strictly decreases from one round to the next (the finds never raise a or b, and `was` < hi)
    for (;;) {
        a = global_find(lab, a);
        b = global_find(lab, b);
        if (a == b) return;
        const unsigned hi = max(a, b), lo = min(a, b);
        const unsigned was = __hip_atomic_fetch_min(&lab[hi], lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (was == hi) return;                   // hi was a root and now hangs under lo
        a = was;                                 // another thread had hooked hi under `was`: go on from what the atomic returned
        b = lo;
    }
}

// Thread t of a frame: t < (tiles_x - 1) height is pixel (y, 32 k - 1) with its right neighbour, the rest are the pixels
// (32 k - 1, x) with their lower neighbours.
__global__ __launch_bounds__(kThreads) void dcx_speckle_border_kernel(const int16_t* __restrict__ in, int height, int width, int tiles_x,
                                                                       int tiles_y, int new_val, int max_diff, unsigned* labels) {
    const size_t frame0 = (size_t)blockIdx.y * height * width;
    long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    const long long n_vert = (long long)(tiles_x - 1) * height;
    unsigned a, b;
    if (t < n_vert) {
        const int k = (int)(t / height) + 1, y = (int)(t % height);
        a = (unsigned)y * (unsigned)width + (unsigned)(k * kTile - 1);
        b = a + 1;
    } else {
        t -= n_vert;
        if (t >= (long long)(tiles_y - 1) * width) return;
        const int k = (int)(t / width) + 1, x = (int)(t % width);
        a = (unsigned)(k * kTile - 1) * (unsigned)width + (unsigned)x;
        b = a + (unsigned)width;
    }
    if (joined(in[frame0 + a], in[frame0 + b], new_val, max_diff)) global_unite(labels + frame0, a, b);
}

// ---- roots and sizes

__global__ __launch_bounds__(kThreads) void dcx_speckle_count_kernel(int pixels, unsigned* labels, unsigned* sizes) {
    const size_t frame0 = (size_t)blockIdx.y * pixels;
    unsigned* lab = labels + frame0;
    const int p = (int)(blockIdx.x * kThreads + threadIdx.x);
    unsigned root = kNone;
    if (p < pixels) {
        root = lab[p];
        if (root != kNone) {
            // ends: a label never exceeds its index, so root strictly decreases until it reaches a root (a label read here may
            // already be the root that its own thread stored: then the walk is only shorter)
            for (unsigned up; (up = lab[root]) != root;) root = up;
            lab[p] = root;
        }
    }
    // one add per root that the wave holds: its lowest lane with that root adds their number
    unsigned long long todo = __ballot(root != kNone);
    while (todo) {                                                              // (wave-uniform; every round clears at least the leader's bit)
        const int leader = __ffsll((long long)todo) - 1;
        const unsigned r = (unsigned)__shfl((int)root, leader);
        const unsigned long long same = __ballot(root == r);
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&sizes[frame0 + r], (unsigned)__popcll(same));
        todo &= ~same;
    }
}

__global__ __launch_bounds__(kThreads) void dcx_speckle_apply_kernel(const int16_t* in, int16_t* out, int pixels, int new_val,
                                                                      int max_speckle_size, const unsigned* __restrict__ labels,
                                                                      const unsigned* __restrict__ sizes) {
    const size_t frame0 = (size_t)blockIdx.y * pixels;
    const int p = (int)(blockIdx.x * kThreads + threadIdx.x);
    if (p >= pixels) return;
    const unsigned l = labels[frame0 + p];
    const int v = in[frame0 + p];
    const bool speckle = l != kNone && sizes[frame0 + l] <= (unsigned)max_speckle_size;
    out[frame0 + p] = (int16_t)(speckle ? new_val : v);
}

inline bool speckle_shape_ok(int batch, int height, int width) {
    return batch >= 1 && height >= 1 && width >= 1 && height <= kMaxSide && width <= kMaxSide &&
           (long long)height * width <= kMaxPixels;
}

}  // namespace

extern "C" size_t dcx_filter_speckles_workspace_bytes(int batch, int height, int width) {
    if (!speckle_shape_ok(batch, height, width)) return 0;
    return (size_t)batch * height * width * 8;
}

extern "C" int dcx_filter_speckles_s16(const int16_t* d_in, int16_t* d_out, int batch, int height, int width, int new_val,
                                       int max_speckle_size, int max_diff, void* d_workspace, size_t workspace_bytes, void* stream) {
    if (!d_in || !d_out || ((uintptr_t)d_in & 1) || ((uintptr_t)d_out & 1) || !d_workspace || ((uintptr_t)d_workspace & 7)) return DCX_E_ARG;
    if (new_val < -32768 || new_val > 32767 || max_speckle_size < 0 || max_diff < 0 || max_diff > 65535) return DCX_E_ARG;
    if (!speckle_shape_ok(batch, height, width)) return DCX_E_SHAPE;
    const size_t px = (size_t)height * width;
    const size_t fit = workspace_bytes / (px * 8);
    if (fit < 1) return DCX_E_WS;
    size_t chunk = fit < (size_t)batch ? fit : (size_t)batch;                  // frames that one pass takes: the batch, or as many as fit
    if (chunk > (size_t)kMaxChunk) chunk = kMaxChunk;
    hipStream_t s = (hipStream_t)stream;
    unsigned* labels = static_cast<unsigned*>(d_workspace);
    unsigned* sizes = labels + chunk * px;
    const int tiles_x = (width + kTile - 1) / kTile, tiles_y = (height + kTile - 1) / kTile;
    const long long pairs = (long long)(tiles_x - 1) * height + (long long)(tiles_y - 1) * width;
    const unsigned px_blocks = (unsigned)((px + kThreads - 1) / kThreads);
    for (int f0 = 0; f0 < batch; f0 += (int)chunk) {
        const unsigned frames = (unsigned)min((int)chunk, batch - f0);
        const int16_t* in = d_in + (size_t)f0 * px;
        hipLaunchKernelGGL(dcx_speckle_tile_kernel, dim3((unsigned)(tiles_x * tiles_y), frames), dim3(kThreads), 0, s, in, height, width,
                           tiles_x, new_val, max_diff, labels, sizes);
        if (pairs > 0)
            hipLaunchKernelGGL(dcx_speckle_border_kernel, dim3((unsigned)((pairs + kThreads - 1) / kThreads), frames), dim3(kThreads), 0, s,
                               in, height, width, tiles_x, tiles_y, new_val, max_diff, labels);
        hipLaunchKernelGGL(dcx_speckle_count_kernel, dim3(px_blocks, frames), dim3(kThreads), 0, s, (int)px, labels, sizes);
        hipLaunchKernelGGL(dcx_speckle_apply_kernel, dim3(px_blocks, frames), dim3(kThreads), 0, s, in, d_out + (size_t)f0 * px, (int)px,
                           new_val, max_speckle_size, labels, sizes);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}
