// dcx_conv_shared.h -- the scaffolding the five convolution kernel templates share (dcx_conv_mfma.h, dcx_conv_wino2h.h,
// dcx_conv_wino2hs.h, dcx_conv_wino2p.h, dcx_conv_wino2ps.h): everything that is NOT specific to a kernel's maths or schedule.
//   device:  packed fp32 helpers, the raw buffer load, the work item and its decode, the persistent XCD-aware item walk, the
//            start / end clock probes, the F(2x2,3x3) row selection and AT coefficients
//   host:    the one launcher of the persistent kernels and the environment-knob reader
// Every device helper is __forceinline__: it disappears at compile time.  These kernels are written around hipcc's register
// allocation, so a change here is checked by comparing the device assembly with the commit before it (tools/isa_same.py), not
// by a benchmark.  That check also decided what is NOT here: a shared helper for the staging descriptor (unit_rsrc), the interior
// test, the padding predicate, the per-unit probe stamps, dcx_conv_wino2h.h's ct_outer decode and the F(2x2,2x2) AT coefficient
// each changed the assembly of some kernel (scheduling order, SGPR counts, in places spills), in every spelling tried, so those
// stay per kernel (profiles/scaffold_isa_identity.txt lists the attempts).
#pragma once
#include "dcx_common.h"

typedef float dcx_f32x16 __attribute__((ext_vector_type(16)));
typedef float dcx_f32x4 __attribute__((ext_vector_type(4)));
typedef float dcx_f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int dcx_u32x4 __attribute__((ext_vector_type(4)));

#define DCX_CCH 16  // input channels per LDS chunk ("unit" of the software pipeline)

// ---- packed fp32 helpers ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 dcx_f4_zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// One v_max_f32.  fmaxf() makes hipcc emit an extra canonicalising v_max per operand (sNaN quieting);
// activations here are finite, and the epilogue runs with the matrix pipe idle, so every VALU counts.
__device__ __forceinline__ float dcx_vmax(float x, float y) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y));
    return r;
}
// one v_pk_add_f32 (hipcc scalarises float2 +/- into two v_add_f32; every VALU instruction in a k-loop costs matrix time)
__device__ __forceinline__ dcx_f32x2 dcx_pk_add(dcx_f32x2 x, dcx_f32x2 y) {
    dcx_f32x2 r;
    asm("v_pk_add_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y));
    return r;
}
__device__ __forceinline__ dcx_f32x2 dcx_pk_sub(dcx_f32x2 x, dcx_f32x2 y) {
    dcx_f32x2 r;
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(x), "v"(y));
    return r;
}
// x - y / x + y on 4 channels (the Winograd input transforms: exact fp32 sums and differences)
__device__ __forceinline__ float4 dcx_sub4(const float4& x, const float4& y) {
    const dcx_f32x2 lo = dcx_pk_sub(dcx_f32x2{x.x, x.y}, dcx_f32x2{y.x, y.y}), hi = dcx_pk_sub(dcx_f32x2{x.z, x.w}, dcx_f32x2{y.z, y.w});
    return make_float4(lo.x, lo.y, hi.x, hi.y);
}
__device__ __forceinline__ float4 dcx_add4(const float4& x, const float4& y) {
    const dcx_f32x2 lo = dcx_pk_add(dcx_f32x2{x.x, x.y}, dcx_f32x2{y.x, y.y}), hi = dcx_pk_add(dcx_f32x2{x.z, x.w}, dcx_f32x2{y.z, y.w});
    return make_float4(lo.x, lo.y, hi.x, hi.y);
}
// y + s * x as two v_pk_fma_f32 (s = +-1 in both halves: exactly y +- x)
__device__ __forceinline__ float4 dcx_fmas4(const float4& x, const dcx_f32x2 s, const float4& y) {
    const dcx_f32x2 lo = __builtin_elementwise_fma(dcx_f32x2{x.x, x.y}, s, dcx_f32x2{y.x, y.y});
    const dcx_f32x2 hi = __builtin_elementwise_fma(dcx_f32x2{x.z, x.w}, s, dcx_f32x2{y.z, y.w});
    return make_float4(lo.x, lo.y, hi.x, hi.y);
}
// y = x * al + be on 4 channels as two v_pk_fma_f32 (packed fp32: 2 results per VALU instruction)
__device__ __forceinline__ float4 dcx_fma4(float4 x, float4 al, float4 be) {
    const dcx_f32x2 lo = __builtin_elementwise_fma(dcx_f32x2{x.x, x.y}, dcx_f32x2{al.x, al.y}, dcx_f32x2{be.x, be.y});
    const dcx_f32x2 hi = __builtin_elementwise_fma(dcx_f32x2{x.z, x.w}, dcx_f32x2{al.z, al.w}, dcx_f32x2{be.z, be.w});
    return make_float4(lo.x, lo.y, hi.x, hi.y);
}
// ReLU + 2x2 max-pool of one float4 as 12 VALU instructions (v_max_f32 with a DPP source = exchange + max in one)
// and NO s_nop: the "VALU write -> DPP read" hazard needs 2 wait states, which hipcc does not pad inside asm.  All 12
// statements are volatile (their order is kept) and each DPP reads a register written >= 3 instructions earlier
// (x, y, z, w round-robin), so the distance holds by construction.  quad_perm [1,0,3,2] = lane^1, [2,3,0,1] = lane^2.
#define DCX_VMAX0(x) asm volatile("v_max_f32 %0, 0, %0" : "+v"(x))
#define DCX_MAX_DPP(x, PERM) asm volatile("v_max_f32_dpp %0, %0, %0 quad_perm:" PERM " row_mask:0xf bank_mask:0xf" : "+v"(x))
__device__ __forceinline__ float4 dcx_relu_quad_max(float4 v) {
    DCX_VMAX0(v.x); DCX_VMAX0(v.y); DCX_VMAX0(v.z); DCX_VMAX0(v.w);
    DCX_MAX_DPP(v.x, "[1,0,3,2]"); DCX_MAX_DPP(v.y, "[1,0,3,2]"); DCX_MAX_DPP(v.z, "[1,0,3,2]"); DCX_MAX_DPP(v.w, "[1,0,3,2]");
    DCX_MAX_DPP(v.x, "[2,3,0,1]"); DCX_MAX_DPP(v.y, "[2,3,0,1]"); DCX_MAX_DPP(v.z, "[2,3,0,1]"); DCX_MAX_DPP(v.w, "[2,3,0,1]");
    return v;
}

// ---- buffer loads -------------------------------------------------------------------------------------------------------
// One raw 128-bit buffer load (voffset per lane, soffset uniform) as float4.  Weights and staged activations both come
// through it; an offset outside the descriptor's range makes the hardware return 0.0f -- the zero padding, with no branch.
constexpr unsigned DCX_OOB = 0x80000000u;      // the offset of a lane that must read zeros
__device__ __forceinline__ float4 dcx_buffer_load_f4(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff = 0) {
    const dcx_u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, soff, 0);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}

// ---- work items and the persistent walk -----------------------------------------------------------------------------------
struct DcxItem {   // one work item = (image, cout tile, [phase,] spatial tile); all fields wave-uniform
    int n, ct, ty, tx;
    int ph;            // phase kernels only: output phase 2a + b
};
// item index -> item: spatial tile innermost, then cout tile, image outermost (skipped images are at the end of the list)
__device__ __forceinline__ DcxItem dcx_decode_item(int wi, int tiles_x, int tiles_y, int n_ct) {
    DcxItem it;
    it.tx = wi % tiles_x; wi /= tiles_x;
    it.ty = wi % tiles_y; wi /= tiles_y;
    it.ct = wi % n_ct;
    it.n = wi / n_ct;
    it.ph = 0;
    return it;
}
// phase kernels: the four phases of a tile are neighbours in the list
__device__ __forceinline__ DcxItem dcx_decode_item_phases(int wi, int tiles_x, int tiles_y, int n_ct) {
    DcxItem it;
    it.ph = wi & 3; wi >>= 2;
    it.tx = wi % tiles_x; wi /= tiles_x;
    it.ty = wi % tiles_y; wi /= tiles_y;
    it.ct = wi % n_ct;
    it.n = wi / n_ct;
    return it;
}

// images the launch really processes
__device__ __forceinline__ int dcx_n_eff(const DcxConvArgs& a) {
    int n_eff = a.n;
    if (a.n_limit != nullptr) n_eff = min(n_eff, *a.n_limit);
    return n_eff;
}
// First work item of XCD x's share: the equal eighth, moved by the weighted deviation in WHOLE CU-ROUNDS (32 items = one item for each
// of an XCD's 32 CUs), rounded to the nearest.  A launch lasts as long as its busiest CU, so a share that is not a multiple of 32 only
// adds a round to a few CUs: with near-equal weights or few items per XCD the deviation rounds to 0 and the split is exactly the equal
// one (a launch of 5 items per workgroup must not become one of 6 for three workgroups: measured -5.5 % on the whole step with
// unquantised shares); a 1.25 % weight moves a boundary of conv1b (2,400 items per XCD) by one round.
__device__ __forceinline__ int dcx_xcd_bound(int total, int x, int cum) {
    const int eq = (int)(((long)total * x) >> 3);
    const int dev = (int)(((long)total * (cum - (x << 13))) >> 16);
    return eq + ((dev + (dev >= 0 ? 16 : -16)) / 32) * 32;
}
// The persistent walk: a workgroup runs items w, w + gstride, ... < w_end of the launch's `total`.  Flat: blockIdx.x, +gridDim.x.
// XCD-aware: block b runs on XCD b % 8 (observed; used for speed only), so the blocks of one XCD walk one
// contiguous eighth of the item list and share halos / repeated inputs / cout tiles through their L2 -- equal eighths unless the
// launcher re-weighted the XCDs.  A workgroup with w >= w_end has no item.
struct DcxWalk { int w, w_end, gstride; };
__device__ __forceinline__ DcxWalk dcx_item_walk(const DcxConvArgs& a, int total) {
    int w = blockIdx.x, w_end = total, gstride = gridDim.x;
    if (a.xcd_walk && (gridDim.x & 7) == 0) {
        const int x = blockIdx.x & 7;
        const int lo = dcx_xcd_bound(total, x, a.xcd_cum[x]);
        w_end = dcx_xcd_bound(total, x + 1, a.xcd_cum[x + 1]);
        gstride = gridDim.x >> 3;
        w = lo + (blockIdx.x >> 3);
    }
    return {w, w_end, gstride};
}

// ---- clock probes of workgroup 0 (DcxConvArgs::clk_probe; tools/unit_probe.py) --------------------------------------------------
// words 0, 1 / 2, 3: {s_memtime, s_memrealtime} at the start / end of the workgroup
__device__ __forceinline__ void dcx_probe_ends(const DcxConvArgs& a, int tid, int word) {
    if (a.clk_probe != nullptr && blockIdx.x == 0 && tid == 0) {
        a.clk_probe[word] = __builtin_amdgcn_s_memtime();
        a.clk_probe[word + 1] = __builtin_amdgcn_s_memrealtime();
    }
}

// ---- Winograd constants -------------------------------------------------------------------------------------------------
// F(2x2,3x3) input transform, row (or column) xi of a 4-wide window d:  t[xi] = d[A] + sgn * d[B]:
//   xi 0 = d0 - d2, xi 1 = d1 + d2, xi 2 = d2 - d1, xi 3 = d1 - d3
__device__ __forceinline__ int dcx_f23_a(int xi) { return xi == 0 ? 0 : xi == 2 ? 2 : 1; }
__device__ __forceinline__ int dcx_f23_b(int xi) { return xi == 2 ? 1 : xi == 3 ? 3 : 2; }
__device__ __forceinline__ float dcx_f23_sgn(int xi) { return xi == 1 ? 1.f : -1.f; }
// output transform of F(2x2,3x3): AT[i][xi], AT = [[1,1,1,0],[0,1,-1,-1]]; T[k = 2 i + j][p = 4 xi + nu] = AT[i][xi] * AT[j][nu]
template <class T> __device__ __forceinline__ T dcx_at23(int i, int xi) { return i == 0 ? (xi < 3 ? T(1) : T(0)) : (xi == 0 ? T(0) : xi == 1 ? T(1) : T(-1)); }

// ---- host: environment knobs and the launcher (definitions: dcx_conv_mfma.hip) -----------------------------------------------
constexpr int DCX_MAX_DEVICES = 64;
int dcx_current_device();    // hipGetDevice() clamped to [0, DCX_MAX_DEVICES)
int dcx_device_cu_count();   // CUs of the CURRENT device (cached per device)
int dcx_fill_xcd_cum(DcxConvArgs& a);    // the current device's cumulative XCD weights; 0 / hipError_t
enum DcxKnob { DCX_KNOB_DETERMINISTIC, DCX_KNOB_XCD_WALK, DCX_KNOB_OCC, DCX_KNOB_CT_OUTER, DCX_KNOB_W2HS, DCX_KNOB_W2HS_ROUNDS,
               DCX_KNOB_W2PS, DCX_KNOB_PROBE_U0, DCX_KNOB_COUNT };
int dcx_env_knob(DcxKnob k);     // atoi of the knob's environment variable, or its default when unset; read ONCE, at first use

// Launches KERNEL on min(items, occ x #CU) persistent workgroups (occ = workgroups per CU the kernel is built for; DCX_OCC=<n>
// lowers it where honour_dcx_occ), with the XCD-aware walk when the grid fills the chip in whole eighths.  after_walk (nullable)
// runs once a.xcd_walk is known.  max_dyn_lds: what the kernel's dynamic-LDS attribute is raised to, once per device.
template <void (*KERNEL)(const DcxConvArgs)>
static int dcx_launch_persistent(DcxConvArgs& a, long items, int threads, int occ, bool honour_dcx_occ, size_t lds_bytes, int max_dyn_lds,
                                 hipStream_t stream, void (*after_walk)(DcxConvArgs&) = nullptr) {
    if (items <= 0 || items > 0x7fffffffL) return DCX_E_SHAPE;
    if (honour_dcx_occ) {
        const int occ_env = dcx_env_knob(DCX_KNOB_OCC);
        if (occ_env > 0 && occ_env < occ) occ = occ_env;
    }
    const long resident = (long)occ * dcx_device_cu_count();
    const long blocks = items < resident ? items : resident;
    a.xcd_walk = dcx_env_knob(DCX_KNOB_XCD_WALK) && blocks == resident && (resident & 7) == 0 ? 1 : 0;
    if (const int rc = dcx_fill_xcd_cum(a)) return rc;
    if (after_walk != nullptr) after_walk(a);
    static bool attr_set[DCX_MAX_DEVICES] = {};      // the attribute is per device (multi-GPU processes)
    const int dev_i = dcx_current_device();
    if (!attr_set[dev_i]) {
        DCX_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, max_dyn_lds));
        attr_set[dev_i] = true;
    }
    if (lds_bytes > 160 * 1024) return DCX_E_SHAPE;
    hipLaunchKernelGGL(KERNEL, dim3((unsigned)blocks), dim3(threads), lds_bytes, stream, a);
    return (int)hipGetLastError();
}
