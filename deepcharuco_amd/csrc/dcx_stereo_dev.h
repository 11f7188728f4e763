// dcx_stereo_dev.h -- what the joint extrinsic solves share (dcx_stereo.hip over two cameras, dcx_rig.hip over up to eight), one
// copy of each fp64 step, on top of dcx_pnp_dev.h (pool, frames, solve) and dcx_lm_dev.h (the LM driver):
//   MaskedPool, the overlap and ident kernels    a camera's pool with its optional per-slot mask, and what reading it needs
//   view_solve                                   the init_views kernels' body: checks, mask compaction, solve()
//   relative_pose                                R_t = R1 R0^T, T_t = t1 - R_t t0 of two poses of one board
//   PairBasis, pair_basis, stereo_row            one row of a camera behind a rig transform: residual and its two lines of
//                                                [J_X (6) | J_P (6)]; the reference camera's rows (SECOND = false) have J_X = 0
//   accumulate_view, view_cost                   a view's rows added to its packed 13 x 13 / its trial cost
//   AnyCamera, any_camera, with_camera           a camera of either model behind a tag, for rigs whose cameras differ
//   view_solve, accumulate_view, view_cost       on AnyCamera: the same step on the camera's own class, through with_camera
//   RigCams, MixedCams, camera_table             a rig's cameras and pools as one kernel argument, all pinholes or tagged
// view_solve, stereo_row, accumulate_view and view_cost are templates on the camera class, as dcx_pnp_dev.h's solver is: PnpCamera
// (dcx_camera_dev.h) or FisheyeCamera (dcx_fisheye_dev.h).  The three that a kernel calls have an AnyCamera overload each, so a
// kernel is one text for a plain camera and for a tagged one: the model is chosen inside the step, not around the kernel's body.
// Everything is force-inlined and has internal linkage, so each translation unit compiles its own copy.
#pragma once
#include "dcx_fisheye_dev.h"
#include "dcx_pnp_dev.h"
#include "dcx_lm_dev.h"

namespace {

constexpr int kLdsStride = 13;           // [J_X (6) | J_P (6) | r]

// A camera of either model (DCX_CAMERA_*).  The tag is the same for every lane of a workgroup that works on one camera, so the
// branch in with_camera() is uniform.
struct AnyCamera {
    int model;
    union {
        PnpCamera pin;
        FisheyeCamera fish;
    };
};

// DcxRigCamera's camera fields under a model tag -> the kernel argument; false if refused: an unknown tag, what pnp_camera() /
// fisheye_camera() refuse, and for a fisheye camera any n_dist but 4 or 0 (k1..k4 in h_dist[0..3], or zeros)
inline bool any_camera(int model, const double* h_camera9, const double* h_dist, int n_dist, AnyCamera& cam) {
    cam.model = model;
    if (model == DCX_CAMERA_PINHOLE) return pnp_camera(h_camera9, h_dist, n_dist, cam.pin);
    if (model != DCX_CAMERA_FISHEYE || !(n_dist == 0 || n_dist == 4) || (n_dist > 0 && !h_dist)) return false;
    return fisheye_camera(h_camera9, n_dist ? h_dist : nullptr, cam.fish);
}

// f(the camera as its own class) -> what f returns
template <class F>
__device__ __forceinline__ auto with_camera(const AnyCamera& cam, F&& f) {
    return cam.model == DCX_CAMERA_FISHEYE ? f(cam.fish) : f(cam.pin);
}

struct MaskedPool {                      // one camera's pool and the optional mask that rides beside it
    CornerPool p;
    const uint8_t* mask;                 // per slot, or null: every row is kept
};

// One wave per view of a pool with a mask: does its slot range meet another view's?
__global__ __launch_bounds__(kLanes) void stereo_overlap_kernel(CornerPool pl, int batch, int32_t* __restrict__ flag) {
    if (ranges_overlap(pl, batch, blockIdx.x) && threadIdx.x == 0) *flag = 1;
}

__global__ __launch_bounds__(256) void stereo_ident_kernel(int n, int32_t* __restrict__ ident) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) ident[i] = i;
}

// View t of a pool: the checks; with a mask the kept rows compacted in order (ballot + prefix popcount, 64 rows at a time) into
// the index list at the view's own slots of `lists`; solve() over an IndexedFrame either way, so a NULL mask and a mask of ones run
// the same instructions on the same values.  -> DCX_PNP_*; out = solve()'s pose words (zero unless it ran), kept = the rows after
// the mask (0 for a view that is empty or cut by the pool).  One wave, the whole block.
template <class CAM>
__device__ __forceinline__ int view_solve(const MaskedPool& pl, const CAM& cam, int t, int32_t* lists, const int32_t* ident,
                                          double (&out)[8], int& kept) {
    const int lane = threadIdx.x;
    const int n = pl.p.counts[t], s0 = pl.p.starts[t];
    int st = DCX_PNP_OK;
    kept = 0;
    const int32_t* idx = ident;
    // Not the header's frame_status(): with a mask this is another function (only the kept rows' ids are checked, and TOO_FEW is
    // judged on the kept rows, after the pool cut).  Its first two rules mirror frame_status(); a change there is a change here.
    if (n <= 0) {
        st = DCX_PNP_TOO_FEW;
    } else if (s0 < 0 || (long long)s0 + n > (long long)pl.p.pool) {
        st = DCX_PNP_TRUNCATED;               // (its slots are not read)
    } else {
        bool bad = false;
        if (pl.mask) {
            int32_t* list = lists + s0;
            for (int base = 0; base < n; base += kLanes) {
                const int i = base + lane;
                const bool in = i < n && pl.mask[(long long)s0 + i] != 0;
                const int at = append_kept(in, lane, kept);
                if (in) {
                    list[at] = i;
                    const int id = pl.p.rows[4 * ((long long)s0 + i) + 2];
                    bad |= id < 0 || id >= pl.p.n_ids;
                }
            }
            idx = list;
        } else {
            for (int i = lane; i < n; i += kLanes) {
                const int id = pl.p.rows[4 * ((long long)s0 + i) + 2];
                bad |= id < 0 || id >= pl.p.n_ids;
            }
            kept = n;
        }
        __syncthreads();                      // one wave: the list is read below by other lanes than wrote it
        if (kept < 4) st = DCX_PNP_TOO_FEW;
        else if (__any(bad)) st = DCX_PNP_BAD_ID;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = 0.0;
    if (st == DCX_PNP_OK) {
        const IndexedFrame g{pl.p.frame(n, s0), idx, kept};
        st = solve(g, cam, out);
    }
    return st;
}

// Two poses (rvec, tvec) of one board, in cameras 0 and 1 -> rig = R_t (9, row major) = R1 R0^T, T_t (3) = t1 - R_t t0
__device__ __forceinline__ void relative_pose(const double* p0, const double* p1, double* rig) {
    double R0[9], R1[9];
    rodrigues(p0, R0);
    rodrigues(p1, R1);
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) rig[a * 3 + b] = R1[a * 3] * R0[b * 3] + R1[a * 3 + 1] * R0[b * 3 + 1] + R1[a * 3 + 2] * R0[b * 3 + 2];
#pragma unroll
    for (int a = 0; a < 3; ++a) rig[9 + a] = p1[3 + a] - (rig[a * 3] * p0[3] + rig[a * 3 + 1] * p0[4] + rig[a * 3 + 2] * p0[5]);
}

// What every row of a pair shares: R(P), t_P, pose_basis()'s G at P, R(X), T_X and Jr(r_X).
struct PairBasis {
    double RP[9], tP[3], G[2][9], RX[9], TX[3], JX[9];
};

template <bool JAC>
__device__ __forceinline__ void pair_basis(const double* x, const double* p, PairBasis& B) {
    if (JAC) pose_basis(p, B.RP, B.G);
    else rodrigues(p, B.RP);
    rodrigues(x, B.RX);
    if (JAC) right_jacobian(x, B.JX);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        B.tP[i] = p[3 + i];
        B.TX[i] = x[3 + i];
    }
}

// One row of camera SECOND's view at (X, P) -> residual (ru, rv); with JAC its two rows of [J_X (6) | J_P (6)]: the header's
// project() and pose_columns() on the point q = R_P m + t_P (camera 0) or R_X q + T_X (camera 1).  false if the
// point is not in front of the camera.
template <bool JAC, bool SECOND, class CAM>
__device__ __forceinline__ bool stereo_row(const CAM& cam, const PairBasis& B, double mx, double my, double u, double v,
                                           double& ru, double& rv, double* ju, double* jv) {
    double q0[3], q[3], du[3], dv[3];
    board_point(B.RP, B.tP, mx, my, q0);
#pragma unroll
    for (int i = 0; i < 3; ++i)
        q[i] = SECOND ? B.RX[i * 3] * q0[0] + B.RX[i * 3 + 1] * q0[1] + B.RX[i * 3 + 2] * q0[2] + B.TX[i] : q0[i];
    if (!project<JAC>(cam, q, u, v, ru, rv, du, dv)) return false;
    if (!JAC) return true;
    // d(u, v)/dq0: camera 1 sees q0 through R_X
    double eu[3], ev[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        eu[j] = SECOND ? du[0] * B.RX[j] + du[1] * B.RX[3 + j] + du[2] * B.RX[6 + j] : du[j];
        ev[j] = SECOND ? dv[0] * B.RX[j] + dv[1] * B.RX[3 + j] + dv[2] * B.RX[6 + j] : dv[j];
    }
    pose_columns(eu, ev, mx, my, B.G, ju + 6, jv + 6);
    if (SECOND) {
        // dq/dr_X = -R_X [q0]x Jr(r_X), so d(u, v)/dr_X = -(e . A), A = [q0]x Jr(r_X)
        const double S[9] = {0.0, -q0[2], q0[1], q0[2], 0.0, -q0[0], -q0[1], q0[0], 0.0};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double su = 0.0, sv = 0.0;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double a = S[i * 3] * B.JX[j] + S[i * 3 + 1] * B.JX[3 + j] + S[i * 3 + 2] * B.JX[6 + j];
                su += eu[i] * a;
                sv += ev[i] * a;
            }
            ju[j] = -su;
            jv[j] = -sv;
            ju[3 + j] = du[j];
            jv[3 + j] = dv[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < 6; ++j) ju[j] = jv[j] = 0.0;
    }
    return true;
}

// One view's rows added to the pair's 91 entries: 64 rows at a time through LDS, every lane its two entries in row order.
template <bool SECOND, class CAM>
__device__ __forceinline__ void accumulate_view(const IndexedFrame& f, const CAM& cam, const PairBasis& B,
                                                double (*sj)[kLdsStride], const int* ea, const int* eb, double* acc, bool& behind) {
    accumulate_rows<13, 2, kLdsStride>(f.n, [&](int i, double* ju, double* jv) {
        double mx, my, u, v;
        f.load(i, mx, my, u, v);
        return stereo_row<true, SECOND>(cam, B, mx, my, u, v, ju[12], jv[12], ju, jv);
    }, sj, ea, eb, acc, behind);
}

template <bool SECOND, class CAM>
__device__ __forceinline__ double view_cost(const IndexedFrame& f, const CAM& cam, const PairBasis& B) {
    double c[1] = {0.0};
    for (int i = threadIdx.x; i < f.n; i += kLanes) {
        double mx, my, u, v, ru, rv;
        f.load(i, mx, my, u, v);
        if (!stereo_row<false, SECOND>(cam, B, mx, my, u, v, ru, rv, nullptr, nullptr)) {
            c[0] = INFINITY;
            continue;
        }
        c[0] += ru * ru + rv * rv;
    }
    wave_sum(c);
    return c[0];
}

// The three steps that take a camera, on a camera of either model: the same step on the camera's own class.  Partial ordering
// prefers these to the templates on CAM, so a kernel that is a template on its camera type reads the same for both.
__device__ __forceinline__ int view_solve(const MaskedPool& pl, const AnyCamera& cam, int t, int32_t* lists, const int32_t* ident,
                                          double (&out)[8], int& kept) {
    return with_camera(cam, [&](const auto& k) { return view_solve(pl, k, t, lists, ident, out, kept); });
}

template <bool SECOND>
__device__ __forceinline__ void accumulate_view(const IndexedFrame& f, const AnyCamera& cam, const PairBasis& B,
                                                double (*sj)[kLdsStride], const int* ea, const int* eb, double* acc, bool& behind) {
    with_camera(cam, [&](const auto& k) { accumulate_view<SECOND>(f, k, B, sj, ea, eb, acc, behind); return 0; });
}

template <bool SECOND>
__device__ __forceinline__ double view_cost(const IndexedFrame& f, const AnyCamera& cam, const PairBasis& B) {
    return with_camera(cam, [&](const auto& k) { return view_cost<SECOND>(f, k, B); });
}

// ---- the camera table of a rig of up to DCX_RIG_MAX_CAMERAS cameras, as the kernels of dcx_rig.hip and dcx_rigpose.hip take it by
// value, and the one host-side check that fills it from the C ABI's DcxRigCamera array

constexpr int kMaxCams = DCX_RIG_MAX_CAMERAS;

struct RigCams {                         // every camera a pinhole: what dcx_rig_calibrate_pool has always passed
    MaskedPool pl[kMaxCams];
    PnpCamera cam[kMaxCams];
};

struct MixedCams {                       // a model tag per camera (dcx_rig_calibrate_models_pool with a fisheye camera in the rig)
    MaskedPool pl[kMaxCams];
    AnyCamera cam[kMaxCams];
};
static_assert(sizeof(MixedCams) <= 2048, "kernel arguments");

// The pools and, per camera, what `camera` makes of its model fields -> false if anything is refused
template <class CAMS, class F>
bool camera_table(int n_cams, const DcxRigCamera* h_cams, int batch, int col_count, int row_count, double square_len, CAMS& cams,
                  int* pools, F&& camera) {
    if (n_cams < 2 || n_cams > kMaxCams || !h_cams) return false;
    for (int c = 0; c < n_cams; ++c) {
        const DcxRigCamera& h = h_cams[c];
        cams.pl[c].mask = h.d_mask;
        if (!corner_pool(h.d_counts, h.d_starts, h.d_rows, h.d_xy, batch, h.pool, col_count, row_count, square_len, cams.pl[c].p))
            return false;
        if (!camera(c, h, cams.cam[c])) return false;
        pools[c] = h.pool;
    }
    return true;
}

}  // namespace
