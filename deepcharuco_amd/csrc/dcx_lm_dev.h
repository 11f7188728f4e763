// dcx_lm_dev.h -- the joint Levenberg-Marquardt driver of the calibrations (dcx_calib_dev.h over NG = 9 pinhole or 8 fisheye
// intrinsics, dcx_stereo.hip over NG = 6 rig parameters, dcx_rig.hip over NG = 42 of which a rig of C cameras uses 6 (C - 1); every unit -- a
// view, a pair, a timestamp -- adds 6 pose parameters that couple only to the NG global ones), one copy.  deepcharuco_amd/_lm.py restates it for the host definitions.  Three parts:
//   1. the automaton (CvLevMarq's rules), plain C++17 that a host compiler takes without any HIP header, so a stand-alone program
//      can walk its branches (tests/lm_host_main.cpp): LmState, lm_reset, lm_fail, lm_decide;
//   2. device helpers in the idiom of dcx_mat_dev.h's accumulate_rows (the caller passes callables): lm_decide_block (the decide
//      kernels' body), lm_trial_pose (the trial kernels' prologue), lm_source (the reduce kernels' entry -> source mapping),
//      lm_damping;
//   3. lm_run, the host loop.
// The rules: damping 1 + 10^lg, lg from -3; a step whose cost is not <= the cost before is rejected: lg + 1 and the same point is
// tried again, up to lg = 16; at 17 the step is taken whatever it costs (forced); an accepted or forced step takes lg - 1, down to
// -16; at most MAX_ITER accepted steps (kJointMaxIter unless the solver says otherwise: the fisheye calibration's 100); stop at |dp| < DBL_EPSILON |p| over all parameters.
// STOP_FORCED is the one policy the two solvers do not share: a step forced with a cost that is not finite (a point behind a
// camera) ends the stereo solve with DEGENERATE / NONFINITE, while calibration goes on from prev_cost = inf as it always has.
// Deliberately NOT in here: the reductions in front of the global solve (calibration 8 slices x 128 added serially, stereo the
// two fan-ins kChunk / kSlices: the order of a sum is part of the output bits), calibration's rolled NG x NG Cholesky on LDS and
// its spelt-out evaluate loop (both explained where they stand, in dcx_calib_dev.h).  calib_trial_kernel there spells
// lm_trial_pose<NG> out for the pinhole instantiation's SGPR spills.
#pragma once
#include "../../include/deepcharuco_amd.h"

#include <math.h>

#ifdef __HIPCC__
#include "dcx_mat_dev.h"
#define DCX_LM_HD __host__ __device__ __forceinline__
#else
#define DCX_LM_HD inline
#endif

namespace {

// ---- 1. the automaton

enum : int { kNextEvaluate = 0, kNextSchur = 1, kFinished = 2 };                  // LmState::code: what the host launches next
enum : int { kLmOk = 0, kLmNoUnits = 1, kLmDegenerate = 2, kLmNonfinite = 3 };    // the overall status, both solvers' numbering
static_assert(DCX_CALIB_OK == kLmOk && DCX_STEREO_OK == kLmOk, "status");
static_assert(DCX_CALIB_NO_VIEWS == kLmNoUnits && DCX_STEREO_NO_PAIRS == kLmNoUnits, "status");
static_assert(DCX_CALIB_DEGENERATE == kLmDegenerate && DCX_STEREO_DEGENERATE == kLmDegenerate, "status");
static_assert(DCX_CALIB_NONFINITE == kLmNonfinite && DCX_STEREO_NONFINITE == kLmNonfinite, "status");

constexpr int kJointMaxIter = 30;
constexpr double kJointEps = 2.220446049250313e-16;         // DBL_EPSILON

// result = h_result: g (NG), rms, accepted steps, attempts, units used, points used, status; the rest is the caller's.  NR: its
// words, 16 for the two solvers whose h_result that is; dcx_rig.hip's NG = 42 needs 48
template <int NG, int NR = 16>
struct LmState {
    static_assert(NG + 6 <= NR, "result");
    double g[NG], g_trial[NG], dg[NG];
    double prev_cost;
    double result[NR];
    int lg, iters, attempts, code;
};

template <int NG, int NR>
DCX_LM_HD void lm_reset(LmState<NG, NR>* st) {
#pragma unroll
    for (int i = 0; i < NR; ++i) st->result[i] = 0.0;
    st->lg = -3;
    st->iters = 0;
    st->attempts = 0;
}

// the step could not be solved: the outputs stay zero but for the counts
template <int NG, int NR>
DCX_LM_HD void lm_fail(LmState<NG, NR>* st, int status) {
    st->result[NG + 1] = st->iters;
    st->result[NG + 2] = st->attempts;
    st->result[NG + 5] = status;
    st->code = kFinished;
}

// One decision.  init: after the first evaluate (cost = the initial cost); else after a trial with its cost, the units' shares
// of |dp|^2 and |p|^2 (the global parameters' are added here) and whether a trial pose is not finite.
// -> 0: nothing to commit, 1: commit the trial and continue (or fail), 2: commit and finish OK
template <int NG, bool STOP_FORCED, int NR, int MAX_ITER = kJointMaxIter>
DCX_LM_HD int lm_decide(LmState<NG, NR>* st, bool init, double cost, double dn, double pn, double units, double points, bool bad) {
    st->result[NG + 3] = units;
    st->result[NG + 4] = points;
    if (init) {
        if (units == 0.0) {
            st->result[NG + 5] = kLmNoUnits;
            st->code = kFinished;
        } else if (!isfinite(cost)) {
            st->result[NG + 5] = kLmDegenerate;
            st->code = kFinished;
        } else {
            st->prev_cost = cost;
            st->code = kNextSchur;
        }
        return 0;
    }
    st->attempts += 1;
    if (!(cost <= st->prev_cost) && ++st->lg <= 16) {    // (a point behind a camera: cost = inf, rejected like an increase)
        st->code = kNextSchur;                           // retry from the same point with more damping
        return 0;
    }
    // accepted, or forced at lg > 16
    st->lg = st->lg - 1 > -16 ? st->lg - 1 : -16;
    st->iters += 1;
    // (rolled: one thread's work, and unrolled the compiler carries all of g_trial through registers to store it in blocks, which
    // costs calibration's decide kernel eight VGPRs)
#pragma unroll 1
    for (int i = 0; i < NG; ++i) {
        const double d = st->g_trial[i] - st->g[i];
        dn += d * d;
        pn += st->g[i] * st->g[i];
        st->g[i] = st->g_trial[i];
        bad |= !isfinite(st->g[i]);
    }
    if (st->iters >= MAX_ITER || sqrt(dn) < kJointEps * sqrt(pn)) {
        int res = kLmOk;
        if (bad || isnan(cost)) res = kLmNonfinite;
        else if (!isfinite(cost)) res = kLmDegenerate;
        if (res == kLmOk) {
            for (int i = 0; i < NG; ++i) st->result[i] = st->g[i];
            st->result[NG] = sqrt(cost / points);
        }
        lm_fail(st, res);                                // (the counts, the status and the state word: also when res is OK)
        return res == kLmOk ? 2 : 1;
    }
    if (STOP_FORCED && !isfinite(cost)) {
        // forced at lg > 16 with a point behind a camera: there are no normal equations to go on from
        lm_fail(st, bad || isnan(cost) ? kLmNonfinite : kLmDegenerate);
        return 1;
    }
    st->prev_cost = cost;
    st->code = kNextEvaluate;
    return 1;
}

#ifdef __HIPCC__

// ---- 2. device helpers

constexpr int kLmThreads = 1024;                         // the decide kernels' one workgroup

__device__ __forceinline__ double lm_damping(int lg) { return 1.0 + pow(10.0, (double)lg); }

// Where value e of the global solve's sums lives: sum V (NG (NG + 1) / 2 packed) and sum g_a (NG) in the unit's packed
// (NG + 7) x (NG + 7) entries, then the unit's Schur part in order.  -> the index there; e < NG (NG + 1) / 2 + NG says which.
template <int NG>
__device__ __forceinline__ int lm_source(int e) {
    constexpr int NS = NG * (NG + 1) / 2, NC = NG + 7;
    if (e < NS) {
        int a, c;
        unpk<NG>(e, a, c);
        return pk<NC>(a, c);
    }
    return e < NS + NG ? pk<NC>(e - NS, NC - 1) : e - (NS + NG);
}

// A unit's trial pose p = pose - (z - Y dg) from its yz (schur_view's U*^-1 W^T, 6 x NG row major, then U*^-1 g_b), and its
// shares of |dp|^2 and |p|^2.
template <int NG>
__device__ __forceinline__ void lm_trial_pose(const double* yz, const double* dg, const double* pose, double* p, double& dn,
                                              double& pn) {
    dn = pn = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double s = yz[6 * NG + k];
#pragma unroll
        for (int j = 0; j < NG; ++j) s -= yz[k * NG + j] * dg[j];
        const double p0 = pose[k];
        p[k] = p0 - s;
        dn += (p[k] - p0) * (p[k] - p0);
        pn += p0 * p0;
    }
}

// The decide kernels' body, one workgroup of kLmThreads: the units' sums in a fixed tree, lm_decide on thread 0, then the trial
// poses committed where the verdict says so.  used(b): unit b takes part; init_cost(b): its cost after evaluate; trial_sums(b, a):
// its trial cost, |dp|^2 and |p|^2 added to a[0..2]; points(b): its rows; finish(b): the caller's own outputs of unit b when the
// solve ends OK (verdict 2).
template <int NG, bool STOP_FORCED, int NR, int MAX_ITER = kJointMaxIter, class Used, class InitCost, class TrialSums, class Points, class Finish>
__device__ __forceinline__ void lm_decide_block(LmState<NG, NR>* st, int batch, int init, double* pose, const double* trial_pose,
                                                const Used& used, const InitCost& init_cost, const TrialSums& trial_sums,
                                                const Points& points, const Finish& finish) {
    __shared__ double s[kLmThreads][6];      // cost, |dp|^2, |p|^2, units, points, non-finite poses
    __shared__ int verdict;
    if (st->code == kFinished) return;
    const int t = threadIdx.x;
    double a[6] = {0, 0, 0, 0, 0, 0};
    for (int b = t; b < batch; b += kLmThreads) {
        if (!used(b)) continue;
        if (init) {
            a[0] += init_cost(b);
        } else {
            trial_sums(b, a);
#pragma unroll
            for (int k = 0; k < 6; ++k)
                if (!isfinite(trial_pose[(long long)b * 6 + k])) a[5] = 1.0;
        }
        a[3] += 1.0;
        a[4] += points(b);
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) s[t][j] = a[j];
    block_tree<kLmThreads, 6>(s);
    if (t == 0) verdict = lm_decide<NG, STOP_FORCED, NR, MAX_ITER>(st, init != 0, s[0][0], s[0][1], s[0][2], s[0][3], s[0][4], s[0][5] != 0.0);
    __syncthreads();
    if (verdict == 0) return;
    for (int b = t; b < batch; b += kLmThreads) {
        if (!used(b)) continue;
#pragma unroll
        for (int k = 0; k < 6; ++k) pose[(long long)b * 6 + k] = trial_pose[(long long)b * 6 + k];
        if (verdict == 2) finish(b);
    }
}

// ---- 3. the host loop

// One attempt per turn: the state word read (one 4-byte copy and one synchronise), then launch_attempt(evaluate) queues the
// attempt's kernels, the evaluate first where the word asks for it.  Every attempt ends in decide, which increments `attempts`
// or finishes: at most max_iter accepted steps, each after at most 20 rejections (lg from -3 climbs to 17), so the loop always
// ends by the state word.
template <class Launch>
inline hipError_t lm_run(hipStream_t s, const int* d_code, int max_iter, const Launch& launch_attempt) {
    for (int guard = 0; guard < max_iter * 40; ++guard) {
        int code = kFinished;
        hipError_t e = hipMemcpyAsync(&code, d_code, sizeof(int), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return e;
        if (code == kFinished) break;
        launch_attempt(code == kNextEvaluate);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

#endif  // __HIPCC__

}  // namespace
