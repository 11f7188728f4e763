"""Times the rig uncertainty (rig.rig_uncertainty_pools, five launches, no synchronisation) at 4,096 timestamps of 16 rows per view
for rigs of 2, 4 and 8 cameras, beside the rig calibration on the same pools in the same process (one MI355X) ->
profiles/rig_cov_probe.json.  No speed is promised anywhere; this is the measurement.  The yardstick is one Levenberg-Marquardt
attempt of the calibration (its time divided by its attempts, the per-view solves and the host's part included): the uncertainty
runs one evaluate, one Schur pass, the two reductions and one per-timestamp pass, which is what an attempt runs.

Scenes: 64 distinct timestamps of an 8 x 8 board (the 16 corners of every other row and column) seen by C pinhole cameras (400 px,
five distortion coefficients) on an arc, their axes meeting on the board 5 degrees apart, 0.3 px of noise, float32 pixels, laid 64
times into C corner pools of 4,096 views each.  The uncertainty is given the device tensors (view status, poses, workspace,
outputs), so nothing is uploaded inside the timed region.  Wall time around a synchronised call and the device time between two
events, medians of ``--repeats`` after one warm-up call.

    python tools/rig_cov_probe.py [--stamps 4096] [--repeats 7] [--out profiles/rig_cov_probe.json]

Which launch carries the time is not this tool's business: run it after ``rocprofv3 --kernel-trace --stats --``, in a run of its own.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BOARD = (8, 8, 0.02)
K = np.array([[400.0, 0, 163.2], [0, 410.0, 117.5], [0, 0, 1]])
DIST = np.array([-0.25, 0.1, 1e-3, -5e-4, -0.02])
SIGMA = 0.3
DEPTH = 0.3
STEP_DEG = 5.0


def make_rig(n_cams):
    """X_c = (rvec, T), c = 1 .. C - 1: camera c's axis meets camera 0's at DEPTH, STEP_DEG * c away about the y axis."""
    from deepcharuco_amd import pnp
    X = []
    for c in range(1, n_cams):
        r = np.array([0.0, 1.0, 0.0]) * np.deg2rad(STEP_DEG * c)
        X.append(np.r_[r, np.array([0, 0, DEPTH]) - pnp._rodrigues(r) @ np.array([0, 0, DEPTH])])
    return np.array(X)


def scenes(n, ids, X, seed=1):
    """n timestamps -> per camera a list of [x, y, id] arrays."""
    from deepcharuco_amd import pnp
    rng = np.random.default_rng(seed)
    obj = pnp.object_points(ids, *BOARD).astype(np.float64)
    k8 = pnp._dist(DIST)
    C = len(X) + 1
    mid = np.array([0.0, 1.0, 0.0]) * np.deg2rad(-STEP_DEG * (C - 1) / 2)       # tilted towards the middle of the arc
    out = [[] for _ in range(C)]
    while len(out[0]) < n:
        r = rng.normal(size=3)
        r *= np.deg2rad(rng.uniform(5, 25)) / np.linalg.norm(r)
        R = pnp._rodrigues(mid) @ pnp._rodrigues(r)
        t = np.array([rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01), rng.uniform(0.95, 1.1) * DEPTH]) - R @ np.array([0.08, 0.08, 0.0])
        views = []
        for c in range(C):
            Rc = pnp._rodrigues(X[c - 1, :3]) if c else np.eye(3)
            p = np.r_[pnp._rvec_of(Rc @ R), Rc @ t + (X[c - 1, 3:] if c else 0.0)]
            pix = pnp._project(obj, np.zeros((len(ids), 2)), p, K, k8, False)[0]
            if pix is None or not np.isfinite(pix).all():
                break
            pix = pix + rng.normal(scale=SIGMA, size=pix.shape)
            views.append(np.c_[pix.astype(np.float32).astype(np.float64), ids])
        if len(views) == C:
            for c in range(C):
                out[c].append(views[c])
    return out


def timed(fn, repeats):
    import torch
    fn()
    torch.cuda.synchronize()
    wall, device = [], []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
        device.append(e0.elapsed_time(e1))
    return {"median_ms": round(statistics.median(wall), 4), "min_ms": round(min(wall), 4), "max_ms": round(max(wall), 4),
            "device_median_ms": round(statistics.median(device), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stamps", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cams", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "rig_cov_probe.json"))
    a = ap.parse_args()
    import torch
    from deepcharuco_amd import _lib, calib, corner_pool, rig
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "stamps": a.stamps, "distinct_stamps": 64, "rows_per_view": 16, "sigma_px": SIGMA,
           "repeats": a.repeats, "csrc_sha256": _lib.csrc_sha256()}
    ids = np.arange(49).reshape(7, 7)[::2, ::2].ravel()
    for C in a.cams:
        base = scenes(64, ids, make_rig(C))
        packs = [corner_pool.pack_keypoints([base[c][i % 64] for i in range(a.stamps)], dev) for c in range(C)]
        packed, pools, b = [p[0] for p in packs], [p[2] for p in packs], a.stamps
        cams, dists = [K] * C, [DIST] * C

        def calibrate():
            return rig.rig_calibrate_pools(packed, b, pools, True, *BOARD, cams, dists)

        r = calibrate()
        t_cal = timed(calibrate, a.repeats)
        st = torch.from_numpy(r.view_status.astype(np.int32)).to(dev)
        pose = torch.zeros((b, 8), dtype=torch.float64, device=dev)
        pose[:, :6] = torch.from_numpy(np.c_[r.rvecs, r.tvecs]).to(dev)
        model = (r.rvec, r.T, st, pose)
        ws = torch.empty(rig.rig_uncertainty_workspace_bytes(C, b, pools), dtype=torch.uint8, device=dev)
        out = (torch.empty(rig.RIGCOV_GLOBAL_WORDS, dtype=torch.float64, device=dev),
               torch.empty((b, calib.COV_POSE_WORDS), dtype=torch.float64, device=dev))

        def cov():
            rig.rig_uncertainty_pools(packed, b, pools, True, *BOARD, cams, dists, model, workspace=ws, out=out)

        t_cov = timed(cov, a.repeats)
        u = rig.unpack_rig_uncertainty(*out, r.T)
        per_attempt = t_cal["median_ms"] / max(r.attempts, 1)
        res[f"{C} cameras"] = {
            "rig_calibrate_pools": dict(t_cal, status=r.status, steps=r.iterations, attempts=r.attempts, rms_px=r.rms,
                                        ms_per_attempt=round(per_attempt, 4)),
            "rig_uncertainty_pools": dict(t_cov, status=u.status, sigma2=u.sigma2, dof=u.dof, workspace_bytes=ws.numel(),
                                          baseline_std_last=float(u.baseline_std[-1]),
                                          attempts_worth=round(t_cov["median_ms"] / per_attempt, 3))}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
