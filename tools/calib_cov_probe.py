"""Times the calibration uncertainty (calib.calibration_uncertainty_pool, four launches, no synchronisation) at 4,096 views of 16 and of
49 rows, beside the calibration call on the same pool in the same process (one MI355X) -> profiles/calib_cov_probe.json.  No speed
is promised anywhere; this is the measurement.  The yardstick is one Levenberg-Marquardt attempt of the calibration (its time
divided by its attempts): the uncertainty runs one evaluate, one Schur pass, one one-workgroup reduction and one per-view pass, which
is what an attempt runs.

Scenes: 64 distinct views of an 8 x 8 board (49 corners, or the 16 of every other row and column) through a 400 px pinhole lens with
five distortion coefficients at 320 x 240, 0.3 px of noise, float32 pixels, laid 64 times into one corner pool of 4,096 views.  The
uncertainty is given the device tensors (view status, poses, workspace, outputs), so nothing is uploaded inside the timed region.
Wall time around a synchronised call and the device time between two events, medians of ``--repeats`` after one warm-up call.

    python tools/calib_cov_probe.py [--views 4096] [--repeats 7] [--out profiles/calib_cov_probe.json]
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
SIZE = (320, 240)
K = np.array([[400.0, 0, 163.2], [0, 410.0, 117.5], [0, 0, 1]])
DIST = np.array([-0.25, 0.1, 1e-3, -5e-4, -0.02])
SIGMA = 0.3


def scenes(n, ids, seed=1):
    from deepcharuco_amd import pnp
    rng = np.random.default_rng(seed)
    obj = pnp.object_points(ids, *BOARD).astype(np.float64)
    k8 = pnp._dist(DIST)
    out = []
    while len(out) < n:
        r = rng.normal(size=3)
        r *= np.deg2rad(rng.uniform(5, 60)) / np.linalg.norm(r)
        t = np.array([rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02), rng.uniform(0.2, 0.3)]) - pnp._rodrigues(r) @ np.array([0.08, 0.08, 0.0])
        pix = pnp._project(obj, np.zeros((len(ids), 2)), np.r_[r, t], K, k8, False)[0]
        if pix is None or not np.isfinite(pix).all():
            continue
        pix = pix + rng.normal(scale=SIGMA, size=pix.shape)
        out.append(np.c_[pix.astype(np.float32).astype(np.float64), ids])
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
    ap.add_argument("--views", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "calib_cov_probe.json"))
    a = ap.parse_args()
    import torch
    from deepcharuco_amd import _lib, calib, corner_pool
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "views": a.views, "distinct_views": 64, "sigma_px": SIGMA, "repeats": a.repeats,
           "csrc_sha256": _lib.csrc_sha256()}
    grid = np.arange(49).reshape(7, 7)
    for rows, ids in ((16, grid[::2, ::2].ravel()), (49, grid.ravel())):
        base = scenes(64, ids)
        packed, b, pool = corner_pool.pack_keypoints([base[i % 64] for i in range(a.views)], dev)
        c = calib.calibrate_charuco_pool(packed, b, pool, True, *BOARD, SIZE)
        t_cal = timed(lambda: calib.calibrate_charuco_pool(packed, b, pool, True, *BOARD, SIZE), a.repeats)
        st = torch.from_numpy(c.view_status.astype(np.int32)).to(dev)
        pose = torch.zeros((b, 8), dtype=torch.float64, device=dev)
        pose[:, :6] = torch.from_numpy(np.c_[c.rvecs, c.tvecs]).to(dev)
        model = (c.camera_matrix, c.dist_coeffs, st, pose)
        ws = torch.empty(calib.uncertainty_workspace_bytes(b), dtype=torch.uint8, device=dev)
        out = (torch.empty(calib.COV_GLOBAL_WORDS, dtype=torch.float64, device=dev),
               torch.empty((b, calib.COV_POSE_WORDS), dtype=torch.float64, device=dev))
        mask = torch.ones(pool, dtype=torch.uint8, device=dev)

        def cov(inliers=None):
            calib.calibration_uncertainty_pool(packed, b, pool, True, *BOARD, model, inliers=inliers, workspace=ws, out=out)

        t_cov = timed(cov, a.repeats)
        t_mask = timed(lambda: cov(mask), a.repeats)
        u = calib.unpack_uncertainty(*out)
        per_attempt = t_cal["median_ms"] / max(c.attempts, 1)
        res[f"{rows} rows per view"] = {
            "calibrate_charuco_pool": dict(t_cal, status=c.status, steps=c.iterations, attempts=c.attempts, rms_px=c.rms,
                                           ms_per_attempt=round(per_attempt, 4)),
            "calibration_uncertainty_pool": dict(t_cov, status=u.status, sigma2=u.sigma2, dof=u.dof, std_fx=float(u.std_intrinsics[0]),
                                                 attempts_worth=round(t_cov["median_ms"] / per_attempt, 3)),
            "calibration_uncertainty_pool, all-ones mask": t_mask}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
