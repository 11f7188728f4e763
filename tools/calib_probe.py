"""Wall time of the device calibration (calib.calibrate_charuco_pool, csrc/dcx_calib.hip) at 64, 512 and 4,096 views of 16 and of
49 corners, its LM step and attempt counts, and the host fp64 definition's wall time (calib.calibrate_camera_host_full) on the
same inputs.

Views: seeded, noisy (sigma = 0.5 px) views of an 8x8-square board (49 corner ids, 2 cm squares) through a 320x240 camera with
five distortion coefficients (tests/test_calib_host.py's scenes); "16 corners" = a random 16 of the 49 ids per view.  Device wall
time: the whole call (it synchronises: the LM loop reads a state word per attempt), median of `--reps` calls after one warm-up,
the pool already on the device.  `rocprofv3 --kernel-trace --stats -- python tools/calib_probe.py --no-host` gives the
per-kernel times.  Prints one JSON object and writes it to --out.

    python tools/calib_probe.py --out profiles/calib_probe.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def views(seed, n_views, n_corners, sigma):
    from deepcharuco_amd import pnp
    from test_calib_host import BOARD, DIST_TRUE, K_TRUE, N_IDS, _pose
    rng = np.random.default_rng(seed)
    k8 = pnp._dist(DIST_TRUE)
    objs, imgs, kps = [], [], []
    for _ in range(n_views):
        while True:
            ids = np.sort(rng.choice(N_IDS, n_corners, replace=False))
            o = pnp.object_points(ids, *BOARD)
            if np.linalg.matrix_rank(o[:, :2] - o[:, :2].mean(0), tol=1e-6) == 2:
                break
        r, t = _pose(rng)
        img, _, _ = pnp._project(o.astype(np.float64), np.zeros((n_corners, 2)), np.r_[r, t], K_TRUE, k8, False)
        img = (img + rng.normal(scale=sigma, size=img.shape)).astype(np.float32)
        objs.append(o)
        imgs.append(img)
        kps.append(np.c_[img.astype(np.float64), ids])
    return objs, imgs, kps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the host definition (for a profiler run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from deepcharuco_amd import calib, corner_pool, pnp
    from test_calib_host import BOARD, SIZE
    assert torch.cuda.is_available(), "calib_probe measures the GPU kernels: no GPU visible"
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(dev), "board": list(BOARD), "image_size": list(SIZE), "sigma_px": 0.5,
              "reps": a.reps, "device_ms": {}, "lm_steps": {}, "lm_attempts": {}, "host_ms": {}, "device_host_gap": {}}
    for n_corners in (16, 49):
        for n_views in (64, 512, 4096):
            key = f"B{n_views}_n{n_corners}"
            objs, imgs, kps = views(1000 + n_views + n_corners, n_views, n_corners, 0.5)
            packed, b, pool = corner_pool.pack_keypoints(kps, dev)
            d = calib.calibrate_charuco_pool(packed, b, pool, True, *BOARD, SIZE)      # warm-up
            ts = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                d = calib.calibrate_charuco_pool(packed, b, pool, True, *BOARD, SIZE)
                ts.append((time.perf_counter() - t0) * 1e3)
            result["device_ms"][key] = float(np.median(ts))
            result["lm_steps"][key] = d.iterations
            result["lm_attempts"][key] = d.attempts
            if not a.no_host:
                t0 = time.perf_counter()
                h = calib.calibrate_camera_host_full(objs, imgs, SIZE)
                result["host_ms"][key] = (time.perf_counter() - t0) * 1e3
                result["device_host_gap"][key] = {
                    "K_rel": float(np.abs(d.camera_matrix - h.camera_matrix).max() / h.camera_matrix[0, 0]),
                    "dist_abs": float(np.abs(d.dist_coeffs - h.dist_coeffs).max()),
                    "rms_rel": abs(d.rms - h.rms) / h.rms, "host_steps": h.iterations, "host_attempts": h.attempts}
            print(key, json.dumps({k: v.get(key) for k, v in result.items() if isinstance(v, dict)}), flush=True)
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f)


if __name__ == "__main__":
    main()
