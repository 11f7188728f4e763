"""Device time of the PnP kernel (dcx_solve_pnp_pool, csrc/dcx_pnp.hip) at B = 32 and B = 128 frames with 16 and 256 points per
frame, against the per-frame time of the host fp64 definition (pnp.solve_pnp_host).

Frames are seeded, noisy (sigma = 0.3 px) views of a 20x20 board (361 corner ids, 2 mm squares), 5-coefficient distortion.  Device
time: hipEvents around `--reps` back-to-back launches on one stream after `--warmup` launches (per launch = total / reps, so it
includes the launch gaps; `rocprofv3 --kernel-trace --stats -- python tools/pnp_probe.py` gives the kernel's own time).  Prints
one JSON object and writes it to --out.

    python tools/pnp_probe.py --out profiles/pnp_probe.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BOARD = (20, 20, 0.002)
K = np.array([[300.0, 0, 160], [0, 300.0, 120], [0, 0, 1]])
DIST5 = np.array([-0.2, 0.05, 1e-3, -1e-3, 0.0])


def frames(rng, b, n_points):
    from deepcharuco_amd import pnp
    out = []
    for _ in range(b):
        ids = np.sort(rng.choice(361, n_points, replace=False))
        r = rng.normal(size=3)
        r *= np.deg2rad(rng.uniform(5, 50)) / np.linalg.norm(r)
        R = pnp._rodrigues(r)
        t = np.array([rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01), rng.uniform(0.12, 0.2)]) - R @ np.array([0.02, 0.02, 0])
        obj = pnp.object_points(ids, *BOARD).astype(np.float64)
        img, _, _ = pnp._project(obj, np.zeros((n_points, 2)), np.r_[r, t], K, pnp._dist(DIST5), False)
        img = img + rng.normal(scale=0.3, size=img.shape)
        out.append(np.c_[img.astype(np.float32).astype(np.float64), ids])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-frames", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from deepcharuco_amd import corner_pool, pnp
    assert torch.cuda.is_available(), "pnp_probe measures the GPU kernel: no GPU visible"
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    result = {"device": torch.cuda.get_device_name(dev), "board": list(BOARD), "dist": DIST5.tolist(), "sigma_px": 0.3,
              "reps": a.reps, "device_ms_per_launch": {}, "lm_steps_mean": {}, "host_ms_per_frame": {}}
    for n_points in (16, 256):
        for b in (32, 128):
            fr = frames(rng, b, n_points)
            packed, bb, pool = corner_pool.pack_keypoints(fr, dev)
            out = pnp.solve_pnp_pool(packed, bb, pool, True, *BOARD, K, DIST5)
            for _ in range(a.warmup):
                pnp.solve_pnp_pool(packed, bb, pool, True, *BOARD, K, DIST5, out=out)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                pnp.solve_pnp_pool(packed, bb, pool, True, *BOARD, K, DIST5, out=out)
            e1.record()
            e1.synchronize()
            st, pose = out[0].cpu().numpy(), out[1].cpu().numpy()
            assert (st == pnp.PNP_OK).all(), st
            key = f"B{b}_n{n_points}"
            result["device_ms_per_launch"][key] = e0.elapsed_time(e1) / a.reps
            result["lm_steps_mean"][key] = float(pose[:, 7].mean())
        fr = frames(rng, a.host_frames, n_points)
        t0 = time.perf_counter()
        for kp in fr:
            pnp.solve_pnp_host(kp, *BOARD, K, DIST5)
        result["host_ms_per_frame"][f"n{n_points}"] = (time.perf_counter() - t0) * 1e3 / a.host_frames
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
