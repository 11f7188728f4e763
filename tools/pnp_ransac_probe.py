"""Device time of the RANSAC pose solver (dcx_solve_pnp_ransac_pool, csrc/dcx_pnp_ransac.hip: 100 hypotheses per frame, then the
refit) beside the plain solver (dcx_solve_pnp_pool) on the same frames in the same process: tools/pnp_probe.py's frames (B = 32 and
128, 16 and 256 points, sigma = 0.3 px, 20x20 board), clean, so that the refit runs over the same rows as the plain solve.

Device time: hipEvents around `--reps` back-to-back calls on one stream after `--warmup` calls (per call = total / reps, launch
gaps included; a RANSAC call is two launches).  The kernels' own times come from a separate run,
`rocprofv3 --kernel-trace --stats -- python tools/pnp_ransac_probe.py --reps 20`.  Prints one JSON object and writes it to --out.

    python tools/pnp_ransac_probe.py --out profiles/pnp_ransac_probe.json
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pnp_probe import BOARD, DIST5, K, frames  # noqa: E402


def timed(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="the timed loop is repeated; the median is reported, all are kept")
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--reproj-error", type=float, default=8.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from deepcharuco_amd import corner_pool, pnp
    assert torch.cuda.is_available(), "pnp_ransac_probe measures the GPU kernels: no GPU visible"
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    result = {"device": torch.cuda.get_device_name(dev), "board": list(BOARD), "dist": DIST5.tolist(), "sigma_px": 0.3,
              "reps": a.reps, "rounds": a.rounds, "iterations": a.iterations, "reproj_error_px": a.reproj_error,
              "plain_ms_per_call": {}, "ransac_ms_per_call": {}, "ransac_over_plain": {}, "all_rounds_ms": {},
              "inliers_mean": {}, "lm_steps_mean": {}}
    for n_points in (16, 256):
        for b in (32, 128):
            fr = frames(rng, b, n_points)
            packed, bb, pool = corner_pool.pack_keypoints(fr, dev)
            args = (packed, bb, pool, True, *BOARD, K, DIST5)
            kw = dict(iterations=a.iterations, reproj_error=a.reproj_error, seed=0)
            plain = pnp.solve_pnp_pool(*args)
            ws = torch.empty((pnp.ransac_workspace_bytes(bb, pool, a.iterations) // 8,), dtype=torch.float64, device=dev)
            out = pnp.solve_pnp_ransac_pool(*args, workspace=ws, **kw)
            t_plain, t_ransac = [], []
            for _ in range(a.rounds):
                t_plain.append(timed(lambda: pnp.solve_pnp_pool(*args, out=plain), a.warmup, a.reps))
                t_ransac.append(timed(lambda: pnp.solve_pnp_ransac_pool(*args, out=out, workspace=ws, **kw), a.warmup, a.reps))
            st, pose, info = out[0].cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy()
            assert (st == pnp.PNP_OK).all() and (plain[0].cpu().numpy() == pnp.PNP_OK).all(), st
            key = f"B{b}_n{n_points}"
            result["plain_ms_per_call"][key] = float(np.median(t_plain))
            result["ransac_ms_per_call"][key] = float(np.median(t_ransac))
            result["ransac_over_plain"][key] = float(np.median(t_ransac) / np.median(t_plain))
            result["all_rounds_ms"][key] = {"plain": t_plain, "ransac": t_ransac}
            result["inliers_mean"][key] = float(info[:, 0].mean())
            result["lm_steps_mean"][key] = float(pose[:, 7].mean())
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
