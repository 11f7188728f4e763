"""Device time of the stereo matcher (disparity.sgm_device, csrc/dcx_sgm.hip) at 32 x 240 x 320 with 64 disparities and at
32 x 480 x 640 with 128, each next to its HBM floor measured in the same process, alternating with it round by round: device
copies that move as many bytes as the matcher moves of S, the one array of it that does not fit a cache.  Per call S (u16,
B H W D 2 bytes) is written once and read and rewritten three times by the path kernels (rows: S = L, then += L; columns: += L
twice) and read once by the select kernel: 8 |S| bytes, which four copy_ calls of an |S|-byte buffer move (4 reads, 4 writes).
The census images (16 B per pixel against 2 D of S) and the frames are left out of the floor.  With --paths 8 the two diagonal
kernels read and rewrite S twice each: 12 |S| bytes, six copy_ calls.

Timing: device events around `inner` back-to-back calls after three warm-up calls of each, rounds repeated until the matcher
alone has run for --seconds (default 1 s) and at least 20 rounds; the figure is the median round's time per call.  Frames: a
2 x 2 box-smoothed random texture, the right frame the left one shifted by 20 px (the loops do not depend on the content).  One
call is checked against the numpy definition at 2 x 48 x 160 before anything is timed.  Also: disparity_to_points_device at the
same shapes.  `rocprofv3 --kernel-trace --stats -- python tools/sgm_probe.py --seconds 0.2` gives the per-kernel times.  Prints
one JSON object and writes it to --out.

    python tools/sgm_probe.py --out profiles/sgm_probe.json
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

S_PASSES = 8                 # reads + writes of S per call (module docstring)
S_PASSES_BY_PATHS = {4: S_PASSES, 8: 12}


def alternate(fns, seconds, min_rounds=20):
    """fns: name -> callable, the first is the one whose total time ends the run -> name -> median ms per call."""
    import torch
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    first = next(iter(fns))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fns[first]()
    ev[1].record()
    torch.cuda.synchronize()
    inner = max(1, int(0.02 / max(ev[0].elapsed_time(ev[1]) * 1e-3, 1e-6)))        # ~20 ms of the matcher per round
    per = {k: [] for k in fns}
    total = 0.0
    while total < seconds or len(per[first]) < min_rounds:
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                f()
            b.record()
            torch.cuda.synchronize()
            ms = a.elapsed_time(b)
            per[k].append(ms / inner)
            if k == first:
                total += ms * 1e-3
    return {k: float(np.median(v)) for k, v in per.items()}, {k: [float(min(v)), float(max(v))] for k, v in per.items()}, \
        inner, len(per[first])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--paths", type=int, default=4, choices=sorted(S_PASSES_BY_PATHS), help="aggregation paths of the matcher")
    a = ap.parse_args()
    import torch
    import disparity_cases as dc
    from deepcharuco_amd import disparity as dp
    assert torch.cuda.is_available(), "sgm_probe measures the GPU kernels: no GPU visible"
    dev = torch.device("cuda", 0)
    paths, s_passes = a.paths, S_PASSES_BY_PATHS[a.paths]

    left, right = dc.two_plane_scene()[:2]
    pair = [np.stack([x, x[::-1]]) for x in (left, right)]
    got = dp.sgm_device(torch.from_numpy(pair[0]).to(dev), torch.from_numpy(pair[1]).to(dev), paths=paths).cpu().numpy()
    assert np.array_equal(got, dp.sgm_host(pair[0], pair[1], paths=paths)), "the device does not match the numpy definition"

    result = {"device": torch.cuda.get_device_name(dev), "seconds": a.seconds, "paths": paths, "s_passes": s_passes, "sgm": {}}
    batch = 32
    Q = np.array([[1, 0, 0, -160.0], [0, 1, 0, -120.0], [0, 0, 0, 300.0], [0, 0, 1.0 / 0.06, 0]])
    for h, w, D in ((240, 320, 64), (480, 640, 128)):
        key = f"{batch}x{h}x{w}_D{D}"
        rng = np.random.default_rng(h)
        frames = [dc.shifted_pair(rng, h, w, 20) for _ in range(batch)]
        fl = torch.from_numpy(np.stack([f[0] for f in frames])).to(dev)
        fr = torch.from_numpy(np.stack([f[1] for f in frames])).to(dev)
        out = torch.empty((batch, h, w), dtype=torch.int16, device=dev)
        ws = torch.empty(dp.sgm_workspace_bytes(batch, h, w, D), dtype=torch.uint8, device=dev)
        s_bytes = batch * h * w * D * 2
        cs, cd = torch.zeros(s_bytes, dtype=torch.uint8, device=dev), torch.empty(s_bytes, dtype=torch.uint8, device=dev)
        xyz = torch.empty((batch, h, w, 3), dtype=torch.float32, device=dev)

        def sgm():
            return dp.sgm_device(fl, fr, 0, D, out=out, workspace=ws, paths=paths)

        def copy():
            for _ in range(s_passes // 2):
                cd.copy_(cs)

        def points():
            return dp.disparity_to_points_device(out, Q, 0, out=xyz)

        ms, spread, inner, rounds = alternate({"sgm": sgm, "copy_floor": copy, "points": points}, a.seconds)
        valid = float((out >= 0).float().mean())
        result["sgm"][key] = {
            "sgm_ms": ms["sgm"], "copy_floor_ms": ms["copy_floor"], "points_ms": ms["points"], "sgm_over_floor": ms["sgm"] / ms["copy_floor"],
            "s_bytes": s_bytes, "s_bytes_moved": s_passes * s_bytes, "sgm_GBps_of_S": s_passes * s_bytes / ms["sgm"] / 1e6,
            "copy_GBps": s_passes * s_bytes / ms["copy_floor"] / 1e6, "frames_per_s": batch / ms["sgm"] * 1e3,
            "min_max_ms": spread, "inner": inner, "rounds": rounds, "valid_fraction": valid}
        print(key, json.dumps(result["sgm"][key]), flush=True)
        del fl, fr, out, ws, cs, cd, xyz
        torch.cuda.empty_cache()
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f)


if __name__ == "__main__":
    main()
