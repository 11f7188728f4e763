"""Device time of the remap (rectify.remap_device, csrc/dcx_rectify.hip's dcx_remap_u8) at 32 x 240 x 320 gray, 32 x 480 x 640 gray
and 32 x 960 x 1280 gray and BGR, against two yardsticks run in the same process, alternating with it round by round:

(a) a device copy of as many bytes as the remap's source + output (torch's copy_ of a u8 buffer of half that size): the ceiling;
(b) what a user would write without this kernel: torch.nn.functional.grid_sample (bilinear, zeros padding, align_corners) on a
    float copy of the frames, the u8 -> float and float -> u8 conversions included.  Its result is NOT the remap's bits (float
    weights, no 5-bit fraction); the largest difference in gray levels is reported.

Timing: device events around `inner` back-to-back calls, rounds repeated until the remap alone has run for --seconds (default
0.5 s) after three warm-up calls of each; the figure is the median round's time per call.  Bytes: what the algorithm needs,
batch * (source + output) + ceil(batch / F) * map (F = the kernel's frame group: the map is read once per group).  The map is a
real one: camera B of tests/stereo_exact.py scaled to the frame, the 15 degree vergence rig of tests/rectify_exact.py, alpha 0.5.

Also: the map build at 1280 x 960 and the points call at 4,096 x 16 slots, each against its numpy definition (wall time, the
device call synchronised).  `rocprofv3 --kernel-trace --stats -- python tools/rectify_probe.py --seconds 0.1 --no-host` gives the
per-kernel times (`--kernel-stats DB` prints them).  Prints one JSON object and writes it to --out.

    python tools/rectify_probe.py --out profiles/rectify_probe.json
"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def kernel_stats(path):
    """The rectification kernels of a rocprofv3 --kernel-trace result (rocpd .db): calls, total and median duration."""
    import sqlite3
    cur = sqlite3.connect(path).cursor()
    cols = [r[1] for r in cur.execute("pragma table_info(kernels)")]
    name_col = "name" if "name" in cols else [c for c in cols if "name" in c][0]
    by = {}
    for name, dur in cur.execute(f"select {name_col}, end - start from kernels"):
        m = re.search(r"dcx_((?:rectify|remap)_\w+?)_kernel(<[^>]*>)?", name)
        if m:
            by.setdefault(m.group(1) + (m.group(2) or ""), []).append(dur)
    print("rocprofv3 --kernel-trace --stats -- python tools/rectify_probe.py --seconds 0.1 --no-host: the rectification kernels")
    print(f"{'kernel':<32} {'calls':>6} {'total_ms':>10} {'median_us':>10} {'min_us':>9} {'max_us':>9}")
    for name, d in sorted(by.items(), key=lambda kv: -sum(kv[1])):
        print(f"{name:<32} {len(d):6d} {sum(d) / 1e6:10.3f} {np.median(d) / 1e3:10.2f} {min(d) / 1e3:9.2f} {max(d) / 1e3:9.2f}")


def alternate(fns, seconds):
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
    inner = max(1, int(0.02 / max(ev[0].elapsed_time(ev[1]) * 1e-3, 1e-6)))        # ~20 ms of the remap per round
    per = {k: [] for k in fns}
    total = 0.0
    while total < seconds:
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
    return {k: float(np.median(v)) for k, v in per.items()}, inner, len(per[first])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-stats", default=None, metavar="DB", help="summarise a rocprofv3 result instead of measuring")
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy definitions (for a profiler run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats)
    import torch
    import torch.nn.functional as TF
    import rectify_exact as rx
    import stereo_exact as sx
    from deepcharuco_amd import rectify as rc, weights
    assert torch.cuda.is_available(), "rectify_probe measures the GPU kernels: no GPU visible"
    dev = torch.device("cuda", 0)
    F = rc.REMAP_FRAME_GROUP
    K320, dist = sx.cam("B")
    R, T = rx.rig_RT("verge15", "B", "C")
    result = {"device": torch.cuda.get_device_name(dev), "seconds": a.seconds, "frame_group": F, "remap": {}}
    batch = 32
    for h, w, ch in ((240, 320, 1), (480, 640, 1), (960, 1280, 1), (960, 1280, 3)):
        key = f"{batch}x{h}x{w}x{ch}"
        s = w / 320.0
        K0, K1 = K320.copy(), sx.cam_K("C").copy()
        K0[:2] *= s
        K1[:2] *= s
        r = rc.stereo_rectify_host(K0, dist, K1, sx.cam_coeffs("C"), (w, h), R, T, alpha=0.5)
        md = rc.undistort_rectify_map_device(K0, dist, r.R1, r.P1, w, h, device=dev)
        base = torch.from_numpy(weights.synthetic_frames("board", 21, 4, h, w)).to(dev)
        frames = base.repeat(batch // 4, 1, 1)
        frames = frames + torch.arange(batch, device=dev, dtype=torch.uint8)[:, None, None]        # (wraps: 32 different frames)
        if ch == 3:
            frames = torch.stack([frames, 255 - frames, frames // 2], 3).contiguous()
        out = torch.empty((batch, h, w) + ((3,) if ch == 3 else ()), dtype=torch.uint8, device=dev)
        n_copy = (frames.numel() + out.numel()) // 2
        cs, cd = torch.zeros(n_copy, dtype=torch.uint8, device=dev), torch.empty(n_copy, dtype=torch.uint8, device=dev)
        mf = md.to(torch.float32) / 32.0
        grid = torch.stack([mf[..., 0] * (2.0 / (w - 1)) - 1.0, mf[..., 1] * (2.0 / (h - 1)) - 1.0], 2)
        grid = torch.where((md == rc.MAP_SENTINEL), torch.full_like(grid, -3.0), grid)[None].expand(batch, h, w, 2)

        def remap():
            return rc.remap_device(frames, md, 0, out=out)

        def copy():
            return cd.copy_(cs)

        def sample():
            x = frames[:, None].float() if ch == 1 else frames.permute(0, 3, 1, 2).float()
            y = TF.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
            y = y.round_().clamp_(0, 255).to(torch.uint8)
            return y[:, 0] if ch == 1 else y.permute(0, 2, 3, 1).contiguous()

        ms, inner, rounds = alternate({"remap": remap, "copy": copy, "grid_sample": sample}, a.seconds)
        gap = int((sample().to(torch.int16) - remap().to(torch.int16)).abs().max())
        need = batch * (frames[0].numel() + out[0].numel()) + -(-batch // F) * md.numel() * 4
        result["remap"][key] = {
            "remap_ms": ms["remap"], "copy_ms": ms["copy"], "grid_sample_ms": ms["grid_sample"], "bytes_needed": need,
            "remap_GBps": need / ms["remap"] / 1e6, "copy_GBps": 2 * n_copy / ms["copy"] / 1e6,
            "remap_over_copy": ms["remap"] / ms["copy"], "grid_sample_over_remap": ms["grid_sample"] / ms["remap"],
            "inner": inner, "rounds": rounds, "grid_sample_max_gray_level_gap": gap}
        print(key, json.dumps(result["remap"][key]), flush=True)
        del frames, out, cs, cd, grid, mf

    def wall(fn, reps=5, sync=True):
        fn()
        ts = []
        for _ in range(reps):
            if sync:
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            if sync:
                torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    w, h = 1280, 960
    K0 = K320.copy()
    K0[:2] *= 4.0
    K1 = sx.cam_K("C").copy()
    K1[:2] *= 4.0
    r = rc.stereo_rectify_host(K0, dist, K1, sx.cam_coeffs("C"), (w, h), R, T)
    mo = torch.empty((h, w, 2), dtype=torch.int32, device=dev)
    result["map_1280x960"] = {"device_ms": wall(lambda: rc.undistort_rectify_map_device(K0, dist, r.R1, r.P1, w, h, out=mo))}
    rng = np.random.default_rng(5)
    n = 4096 * 16
    packed = np.zeros(2 * 4096 + 6 * n, np.int32)
    packed[:4096] = 16
    packed[4096:8192] = 16 * np.arange(4096)
    xy = np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n)], 1).astype(np.float32)
    packed[8192 + 4 * n:].view(np.float32)[:] = xy.ravel()
    pd = torch.from_numpy(packed).to(dev)
    po = torch.empty((n, 2), dtype=torch.float64, device=dev)
    result["points_4096x16"] = {"device_ms": wall(lambda: rc.rectify_points_pool(pd, 4096, n, True, K0, dist, r.R1, r.P1, out=po))}
    if not a.no_host:
        result["map_1280x960"]["host_ms"] = wall(lambda: rc.undistort_rectify_map_host(K0, dist, r.R1, r.P1, w, h), 3, False)
        hm = rc.undistort_rectify_map_host(K0, dist, r.R1, r.P1, w, h)
        result["map_1280x960"]["entries_differing"] = int((hm != mo.cpu().numpy()).sum())
        result["points_4096x16"]["host_ms"] = wall(lambda: rc.rectify_points_host(xy.astype(np.float64), K0, dist, r.R1, r.P1), 3, False)
        hp = rc.rectify_points_host(xy.astype(np.float64), K0, dist, r.R1, r.P1)
        result["points_4096x16"]["device_host_gap_px"] = float(np.nanmax(np.abs(hp - po.cpu().numpy())))
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f)


if __name__ == "__main__":
    main()
