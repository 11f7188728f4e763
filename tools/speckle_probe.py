"""Device time of the speckle filter (disparity.filter_speckles_device, csrc/dcx_speckle.hip) at 32 x 240 x 320 and at
32 x 480 x 640, each next to a device copy of the bytes the filter moves, measured in the same process and alternating with it
round by round.  Per pixel the filter moves 30 bytes when every chain of labels is one step long: the tile kernel reads the map
(2) and writes a label and a cleared size (8); the count kernel reads and rewrites the label (8); the apply kernel reads label,
size and map and writes the result (12); the border kernel's pairs (two per 32 pixels) and the count kernel's adds are left out.
One copy_ of a 15-bytes-per-pixel buffer moves as much (a read and a write).

Maps: a slanted plane (16 x disparity, one sixteenth per 2 px) of which a tenth is invalid and a twentieth replaced by random
values, which makes the single-pixel and few-pixel components a matcher leaves behind; new_val -16, max_speckle_size 100,
max_diff 32 (cv2's speckleWindowSize = 100, speckleRange = 2).

Every GPU step is a child process of its own under a time limit (the check against the numpy definition at 2 x 48 x 160, then one
per shape); the parent never opens the GPU and stops at the first step that fails.  Timing: device events around `inner`
back-to-back calls after three warm-up calls of each, rounds repeated until the filter alone has run for --seconds (default
1 s) and at least 20 rounds; the figure is the median round's time per call.  Prints one JSON object and writes it to --out.

    python tools/speckle_probe.py --out profiles/speckle_probe.json
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

BYTES_PER_PIXEL = 30         # module docstring
NEW_VAL, MAX_SIZE, MAX_DIFF = -16, 100, 32
BATCH = 32
SHAPES = ((240, 320), (480, 640))
STEP_LIMIT_S = 240           # of one child


def scene(seed, batch, h, w):
    rng = np.random.default_rng([53, seed, h, w])
    xs = np.arange(w)[None, None, :] + 3 * np.arange(h)[None, :, None] + 40 * np.arange(batch)[:, None, None]
    d = (160 + xs // 2 % 640).astype(np.int16)
    noise = rng.random(d.shape)
    d[noise < 0.05] = rng.integers(0, 1024, int((noise < 0.05).sum()), dtype=np.int16)
    d[noise > 0.90] = NEW_VAL
    return d


def child(case, seconds):
    import torch
    from deepcharuco_amd import disparity as dp
    from sgm_probe import alternate
    assert torch.cuda.is_available(), "speckle_probe measures the GPU kernels: no GPU visible"
    dev = torch.device("cuda", 0)
    if case == "check":
        d = scene(0, 2, 48, 160)
        want = dp.filter_speckles_host(d, NEW_VAL, MAX_SIZE, MAX_DIFF)
        got = dp.filter_speckles_device(torch.from_numpy(d).to(dev), NEW_VAL, MAX_SIZE, MAX_DIFF).cpu().numpy()
        assert np.array_equal(got, want), "the device does not match the numpy definition"
        assert (want != d).any() and (want != NEW_VAL).any()
        print(json.dumps({"device": torch.cuda.get_device_name(dev), "check_removed": int((want != d).sum())}))
        return
    h, w = (int(v) for v in case.split("x"))
    src = torch.from_numpy(scene(1, BATCH, h, w)).to(dev)
    out = torch.empty_like(src)
    ws = torch.empty(dp.filter_speckles_workspace_bytes(BATCH, h, w), dtype=torch.uint8, device=dev)
    moved = BATCH * h * w * BYTES_PER_PIXEL
    cs, cd = torch.zeros(moved // 2, dtype=torch.uint8, device=dev), torch.empty(moved // 2, dtype=torch.uint8, device=dev)

    def speckle():
        return dp.filter_speckles_device(src, NEW_VAL, MAX_SIZE, MAX_DIFF, out=out, workspace=ws)

    def copy():
        cd.copy_(cs)

    ms, spread, inner, rounds = alternate({"speckle": speckle, "copy_floor": copy}, seconds)
    print(json.dumps({"speckle_ms": ms["speckle"], "copy_floor_ms": ms["copy_floor"], "speckle_over_floor": ms["speckle"] / ms["copy_floor"],
                      "bytes_moved": moved, "speckle_GBps": moved / ms["speckle"] / 1e6, "copy_GBps": moved / ms["copy_floor"] / 1e6,
                      "frames_per_s": BATCH / ms["speckle"] * 1e3, "min_max_ms": spread, "inner": inner, "rounds": rounds,
                      "removed_fraction": float((out != src).float().mean()), "valid_fraction": float((out != NEW_VAL).float().mean())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--case", default=None, help="internal: the one step that this process runs")
    a = ap.parse_args()
    if a.case:
        return child(a.case, a.seconds)
    result = {"seconds": a.seconds, "bytes_per_pixel": BYTES_PER_PIXEL, "batch": BATCH, "speckle": {}}
    for case in ["check"] + [f"{h}x{w}" for h, w in SHAPES]:
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--seconds", str(a.seconds)],
                             capture_output=True, text=True, timeout=STEP_LIMIT_S)
        if res.returncode != 0:
            sys.exit(f"step {case} failed with status {res.returncode}; nothing more is run:\n{res.stdout[-2000:]}{res.stderr[-4000:]}")
        step = json.loads(res.stdout.strip().splitlines()[-1])
        print(case, json.dumps(step), flush=True)
        if case == "check":
            result.update(step)
        else:
            result["speckle"][f"{BATCH}x{case}"] = step
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f)


if __name__ == "__main__":
    main()
