"""Wall time of the device stereo calibration (stereo.stereo_calibrate_pool, csrc/dcx_stereo.hip) at 64, 512 and 4,096 pairs of 16
and of 49 rows per view, its LM step and attempt counts, the host fp64 definition's wall time (stereo.stereo_calibrate_host_full)
on the same inputs, and, in the same process, the yardstick: the intrinsics calibration (calib.calibrate_charuco_pool) on camera
0's views of the same scenes -- the same launch pattern with a 9x9 shared block instead of a 6x6 one and half the rows.

Scenes: tests/stereo_exact.py's, sigma = 0.5 px, the 7x11 board (60 ids), cameras A (no distortion) and B (five coefficients), the
90 degree toe-in rig; "16 rows" = a random 16 of the 60 ids per view, drawn independently for the two cameras.  Device wall time:
the whole call (it synchronises: the rig init's medians and the LM loop's state word are read on the host), median of `--reps`
calls after one warm-up, the pools already on the device; "bits" is the result's rms and T as hex, to compare two builds (DCX_LIB
selects one).  `rocprofv3 --kernel-trace --stats -- python tools/stereo_probe.py --no-host` gives the per-kernel times.  Prints one JSON object and writes it to --out.

    python tools/stereo_probe.py --out profiles/stereo_probe.json
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


def timed(fn, reps):
    import torch
    out = fn()                                                 # warm-up
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), out


def kernel_stats(path):
    """The stereo and calibration kernels of a rocprofv3 --kernel-trace result (rocpd .db): calls, total and MEDIAN duration."""
    import sqlite3
    cur = sqlite3.connect(path).cursor()
    cols = [r[1] for r in cur.execute("pragma table_info(kernels)")]
    name_col = "name" if "name" in cols else [c for c in cols if "name" in c][0]
    by = {}
    for name, dur in cur.execute(f"select {name_col}, end - start from kernels"):
        m = re.search(r"((?:stereo|calib)_\w+?)_kernel", name)       # e.g. "(anonymous namespace)::stereo_schur_kernel(Ws)"
        if m:
            by.setdefault(m.group(1), []).append(dur)
    print("rocprofv3 --kernel-trace --stats -- python tools/stereo_probe.py --no-host: the stereo kernels and the yardstick's")
    print(f"{'kernel':<28} {'calls':>6} {'total_ms':>10} {'median_us':>10} {'min_us':>9} {'max_us':>9}")
    for name, d in sorted(by.items(), key=lambda kv: -sum(kv[1])):
        print(f"{name:<28} {len(d):6d} {sum(d) / 1e6:10.3f} {np.median(d) / 1e3:10.2f} {min(d) / 1e3:9.2f} {max(d) / 1e3:9.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-stats", default=None, metavar="DB", help="summarise a rocprofv3 result instead of measuring")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the host definition (for a profiler run)")
    ap.add_argument("--host-max-pairs", type=int, default=4096, help="run the host definition only up to this many pairs")
    ap.add_argument("--models", default=None, metavar="M0,M1",
                    help="the two cameras' models, pinhole or fisheye, e.g. fisheye,pinhole: tests/fisheye_rig_exact.py's scenes of two "
                         "cameras 30 degrees apart (fisheye: the lenses F, F0; pinhole: P, P0) through stereo_calibrate_pool(models=...); "
                         "the calibration yardstick is left out.  Unset: the all-pinhole run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats)
    import torch
    import stereo_exact as sx
    from deepcharuco_amd import calib, corner_pool, stereo
    assert torch.cuda.is_available(), "stereo_probe measures the GPU kernels: no GPU visible"
    dev = torch.device("cuda", 0)
    size0 = (320, 240)
    models = a.models.split(",") if a.models else None
    if models is not None:
        import fisheye_rig_exact as frx
        assert len(models) == 2 and all(m in stereo.MODELS for m in models), f"--models takes two of {stereo.MODELS}"
        names = tuple({"fisheye": ("F", "F0"), "pinhole": ("P", "P0")}[m][c] for c, m in enumerate(models))
    result = {"device": torch.cuda.get_device_name(dev), "board": list(sx.BOARD_S), "rig": "toe90", "cameras": "A/B", "sigma_px": 0.5,
              "reps": a.reps, "stereo_ms": {}, "lm_steps": {}, "lm_attempts": {}, "bits": {}, "calib_cam0_ms": {}, "calib_lm_steps": {},
              "calib_lm_attempts": {}, "stereo_over_calib": {}, "host_ms": {}, "device_host_gap": {}}
    for n_rows in (16, 49):
        for n_pairs in (64, 512, 4096):
            key = f"T{n_pairs}_n{n_rows}"
            if models is not None:
                m = frx.scene(3000 + n_pairs + n_rows, n_pairs, (0, 30), names, sigma=0.5, rows=n_rows)
                (K0, K1), (d0, d1) = frx.cam_args(m)
                kps0, kps1, cams, board = m.kps[0], m.kps[1], (K0, d0, K1, d1), m.board
                (p0, b, pool0), (p1, _, pool1) = corner_pool.pack_keypoints(kps0, dev), corner_pool.pack_keypoints(kps1, dev)
                ms, d = timed(lambda: stereo.stereo_calibrate_pool(p0, p1, b, pool0, pool1, True, *board, *cams, models=models), a.reps)
                assert d.status == stereo.STEREO_OK, (key, d.status)
                result["cameras"], result["rig"] = "/".join(names), "30 degrees"
                result["stereo_ms"][key], result["lm_steps"][key], result["lm_attempts"][key] = ms, d.iterations, d.attempts
                result["bits"][key] = {"rms": float(d.rms).hex(), "T": [float(v).hex() for v in np.ravel(d.T)]}
                if not a.no_host and n_pairs <= a.host_max_pairs:
                    t0 = time.perf_counter()
                    h = stereo.stereo_calibrate_host_full(kps0, kps1, *board, *cams, models=models)
                    result["host_ms"][key] = (time.perf_counter() - t0) * 1e3
                    result["device_host_gap"][key] = {
                        "R_abs": float(np.abs(d.R - h.R).max()), "T_rel": float(np.linalg.norm(d.T - h.T) / np.linalg.norm(h.T)),
                        "rms_rel": abs(d.rms - h.rms) / h.rms, "host_steps": h.iterations, "host_attempts": h.attempts,
                        "pairs": [d.pairs_used, h.pairs_used]}
                print(key, json.dumps({k: v.get(key) for k, v in result.items() if isinstance(v, dict)}), flush=True)
                continue
            s = sx.scene(3000 + n_pairs + n_rows, n_pairs, "toe90", sx.BOARD_S, "A", "B", sigma=0.5, rows=n_rows)
            cams = sx.cam_args(s)
            (p0, b, pool0), (p1, _, pool1) = corner_pool.pack_keypoints(s.kps0, dev), corner_pool.pack_keypoints(s.kps1, dev)
            ms, d = timed(lambda: stereo.stereo_calibrate_pool(p0, p1, b, pool0, pool1, True, *s.board, *cams), a.reps)
            assert d.status == stereo.STEREO_OK, (key, d.status)
            cms, c = timed(lambda: calib.calibrate_charuco_pool(p0, b, pool0, True, *s.board, size0), a.reps)
            assert c.status == calib.CALIB_OK, (key, c.status)
            result["stereo_ms"][key], result["lm_steps"][key], result["lm_attempts"][key] = ms, d.iterations, d.attempts
            result["bits"][key] = {"rms": float(d.rms).hex(), "T": [float(v).hex() for v in np.ravel(d.T)]}
            result["calib_cam0_ms"][key], result["calib_lm_steps"][key], result["calib_lm_attempts"][key] = cms, c.iterations, c.attempts
            result["stereo_over_calib"][key] = ms / cms
            if not a.no_host and n_pairs <= a.host_max_pairs:
                t0 = time.perf_counter()
                h = stereo.stereo_calibrate_host_full(s.kps0, s.kps1, *s.board, *cams)
                result["host_ms"][key] = (time.perf_counter() - t0) * 1e3
                result["device_host_gap"][key] = {
                    "R_abs": float(np.abs(d.R - h.R).max()), "T_rel": float(np.linalg.norm(d.T - h.T) / np.linalg.norm(h.T)),
                    "rms_rel": abs(d.rms - h.rms) / h.rms, "host_steps": h.iterations, "host_attempts": h.attempts,
                    "pairs": [d.pairs_used, h.pairs_used]}
            print(key, json.dumps({k: v.get(key) for k, v in result.items() if isinstance(v, dict)}), flush=True)
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f)


if __name__ == "__main__":
    main()
