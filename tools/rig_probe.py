"""Wall time of the device rig calibration (rig.rig_calibrate_pools, csrc/dcx_rig.hip) at 4,096 timestamps of 16 rows per view for
rigs of 2, 4 and 8 cameras, its LM step and attempt counts, and in the same process the two yardsticks: the stereo solver
(stereo.stereo_calibrate_pool) on the first two cameras of the same scene -- the same launch chain with a 6x6 shared block -- and
the host fp64 definition (rig.rig_calibrate_host_full) on the same inputs.

Scenes: tests/rig_exact.py's, sigma = 0.5 px, the 7x11 board (60 ids), the cameras on an arc from -35 to +35 degrees (C = 2: 0 and
30) with the models A, B, C, A4 in turn, every camera seeing every timestamp; "16 rows" = a random 16 of the 60 ids per view.
Device wall time: the whole call (it synchronises: the tree, the medians and the LM loop's state word are read on the host),
median of `--reps` calls after one warm-up, the pools already on the device.  With `--models` (a cycle of pinhole / fisheye, e.g.
`--models fisheye,pinhole`) the scenes are tests/fisheye_rig_exact.py's of the same geometry with camera c's model taken from the
cycle (fisheye: the lenses F, F0 in turn; pinhole: P, P0), measured beside the all-pinhole rig (P, P0 in turn) of that geometry in the
same process; the stereo yardstick is left out (the stereo solver takes pinholes only).  `rocprofv3 --kernel-trace --stats -- python
tools/rig_probe.py --no-host` gives the per-kernel times.  Prints one JSON object and writes it to --out.

    python tools/rig_probe.py --out profiles/rig_probe.json
    python tools/rig_probe.py --models fisheye,pinhole --no-host --out profiles/rig_probe_fisheye.json
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


def mixed(a, dev):
    """--models: rigs of 2, 4 and 8 cameras with the cycle's models beside the all-pinhole rig of the same geometry."""
    import fisheye_rig_exact as frx
    import rig_exact as rx
    from deepcharuco_amd import corner_pool, rig
    cycle = a.models.split(",")
    assert all(m in rig.MODELS for m in cycle), f"--models takes a comma-separated cycle of {rig.MODELS}"
    lens = {"fisheye": ("F", "F0"), "pinhole": ("P", "P0")}
    result = {"models": cycle, "sigma_px": 0.5, "stamps": a.stamps, "rows": a.rows, "reps": a.reps, "cams": {}, "mixed_ms": {},
              "mixed_lm": {}, "pinhole_ms": {}, "pinhole_lm": {}, "mixed_us_per_attempt": {}, "pinhole_us_per_attempt": {},
              "host_ms": {}, "device_host_gap": {}}
    for n_cams in (2, 4, 8):
        key = f"C{n_cams}"
        angles = (0, 30) if n_cams == 2 else tuple(np.linspace(-35, 35, n_cams).tolist())
        for kind, of in (("mixed", lambda c: cycle[c % len(cycle)]), ("pinhole", lambda c: "pinhole")):
            names = tuple(lens[of(c)][(c // 2) % 2] for c in range(n_cams))
            s = frx.scene(4000 + n_cams, a.stamps, angles, names, sigma=0.5, rows=a.rows)
            cameras, dists = frx.cam_args(s)
            models = frx.models(s) if kind == "mixed" else None
            packs = [corner_pool.pack_keypoints(k, dev) for k in s.kps]
            packed, pools = [p[0] for p in packs], [p[2] for p in packs]
            ms, d = timed(lambda: rig.rig_calibrate_pools(packed, a.stamps, pools, True, *s.board, cameras, dists, models=models), a.reps)
            assert d.status == rig.RIG_OK, (key, kind, d.status)
            result[kind + "_ms"][key], result[kind + "_lm"][key] = ms, [d.iterations, d.attempts]
            result[kind + "_us_per_attempt"][key] = 1e3 * ms / d.attempts
            if kind == "mixed":
                result["cams"][key] = list(names)
                if not a.no_host and n_cams <= a.host_max_cams:
                    t0 = time.perf_counter()
                    h = rig.rig_calibrate_host_full(s.kps, *s.board, cameras, dists, models=models)
                    result["host_ms"][key] = (time.perf_counter() - t0) * 1e3
                    result["device_host_gap"][key] = {
                        "R_abs": float(np.abs(d.R - h.R).max()),
                        "T_rel": float(np.max(np.linalg.norm(d.T[1:] - h.T[1:], axis=1) / np.linalg.norm(h.T[1:], axis=1))),
                        "rms_rel": abs(d.rms - h.rms) / h.rms, "host_lm": [h.iterations, h.attempts], "rig_error": list(rx.rig_errors(d, s))}
        print(key, json.dumps({k: v.get(key) for k, v in result.items() if isinstance(v, dict)}), flush=True)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stamps", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--no-host", action="store_true", help="skip the host definition (for a profiler run)")
    ap.add_argument("--host-max-cams", type=int, default=8, help="run the host definition only up to this many cameras")
    ap.add_argument("--models", default=None, help="a cycle of camera models, e.g. fisheye,pinhole (unset: the all-pinhole run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import rig_exact as rx
    import stereo_exact as sx
    from deepcharuco_amd import corner_pool, rig, stereo
    assert torch.cuda.is_available(), "rig_probe measures the GPU kernels: no GPU visible"
    dev = torch.device("cuda", 0)
    if a.models:
        result = {"device": torch.cuda.get_device_name(dev), **mixed(a, dev)}
        print(json.dumps(result))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(result, f)
        return
    result = {"device": torch.cuda.get_device_name(dev), "board": list(sx.BOARD_S), "sigma_px": 0.5, "stamps": a.stamps, "rows": a.rows,
              "reps": a.reps, "rig_ms": {}, "lm_steps": {}, "lm_attempts": {}, "stereo01_ms": {}, "stereo_lm_steps": {},
              "stereo_lm_attempts": {}, "rig_over_stereo": {}, "rig_us_per_attempt": {}, "stereo_us_per_attempt": {}, "host_ms": {},
              "device_host_gap": {}}
    for n_cams in (2, 4, 8):
        key = f"C{n_cams}"
        angles = (0, 30) if n_cams == 2 else tuple(np.linspace(-35, 35, n_cams).tolist())
        names = tuple(("A", "B", "C", "A4")[c % 4] for c in range(n_cams))
        s = rx.scene(4000 + n_cams, a.stamps, angles, names, sigma=0.5, rows=a.rows)
        cameras, dists = rx.cam_args(s)
        packs = [corner_pool.pack_keypoints(k, dev) for k in s.kps]
        packed, pools = [p[0] for p in packs], [p[2] for p in packs]
        ms, d = timed(lambda: rig.rig_calibrate_pools(packed, a.stamps, pools, True, *s.board, cameras, dists), a.reps)
        assert d.status == rig.RIG_OK, (key, d.status)
        sms, st = timed(lambda: stereo.stereo_calibrate_pool(packed[0], packed[1], a.stamps, pools[0], pools[1], True, *s.board,
                                                             cameras[0], dists[0], cameras[1], dists[1]), a.reps)
        assert st.status == stereo.STEREO_OK, (key, st.status)
        result["rig_ms"][key], result["lm_steps"][key], result["lm_attempts"][key] = ms, d.iterations, d.attempts
        result["stereo01_ms"][key], result["stereo_lm_steps"][key], result["stereo_lm_attempts"][key] = sms, st.iterations, st.attempts
        result["rig_over_stereo"][key] = ms / sms
        result["rig_us_per_attempt"][key], result["stereo_us_per_attempt"][key] = 1e3 * ms / d.attempts, 1e3 * sms / st.attempts
        if not a.no_host and n_cams <= a.host_max_cams:
            t0 = time.perf_counter()
            h = rig.rig_calibrate_host_full(s.kps, *s.board, cameras, dists)
            result["host_ms"][key] = (time.perf_counter() - t0) * 1e3
            result["device_host_gap"][key] = {
                "R_abs": float(np.abs(d.R - h.R).max()),
                "T_rel": float(np.max(np.linalg.norm(d.T[1:] - h.T[1:], axis=1) / np.linalg.norm(h.T[1:], axis=1))),
                "rms_rel": abs(d.rms - h.rms) / h.rms, "host_steps": h.iterations, "host_attempts": h.attempts,
                "stamps": [d.stamps_used, h.stamps_used], "rig_error": list(rx.rig_errors(d, s))}
        print(key, json.dumps({k: v.get(key) for k, v in result.items() if isinstance(v, dict)}), flush=True)
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f)


if __name__ == "__main__":
    main()
