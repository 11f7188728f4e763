"""Wall time of the device rig pose solve (rig.rig_pose_pools, csrc/dcx_rigpose.hip) at 4,096 timestamps of 16 rows per view for rigs
of 2, 4 and 8 cameras, all-pinhole and alternating fisheye / pinhole, and in the same process the two yardsticks a caller without
it has: pnp.solve_pnp_pool on camera 0's pool alone (one camera's pose, the others' rows unused), and C per-camera pose calls
(solve_pnp_pool or fisheye.solve_pnp_fisheye_pool per camera: C unrelated poses, each in its own camera's frame).

Scenes: tests/fisheye_rig_exact.py's, sigma = 0.5 px, the 7x11 board (60 ids), the cameras on an arc from -35 to +35 degrees (C = 2:
0 and 30), the pinholes P, P0 in turn or (alternating) the lenses F, F0 and the pinholes P, P0 in turn, every camera seeing every
timestamp, the scene's true rig held fixed; "16 rows" = a random 16 of the 60 ids per view.  Every call is enqueued with its
workspace and outputs preallocated and timed to the stream's end: the median of `--reps` (7) calls after one warm-up, the pools
already on the device.  `rocprofv3 --kernel-trace --stats -- python tools/rigpose_probe.py` gives the per-kernel times.  Prints one
JSON object and writes it to --out.

    python tools/rigpose_probe.py --out profiles/rigpose_probe.json
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
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--stamps", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import fisheye_rig_exact as frx
    import rigpose_exact as px
    from deepcharuco_amd import corner_pool, fisheye, pnp, rig
    assert torch.cuda.is_available(), "rigpose_probe measures the GPU kernels: no GPU visible"
    dev = torch.device("cuda", 0)
    lens = {"fisheye": ("F", "F0"), "pinhole": ("P", "P0")}
    result = {"device": torch.cuda.get_device_name(dev), "sigma_px": 0.5, "stamps": a.stamps, "rows": a.rows, "reps": a.reps}
    for kind, of in (("pinhole", lambda c: "pinhole"), ("alternating", lambda c: ("fisheye", "pinhole")[c % 2])):
        part = {"cams": {}, "rig_pose_ms": {}, "camera0_pnp_ms": {}, "per_camera_pnp_ms": {}, "ok": {}, "lm_steps_mean": {},
                "rms_px_median": {}, "camera0_rms_px_median": {}}
        for n_cams in (2, 4, 8):
            key = f"C{n_cams}"
            angles = (0, 30) if n_cams == 2 else tuple(np.linspace(-35, 35, n_cams).tolist())
            names = tuple(lens[of(c)][(c // 2) % 2] for c in range(n_cams))
            s = frx.scene(4000 + n_cams, a.stamps, angles, names, sigma=0.5, rows=a.rows)
            cameras, dists = frx.cam_args(s)
            models = frx.models(s)
            packs = [corner_pool.pack_keypoints(k, dev) for k in s.kps]
            packed, pools = [p[0] for p in packs], [p[2] for p in packs]
            R, T = px.rig_rt(s.X)
            ws = torch.empty(rig.rig_pose_workspace_bytes(n_cams, a.stamps, pools), dtype=torch.uint8, device=dev)
            out = rig.rig_pose_pools(packed, a.stamps, pools, True, *s.board, cameras, dists, (R, T), models=models, workspace=ws)
            ms, got = timed(lambda: rig.rig_pose_pools(packed, a.stamps, pools, True, *s.board, cameras, dists, (R, T), models=models,
                                                       workspace=ws, out=out), a.reps)
            r = rig.unpack_rig_poses(*got)
            solve = [fisheye.solve_pnp_fisheye_pool if m == "fisheye" else pnp.solve_pnp_pool for m in models]
            outs = [solve[c](packed[c], a.stamps, pools[c], True, *s.board, cameras[c], dists[c]) for c in range(n_cams)]
            ms0, own = timed(lambda: solve[0](packed[0], a.stamps, pools[0], True, *s.board, cameras[0], dists[0], out=outs[0]), a.reps)
            msc, _ = timed(lambda: [solve[c](packed[c], a.stamps, pools[c], True, *s.board, cameras[c], dists[c], out=outs[c])
                                    for c in range(n_cams)], a.reps)
            ok = r.status == pnp.PNP_OK
            part["cams"][key] = list(names)
            part["rig_pose_ms"][key], part["camera0_pnp_ms"][key], part["per_camera_pnp_ms"][key] = ms, ms0, msc
            part["ok"][key] = int(ok.sum())
            part["lm_steps_mean"][key] = float(r.iterations[ok].mean())
            part["rms_px_median"][key] = float(np.median(r.rms[ok]))
            part["camera0_rms_px_median"][key] = float(np.median(own[1].cpu().numpy()[:, 6]))
            print(kind, key, json.dumps({k: v.get(key) for k, v in part.items()}), flush=True)
        result[kind] = part
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f)


if __name__ == "__main__":
    main()
