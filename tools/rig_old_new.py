"""Is a solver as fast through this tree's library as through another build's (the parent commit's), and are the bits the same?
One runner, two scene sets (--set):
  rig    rig.rig_calibrate_pools on tools/rig_probe.py's scenes (4,096 timestamps x 16 rows; rigs of PROBE_CAMS cameras, default
         2,4,8; all-pinhole, or with --models that tool's rigs with the cycle's models).  This is what made the
         all_pinhole_parent_vs_this block of profiles/rig_probe_fisheye.json.
  calib  the single-camera entries of both camera models on tools/fisheye_probe.py's pool (64 noise-free views of 28 corners laid
         64 times into 4,096 views: the fisheye calibration crosses decide's 1,024-thread stride and fills all eight slices of
         reduce_solve): calibrate_charuco_pool, calibrate_fisheye_pool, and per model the undistort + rectify map at 640 x 480
         and the rectified points of that pool.  The pinhole calls get the fisheye pixels, as in that tool: same work, no fit.
The scenes are made once, then one child process per measurement (a process binds one library through DCX_LIB), alternating base /
this for PROBE_ROUNDS rounds (default 3); per process the median of 9 calls after a warm-up.  The margin is the spread (max - min)
of the base's own process medians.  same_bits: every run of a case, through either library, recorded the same result: for a
calibration theta, rms, steps, attempts and views as hex and a SHA-256 over every view's status, pose and rms; for a map or a point
array a SHA-256 over all of it.  Prints one JSON object and writes it to --out.

    git worktree add /tmp/base <parent> && make -C /tmp/base/deepcharuco_amd/csrc
    python tools/rig_old_new.py --base-lib /tmp/base/deepcharuco_amd/libdeepcharuco_amd.so --out profiles/rig_old_new.json
    python tools/rig_old_new.py --models fisheye,pinhole --base-lib ... --out ...
    python tools/rig_old_new.py --set calib --base-lib ... --out profiles/calib_old_new_shared.json
"""
import argparse, ctypes, hashlib, json, os, pickle, subprocess, sys, tempfile, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests")); sys.path.insert(0, os.path.join(REPO, "tools"))
STAMPS, ROWS, REPS = 4096, 16, 9
CAMS = tuple(int(v) for v in os.environ.get("PROBE_CAMS", "2,4,8").split(","))
ROUNDS = int(os.environ.get("PROBE_ROUNDS", "3"))
MAP_SIZE = (640, 480)

def timed(call):
    """-> the last result and the ms of REPS synchronised calls after one warm-up call"""
    import torch
    d, ts = call(), []
    for _ in range(REPS):
        torch.cuda.synchronize(); t0 = time.perf_counter(); d = call(); torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
    return d, ts

def rig_cases(scenes, dev):
    from deepcharuco_amd import corner_pool, rig
    for key, (kps, board, cameras, dists, models) in scenes.items():
        packs = [corner_pool.pack_keypoints(k, dev) for k in kps]
        packed, pools = [p[0] for p in packs], [p[2] for p in packs]
        d, ts = timed(lambda: rig.rig_calibrate_pools(packed, STAMPS, pools, True, *board, cameras, dists, models=models))
        yield key, {"ms": ts, "lm": [d.iterations, d.attempts], "rms": d.rms.hex() if hasattr(d.rms, "hex") else float(d.rms).hex(),
                    "T": [float(v).hex() for v in d.T.ravel()]}

def calib_cases(frames, dev):
    import torch
    import fisheye_probe as fp
    from deepcharuco_amd import calib, corner_pool, fisheye as fe, rectify as rc
    sha = lambda *arrays: hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)).hexdigest()
    packed, b, pool = corner_pool.pack_keypoints(frames, dev)
    for key, call in (("calibrate_charuco_pool", lambda: calib.calibrate_charuco_pool(packed, b, pool, True, *fp.BOARD, fp.SIZE)),
                      ("calibrate_fisheye_pool", lambda: fe.calibrate_fisheye_pool(packed, b, pool, True, *fp.BOARD, fp.SIZE))):
        d, ts = timed(call)
        yield key, {"ms": ts, "lm": [d.iterations, d.attempts], "status": d.status, "views": [d.views_used, d.points_used],
                    "rms": float(d.rms).hex(), "theta": [float(v).hex() for v in np.r_[d.camera_matrix.ravel(), d.dist_coeffs.ravel()]],
                    "views_sha256": sha(d.view_status, d.rvecs, d.tvecs, d.view_rms, d.view_points)}
    # a rectifying rotation and a new projection, so that no factor of the kernels is 0 or 1; the pinhole's five coefficients are
    # a lens of its own model (the fisheye's four mean something else there)
    r = np.array([0.02, -0.03, 0.01])
    th = np.linalg.norm(r); kx = np.cross(np.eye(3), r / th)
    R = np.eye(3) + np.sin(th) * kx + (1 - np.cos(th)) * kx @ kx
    P = np.array([[200.0, 0, 320.0, 0], [0, 200.0, 240.0, 0], [0, 0, 1, 0]])
    pin = np.array([-0.25, 0.08, 0.001, -0.0005, -0.01])
    maps = torch.empty((MAP_SIZE[1], MAP_SIZE[0], 2), dtype=torch.int32, device=dev)
    pts = torch.empty((pool, 2), dtype=torch.float64, device=dev)
    for key, call in (("map_pinhole", lambda: rc.undistort_rectify_map_device(fp.K, pin, R, P, *MAP_SIZE, out=maps)),
                      ("map_fisheye", lambda: fe.undistort_rectify_map_fisheye_device(fp.K, fp.DIST, R, P, *MAP_SIZE, out=maps)),
                      ("points_pinhole", lambda: rc.rectify_points_pool(packed, b, pool, True, fp.K, pin, R, P, out=pts)),
                      ("points_fisheye", lambda: fe.rectify_points_fisheye_pool(packed, b, pool, True, fp.K, fp.DIST, R, P, out=pts))):
        d, ts = timed(call)
        a = d.cpu().numpy()
        outside = np.isnan(a) if a.dtype.kind == "f" else a == rc.MAP_SENTINEL
        yield key, {"ms": ts, "shape": list(a.shape), "outside": int(outside.sum()), "sha256": sha(a)}

def worker(path):
    import torch
    from deepcharuco_amd import _lib
    have = ctypes.CDLL(_lib.LIB_PATH)
    for name in [n for n in _lib.SIGNATURES if not hasattr(have, n)]:
        _lib.SIGNATURES.pop(name)                                 # an older build lacks the entries added since
    which, scenes = pickle.load(open(path, "rb"))
    print("RESULT " + json.dumps(dict({"rig": rig_cases, "calib": calib_cases}[which](scenes, torch.device("cuda", 0)))), flush=True)

def rig_scenes(models):
    import fisheye_rig_exact as frx
    import rig_exact as rx
    cycle, lens = models.split(",") if models else None, {"fisheye": ("F", "F0"), "pinhole": ("P", "P0")}
    scenes = {}
    for n_cams in CAMS:
        angles = (0, 30) if n_cams == 2 else tuple(np.linspace(-35, 35, n_cams).tolist())
        if cycle:
            names = tuple(lens[cycle[c % len(cycle)]][(c // 2) % 2] for c in range(n_cams))
            s = frx.scene(4000 + n_cams, STAMPS, angles, names, sigma=0.5, rows=ROWS)
            scenes[f"C{n_cams}"] = (s.kps, s.board, *frx.cam_args(s), frx.models(s))
        else:
            names = tuple(("A", "B", "C", "A4")[c % 4] for c in range(n_cams))
            s = rx.scene(4000 + n_cams, STAMPS, angles, names, sigma=0.5, rows=ROWS)
            scenes[f"C{n_cams}"] = (s.kps, s.board, *rx.cam_args(s), None)
        print("scene", n_cams, flush=True)
    return scenes

def calib_scenes():
    import fisheye_probe as fp
    base = fp.scenes(64)
    return [base[i % 64] for i in range(STAMPS)]

def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base-lib", required=True, help="the other build's libdeepcharuco_amd.so")
    ap.add_argument("--set", default="rig", choices=("rig", "calib"), help="the scene set (see above)")
    ap.add_argument("--models", default=None, help="rig set: a cycle of camera models, e.g. fisheye,pinhole (unset: the all-pinhole run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    scenes = rig_scenes(a.models) if a.set == "rig" else calib_scenes()
    path = os.path.join(tempfile.mkdtemp(), "scenes.pkl")
    pickle.dump((a.set, scenes), open(path, "wb"))
    libs = {"parent": os.path.abspath(a.base_lib), "this": os.path.join(REPO, "deepcharuco_amd", "libdeepcharuco_amd.so")}
    runs = []
    for rnd in range(ROUNDS):
        for name in ("parent", "this"):
            env = dict(os.environ, DCX_LIB=libs[name])
            r = subprocess.run([sys.executable, __file__, "--worker", path], env=env, capture_output=True, text=True, timeout=240)
            if r.returncode != 0:
                print(r.stdout[-2000:], r.stderr[-4000:]); sys.exit(r.returncode or 1)
            res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
            runs.append({"lib": name, "round": rnd, **res})
            print(name, rnd, {k: round(float(np.median(v["ms"])), 4) for k, v in res.items()}, flush=True)
    summary = {}
    for key in [k for k in runs[0] if k not in ("lib", "round")]:
        med = {n: [float(np.median(r[key]["ms"])) for r in runs if r["lib"] == n] for n in libs}
        summary[key] = {"parent_medians_ms": med["parent"], "this_medians_ms": med["this"],
                        "parent_ms": float(np.median(med["parent"])), "this_ms": float(np.median(med["this"])),
                        "parent_spread_ms": max(med["parent"]) - min(med["parent"]),
                        "same_bits": len({json.dumps({f: v for f, v in r[key].items() if f != "ms"}, sort_keys=True) for r in runs}) == 1}
    print(json.dumps(summary, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"set": a.set, "models": a.models.split(",") if a.models else None, "stamps": STAMPS, "rows": ROWS if a.set == "rig" else 28, "reps": REPS,
                       "summary": summary, "runs": runs}, f)

if __name__ == "__main__":
    worker(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[1] == "--worker" else main()
