"""Is the rig calibration as fast through this tree's library as through another build's (the parent commit's)?
rig.rig_calibrate_pools on tools/rig_probe.py's scenes (4,096 timestamps x 16 rows; rigs of PROBE_CAMS cameras, default 2,4,8;
all-pinhole, or with --models that tool's rigs with the cycle's models), the base library against this tree's: the scenes are made once, then one child process per measurement (a process binds one
library), alternating base / this for PROBE_ROUNDS rounds (default 3); per process the median of 9 calls after a warm-up.  The
margin is the spread (max - min) of the base's own process medians.  Also says whether every run gave the same bits.  Prints one
JSON object and writes it to --out; this is what made the all_pinhole_parent_vs_this block of profiles/rig_probe_fisheye.json.

    git worktree add /tmp/base <parent> && make -C /tmp/base/deepcharuco_amd/csrc
    python tools/rig_old_new.py --base-lib /tmp/base/deepcharuco_amd/libdeepcharuco_amd.so --out profiles/rig_old_new.json
    python tools/rig_old_new.py --models fisheye,pinhole --base-lib ... --out ...
"""
import argparse, ctypes, json, os, pickle, subprocess, sys, tempfile, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests"))
STAMPS, ROWS, REPS = 4096, 16, 9
CAMS = tuple(int(v) for v in os.environ.get("PROBE_CAMS", "2,4,8").split(","))
ROUNDS = int(os.environ.get("PROBE_ROUNDS", "3"))

def worker(path):
    import torch
    from deepcharuco_amd import _lib, corner_pool, rig
    have = ctypes.CDLL(_lib.LIB_PATH)
    for name in [n for n in _lib.SIGNATURES if not hasattr(have, n)]:
        _lib.SIGNATURES.pop(name)                                 # an older build lacks the entries added since
    dev = torch.device("cuda", 0)
    out = {}
    for key, (kps, board, cameras, dists, models) in pickle.load(open(path, "rb")).items():
        packs = [corner_pool.pack_keypoints(k, dev) for k in kps]
        packed, pools = [p[0] for p in packs], [p[2] for p in packs]
        call = lambda: rig.rig_calibrate_pools(packed, STAMPS, pools, True, *board, cameras, dists, models=models)
        d = call()
        ts = []
        for _ in range(REPS):
            torch.cuda.synchronize(); t0 = time.perf_counter(); d = call(); ts.append((time.perf_counter() - t0) * 1e3)
        out[key] = {"ms": ts, "lm": [d.iterations, d.attempts], "rms": d.rms.hex() if hasattr(d.rms, "hex") else float(d.rms).hex(),
                    "T": [float(v).hex() for v in d.T.ravel()]}
    print("RESULT " + json.dumps(out), flush=True)

def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base-lib", required=True, help="the other build's libdeepcharuco_amd.so")
    ap.add_argument("--models", default=None, help="a cycle of camera models, e.g. fisheye,pinhole (unset: the all-pinhole run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import fisheye_rig_exact as frx
    import rig_exact as rx
    cycle, lens = a.models.split(",") if a.models else None, {"fisheye": ("F", "F0"), "pinhole": ("P", "P0")}
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
    path = os.path.join(tempfile.mkdtemp(), "scenes.pkl")
    pickle.dump(scenes, open(path, "wb"))
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
            print(name, rnd, {k: round(float(np.median(v["ms"])), 3) for k, v in res.items()}, flush=True)
    summary = {}
    for key in [f"C{n}" for n in CAMS]:
        med = {n: [float(np.median(r[key]["ms"])) for r in runs if r["lib"] == n] for n in libs}
        summary[key] = {"parent_medians_ms": med["parent"], "this_medians_ms": med["this"],
                        "parent_ms": float(np.median(med["parent"])), "this_ms": float(np.median(med["this"])),
                        "parent_spread_ms": max(med["parent"]) - min(med["parent"]),
                        "same_bits": len({(r[key]["rms"], tuple(r[key]["T"]), tuple(r[key]["lm"])) for r in runs}) == 1}
    print(json.dumps(summary, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"models": cycle, "stamps": STAMPS, "rows": ROWS, "reps": REPS, "summary": summary, "runs": runs}, f)

if __name__ == "__main__":
    worker(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[1] == "--worker" else main()
