"""Do the host definitions of calib, fisheye, stereo and rig return the bits another tree's do (the parent commit's), and are the
device wrappers as fast through this tree's Python as through that one's?

  (default)  every scene of scenes() through both trees on the CPU, each tree in a fresh child process with its own PYTHONPATH
             (the tree, then its tests/ for the scene builders); every field of every result is compared as bytes (an array by
             dtype, shape and a SHA-256 of its bytes, a float by its hex form, an exception by its type and text).  The scenes are
             the builders of tests/test_{calib,calib_ransac,fisheye,stereo,rig,fisheye_rig}_host.py: masks, pool_order, with_margin,
             models with a fisheye camera, every failure status those tests reach, the cv2-style tuples.
  --time     on a GPU: stereo_calibrate_pool, rig_calibrate_pools (C = 2, 4, 8), calibrate_charuco_pool and calibrate_fisheye_pool end
             to end on tools/rig_old_new.py's shapes, through both trees' Python and ONE library (this tree's: the parent's sources are
             the same), seven rounds each, alternating; per process the median of 9 calls after a warm-up.  The margin is the spread
             (max - min) of the parent's own process medians.
The other tree is --base-tree, or without it the parent commit unpacked with git archive into a scratch directory.  Prints a
summary and merges its block ("host" or "time") into --out.

    python tools/host_old_new.py --out profiles/host_old_new.json
    git archive HEAD^ | tar -x -C build/parent && python tools/host_old_new.py --time --base-tree build/parent --out profiles/host_old_new.json
"""
import argparse, hashlib, json, os, pickle, subprocess, sys, tempfile, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS, REPS = int(os.environ.get("PROBE_ROUNDS", "7")), 9

def flat(key, v, out):
    """One result -> out[key/field] = a string that is equal iff the bytes are"""
    if isinstance(v, tuple) and hasattr(v, "_fields"):
        for f, x in zip(v._fields, v):
            flat(f"{key}/{f}", x, out)
    elif isinstance(v, (tuple, list)):
        out[f"{key}/len"] = str(len(v))
        for i, x in enumerate(v):
            flat(f"{key}/{i}", x, out)
    elif isinstance(v, np.ndarray):
        out[key] = f"{v.dtype} {v.shape} {hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()}"
    elif isinstance(v, (float, np.floating)):
        out[key] = "float " + float(v).hex()
    else:
        out[key] = f"{type(v).__name__} {v!r}"

def scenes():
    """-> [(name, call)]; imported inside a child, so the modules are its tree's"""
    import camera_exact as cx, fisheye_exact as fx, fisheye_rig_exact as frx, rig_exact as rx, stereo_exact as sx
    import test_calib_host as tc, test_calib_ransac_host as tcr, test_fisheye_host as tf, test_fisheye_rig_host as tfr
    import test_rig_host as tr, test_stereo_host as ts
    from deepcharuco_amd import calib, fisheye as fe, pnp, rig, stereo
    out = []
    add = lambda name, call: out.append((name, call))
    # ---- calib
    objs, imgs, _, _ = tc.make_views(30, 20, sigma=0.3)
    col = np.arange(7) * 7
    m_col = imgs[0][:7] * 0 + np.c_[np.linspace(20, 300, 7), np.linspace(30, 200, 7)].astype(np.float32)
    objs2 = [objs[0][:3], objs[0][:0]] + objs[:10] + [pnp.object_points(col, *tc.BOARD)] + objs[10:]
    imgs2 = [imgs[0][:3], imgs[0][:0]] + imgs[:10] + [m_col] + imgs[10:]
    clean = tc.make_views(3, 24)
    add("calib/noisy20", lambda: calib.calibrate_camera_host_full(objs, imgs, tc.SIZE))
    add("calib/too_few+degenerate", lambda: calib.calibrate_camera_host_full(objs2, imgs2, tc.SIZE))
    add("calib/no_views", lambda: calib.calibrate_camera_host_full(objs2[:2], imgs2[:2], tc.SIZE))
    add("calib/clean24_f64", lambda: calib.calibrate_camera_host_full(*tc.make_views(1, 24, f32=False)[:2], tc.SIZE))
    add("calib/cv2_tuple", lambda: calib.calibrate_camera_host(*clean[:2], tc.SIZE))
    add("calib/cv2_raises_view", lambda: calib.calibrate_camera_host(objs2, imgs2, tc.SIZE))
    add("calib/cv2_raises_no_views", lambda: calib.calibrate_camera_host(objs2[:2], imgs2[:2], tc.SIZE))
    # ---- the consensus calibration
    for seed, sigma in tcr.SCENES:
        kps = tcr.scene(seed, sigma)[0]
        add(f"ransac/planted{seed}", lambda kps=kps: calib.calibrate_camera_ransac_host_full(kps, *tc.BOARD, tc.SIZE, with_margin=True))
    kps3 = tcr.scene(3, 0.0)[0]
    add("ransac/pool_order", lambda: calib.calibrate_camera_ransac_host_full(kps3, *tc.BOARD, tc.SIZE, pool_order=True, rounds=1))
    add("ransac/small_view", lambda: calib.calibrate_camera_ransac_host_full(tcr.small_view_batch()[0], *tc.BOARD, tc.SIZE, seed=tcr.SMALL_SEED))
    every = tcr.every_status_batch()[0]
    add("ransac/every_status", lambda: calib.calibrate_camera_ransac_host_full(every, *tc.BOARD, tc.SIZE))
    add("ransac/no_views", lambda: calib.calibrate_camera_ransac_host_full([every[2], every[3], every[9]], *tc.BOARD, tc.SIZE))
    add("ransac/cv2_tuple", lambda: calib.calibrate_camera_ransac_host(kps3, *tc.BOARD, tc.SIZE))
    add("ransac/cv2_raises_bad_id", lambda: calib.calibrate_camera_ransac_host(every, *tc.BOARD, tc.SIZE))
    add("ransac/cv2_raises_view", lambda: calib.calibrate_camera_ransac_host(every[:8], *tc.BOARD, tc.SIZE))
    # ---- fisheye
    for name, (K, k) in zip(tf.CAM_IDS, tf.CAMS):
        v = fx.make_views(11, 12, K, k)
        add(f"fisheye/{name}", lambda v=v: fe.calibrate_fisheye_host_full(v[0], v[1], fx.SIZE))
        add(f"fisheye/{name}/cv2_tuple", lambda v=v, K=K: fe.calibrate_fisheye_host(v[0], v[1], fx.SIZE, focal0=K[0, 0] * 1.1))
    fo, fi, _, _ = fx.make_views(11, 12, *tf.CAMS[1])
    add("fisheye/noisy", lambda: fe.calibrate_fisheye_host_full(*fx.make_views(5, 10, *tf.CAMS[1], sigma=0.3)[:2], fx.SIZE))
    add("fisheye/degenerate+too_few", lambda: fe.calibrate_fisheye_host_full(fo + [fo[0][:3]], fi + [fi[0][:3]], fx.SIZE, focal0=90.0))
    add("fisheye/no_views", lambda: fe.calibrate_fisheye_host_full([o[:3] for o in fo], [m[:3] for m in fi], fx.SIZE))
    add("fisheye/cv2_raises", lambda: fe.calibrate_fisheye_host(fo + [fo[0][:3]], fi + [fi[0][:3]], fx.SIZE))
    # ---- stereo
    full = lambda s, **kw: stereo.stereo_calibrate_host_full(s.kps0, s.kps1, *s.board, *sx.cam_args(s), **kw)
    for rg, c0, c1, board in ts.TRUTH_CASES[::4] + ts.TRUTH_CASES[1:2]:
        add(f"stereo/truth/{rg}/{c0}{c1}", lambda a=(1, 6, rg, board, c0, c1): full(sx.scene(*a), with_margin=True))
    for rg, c0, c1 in (("small", "A", "B"), ("toe90", "B", "C"), ("r170", "C", "A")):
        add(f"stereo/noisy/{rg}", lambda a=(2, 5, rg, sx.BOARD_S, c0, c1): full(sx.scene(*a, sigma=0.3), with_margin=True))
    seven = lambda seed: np.random.default_rng(seed).integers(6, 21, (7, 2)).tolist()       # seven timestamps, 6-20 rows per view
    for seed in range(4):
        rows = [tuple(r) for r in seven(seed)]
        add(f"stereo/seven/{seed}", lambda seed=seed, rows=rows: full(sx.scene(20 + seed, 7, "toe90", sx.BOARD_S, "A", "B", sigma=0.3, rows=rows)))
    add("stereo/disjoint", lambda: full(sx.scene(3, 6, "toe90", sx.BOARD_S, "A", "B", disjoint=True)))
    book = ts._bookkeeping_scene()[0]
    add("stereo/too_few+bad_id", lambda: full(book, with_margin=True))
    add("stereo/no_pairs", lambda: stereo.stereo_calibrate_host_full([book.kps0[0][:3], book.kps0[1], np.zeros((0, 3))],
                                                                      [book.kps1[0], np.zeros((0, 3)), book.kps1[3]], *book.board, *sx.cam_args(book), with_margin=True))
    planted, good = ts.planted_scene()
    add("stereo/masks", lambda: full(planted, masks=good, with_margin=True))
    add("stereo/masks/one_camera", lambda: full(planted, masks=(None, good[1])))
    add("stereo/masks/pool_order", lambda: full(planted, masks=good, pool_order=True))
    add("stereo/planted_unmasked", lambda: full(planted))
    used = [0, 3, 5, 6, 7]
    add("stereo/cv2_tuple", lambda: stereo.stereo_calibrate_host([book.kps0[t] for t in used], [book.kps1[t] for t in used], *book.board, *sx.cam_args(book)))
    add("stereo/cv2_raises_bad_id", lambda: stereo.stereo_calibrate_host(book.kps0, book.kps1, *book.board, *sx.cam_args(book)))
    add("stereo/cv2_raises_view", lambda: stereo.stereo_calibrate_host(book.kps0[:2], book.kps1[:2], *book.board, *sx.cam_args(book)))
    add("stereo/cv2_raises_empty_view", lambda: stereo.stereo_calibrate_host(book.kps0[4:6], [np.zeros((0, 3)), book.kps1[5]], *book.board, *sx.cam_args(book)))
    for cams in tfr.STEREO_PAIRS:
        for sigma in (0.0, 0.3):
            s = frx.scene(3, 6, (0, 30), cams, sigma=sigma)
            s = s._replace(kps=[s.kps[0][:2] + [s.kps[0][2][:3]] + s.kps[0][3:], list(s.kps[1])])
            args, kw = tfr.stereo_args(s)
            add(f"stereo/models/{'/'.join(cams)}/{sigma}", lambda args=args, kw=kw: stereo.stereo_calibrate_host_full(*args, with_margin=True, **kw))
        add(f"stereo/models/{'/'.join(cams)}/cv2_tuple", lambda args=args, kw=kw: stereo.stereo_calibrate_host(*[a[:2] if i < 2 else a for i, a in enumerate(args)], **kw))
    # ---- rig
    rfull = lambda s, **kw: rig.rig_calibrate_host_full(s.kps, *s.board, *rx.cam_args(s), **kw)
    add("rig/fan3", lambda: rfull(rx.scene(1, 8, **tr.FAN3), with_margin=True))
    add("rig/fan4", lambda: rfull(rx.scene(1, 8, **tr.FAN4), with_margin=True))
    add("rig/chain4", lambda: rfull(tr.chain_scene(), with_margin=True))
    add("rig/noisy/fan3", lambda: rfull(rx.scene(2, 5, sigma=0.3, rows=14, **tr.FAN3), with_margin=True))
    add("rig/noisy/fan4", lambda: rfull(rx.scene(2, 4, sigma=0.3, rows=12, **tr.FAN4)))
    add("rig/noisy/chain4", lambda: rfull(rx.scene(2, 6, visible=rx.chain_visibility(4, 2), sigma=0.3, rows=14, **tr.CHAIN4), with_margin=True))
    for sigma in (0.0, 0.3):
        s2 = rx.scene(3, 6, (0, 30), ("A", "B"), sigma=sigma)
        s2 = s2._replace(kps=[s2.kps[0][:2] + [s2.kps[0][2][:3]] + s2.kps[0][3:], list(s2.kps[1])])
        add(f"rig/two/{sigma}", lambda s2=s2: rfull(s2, with_margin=True))
    for seed in range(4):
        add(f"rig/two/seven/{seed}", lambda seed=seed: rfull(rx.scene(20 + seed, 7, (0, 30), ("A", "B"), sigma=0.3,
                                                                     rows=seven(seed))))
    rbook = tr._bookkeeping_scene()[0]
    add("rig/too_few+bad_id+lonely", lambda: rfull(rbook, with_margin=True))
    s9, none = rx.scene(4, 3, rows=9, **tr.FAN3), np.zeros((0, 3))
    kps9 = [[s9.kps[0][0], none, none], [none, s9.kps[1][1], none], [none, none, s9.kps[2][2][:3]]]
    add("rig/no_stamps", lambda: rig.rig_calibrate_host_full(kps9, *s9.board, *rx.cam_args(s9), with_margin=True))
    add("rig/disconnected", lambda: rfull(tr.disconnected_scene(), with_margin=True))
    rplanted, rgood = tr.planted_scene()
    add("rig/masks", lambda: rfull(rplanted, masks=rgood, with_margin=True))
    add("rig/masks/one_camera", lambda: rfull(rplanted, masks=[None, rgood[1], None]))
    add("rig/masks/pool_order", lambda: rfull(rplanted, masks=rgood, pool_order=True))
    add("rig/planted_unmasked", lambda: rfull(rplanted))
    add("rig/cv2_tuple", lambda: rig.rig_calibrate_host([[kl[t] for t in (0, 4, 5, 6)] for kl in rbook.kps], *rbook.board, *rx.cam_args(rbook)))
    add("rig/cv2_raises_bad_id", lambda: rig.rig_calibrate_host(rbook.kps, *rbook.board, *rx.cam_args(rbook)))
    add("rig/cv2_raises_view", lambda: rig.rig_calibrate_host([kl[:2] for kl in rbook.kps], *rbook.board, *rx.cam_args(rbook)))
    add("rig/cv2_raises_no_stamps", lambda: rig.rig_calibrate_host(kps9, *s9.board, *rx.cam_args(s9)))
    for name in tfr.CLASSES:
        for sigma in (0.0, 0.3):
            add(f"rig/models/{name}/{sigma}", lambda name=name, sigma=sigma: tfr.solve(tfr.class_scene(name, 1 if sigma == 0 else 2, sigma=sigma), with_margin=True))
    add("rig/models/outside", lambda: tfr.solve(tfr.outside_scene()[0], with_margin=True))
    add("rig/models/on_axis", lambda: tfr.solve(tfr.on_axis_scene(), with_margin=True))
    add("rig/models/wide", lambda: tfr.solve(tfr.wide_scene(0.3), with_margin=True))
    add("rig/models/disconnected", lambda: tfr.solve(tfr.disconnected_scene()))
    so = tfr.outside_scene()[0]
    add("rig/models/cv2_raises_view", lambda: rig.rig_calibrate_host(so.kps, *so.board, *frx.cam_args(so), models=frx.models(so)))
    return out

def host_worker(path):
    got, names = {}, []
    for name, call in scenes():
        try:
            r = call()
        except Exception as e:                       # what a scene raises is part of what it returns
            r = ("raised", type(e).__name__, str(e))
        flat(name, r, got)
        names.append(name)
    json.dump({"scenes": names, "fields": got}, open(path, "w"))

def timed(call):
    import torch
    call(); ts = []
    for _ in range(REPS):
        torch.cuda.synchronize(); t0 = time.perf_counter(); call(); torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))

def time_worker(path):
    import torch
    from deepcharuco_amd import calib, corner_pool, fisheye as fe, rig, stereo
    rigs, frames, board, size = pickle.load(open(path, "rb"))
    dev, got = torch.device("cuda", 0), {}
    for key, (kps, rboard, cameras, dists) in rigs.items():
        packs = [corner_pool.pack_keypoints(k, dev) for k in kps]
        packed, pools, B = [p[0] for p in packs], [p[2] for p in packs], len(kps[0])
        got[f"rig_calibrate_pools/{key}"] = timed(lambda: rig.rig_calibrate_pools(packed, B, pools, True, *rboard, cameras, dists))
        if len(kps) == 2:
            got["stereo_calibrate_pool"] = timed(lambda: stereo.stereo_calibrate_pool(packed[0], packed[1], B, pools[0], pools[1], True, *rboard,
                                                                                      cameras[0], dists[0], cameras[1], dists[1]))
    packed, b, pool = corner_pool.pack_keypoints(frames, dev)
    got["calibrate_charuco_pool"] = timed(lambda: calib.calibrate_charuco_pool(packed, b, pool, True, *board, size))
    got["calibrate_fisheye_pool"] = timed(lambda: fe.calibrate_fisheye_pool(packed, b, pool, True, *board, size))
    json.dump(got, open(path + ".out", "w"))

def child(tree, mode, path, lib=None):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([tree, os.path.join(tree, "tests")]))
    if lib:
        env["DCX_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, path], env=env, cwd=tree, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        print(r.stdout[-2000:], r.stderr[-4000:]); sys.exit(r.returncode or 1)

def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base-tree", default=None, help="the other tree (default: the parent commit, unpacked with git archive)")
    ap.add_argument("--time", action="store_true", help="time the device wrappers instead (needs a GPU)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    tmp = tempfile.mkdtemp()
    base = a.base_tree and os.path.abspath(a.base_tree)
    if base is None:
        base = os.path.join(tmp, "parent")
        os.makedirs(base)
        subprocess.run(f"git -C {REPO} archive HEAD^ | tar -x -C {base}", shell=True, check=True)
    trees = {"parent": base, "this": REPO}
    if not a.time:
        got, names = {}, {}
        for name, tree in trees.items():
            child(tree, "--host-worker", os.path.join(tmp, name + ".json"))
            doc = json.load(open(os.path.join(tmp, name + ".json")))
            got[name], names[name] = doc["fields"], doc["scenes"]
        assert names["parent"] == names["this"]
        keys = sorted(set(got["parent"]) | set(got["this"]))
        moved = [k for k in keys if got["parent"].get(k) != got["this"].get(k)]
        block = {"scenes": len(names["this"]), "fields": len(keys),
                 "fields_moved": moved, "raised": sorted(k[:-2] for k in keys if k.endswith("/0") and got["this"].get(k) == "str 'raised'"),
                 "numpy": np.__version__}
        for k in moved:
            print("MOVED", k, got["parent"].get(k), got["this"].get(k))
        print(json.dumps({k: v for k, v in block.items()}, indent=1))
    else:
        sys.path[:0] = [REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tools")]
        import fisheye_probe as fp, rig_old_new as ron
        rigs = {k: v[:4] for k, v in ron.rig_scenes(None).items()}
        path = os.path.join(tmp, "scenes.pkl")
        pickle.dump((rigs, ron.calib_scenes(), fp.BOARD, fp.SIZE), open(path, "wb"))
        lib = os.path.join(REPO, "deepcharuco_amd", "libdeepcharuco_amd.so")
        runs = {n: [] for n in trees}
        for rnd in range(ROUNDS):
            for name, tree in trees.items():
                child(tree, "--time-worker", path, lib)
                runs[name].append(json.load(open(path + ".out")))
                print(name, rnd, {k: round(v, 3) for k, v in runs[name][-1].items()}, flush=True)
        block = {"rounds": ROUNDS, "reps": REPS, "stamps": ron.STAMPS, "cases": {}}
        for key in runs["this"][0]:
            p, t = [r[key] for r in runs["parent"]], [r[key] for r in runs["this"]]
            block["cases"][key] = {"parent_medians_ms": p, "this_medians_ms": t, "parent_ms": float(np.median(p)), "this_ms": float(np.median(t)),
                                   "parent_spread_ms": max(p) - min(p), "inside": abs(float(np.median(t)) - float(np.median(p))) <= max(p) - min(p)
                                   or float(np.median(t)) <= float(np.median(p))}
        print(json.dumps({k: {f: v for f, v in c.items() if not f.endswith("medians_ms")} for k, c in block["cases"].items()}, indent=1))
        moved = [k for k, c in block["cases"].items() if not c["inside"]]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
        doc["time" if a.time else "host"] = block
        json.dump(doc, open(a.out, "w"), indent=1)
    sys.exit(1 if moved else 0)

if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] in ("--host-worker", "--time-worker"):
        (host_worker if sys.argv[1] == "--host-worker" else time_worker)(sys.argv[2])
    else:
        main()
