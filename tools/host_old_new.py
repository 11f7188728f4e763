"""Do the host definitions of calib, fisheye, stereo, rig, pnp and rectify return the bits another tree's do (the parent commit's),
and are the device wrappers as fast through this tree's Python as through that one's?

  (default)  every scene of scenes() through both trees on the CPU, each tree in a fresh child process with its own PYTHONPATH
             (the tree, then its tests/ for the scene builders); every field of every result is compared as bytes (an array by
             dtype, shape and a SHA-256 of its bytes, a float by its hex form, an exception by its type and text).  The scenes are
             the builders of tests/test_{calib,calib_ransac,fisheye,stereo,rig,fisheye_rig}_host.py: masks, pool_order, with_margin,
             models with a fisheye camera, every failure status those tests reach, the cv2-style tuples; and (pose_scenes) those of
             tests/test_{pnp,pnp_ransac,fisheye_ransac,rectify,rigpose,pose_exact}_host.py: the single-view pose solvers of both
             models plain and behind the consensus search, the rig pose, the maps, the rectified points, the rectifications, and the
             projection texts called directly with their Jacobians.  A second block, "oracles" (oracle_scenes), does the same for
             the exact modules those tests are held to: their scene builders and their residuals, costs, finite-difference Jacobians
             and stationarity.  With --suite it also holds the wall time of the six host test files that use them, three runs of
             each tree, alternating; this tree's median must be inside the parent's own spread.
  --time     on a GPU: stereo_calibrate_pool, rig_calibrate_pools (C = 2, 4, 8), calibrate_charuco_pool and calibrate_fisheye_pool end
             to end on tools/rig_old_new.py's shapes, and the per-batch wrappers of both models (solve_pnp_*pool, solve_pnp_*ransac_pool,
             rectify_points_*pool, undistort_rectify_map_*device) on its 4,096 views with out / workspace preallocated, through both
             trees' Python and ONE library (this tree's: the parent's sources are
             the same), seven rounds each, alternating; per process the median of 9 calls after a warm-up.  The margin is the spread
             (max - min) of the parent's own process medians.
The other tree is --base-tree, or without it the parent commit unpacked with git archive into a scratch directory.  Prints a
summary and merges its blocks ("host" and "oracles", or "time") into --out.

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
        if v.dtype == np.longdouble and v.itemsize == 16:      # an x87 long double is 10 bytes of value and 6 of padding
            v = np.ascontiguousarray(v).view(np.uint8).reshape(v.shape + (16,))[..., :10]
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
    pose_scenes(add)
    return out

def pose_scenes(add):
    """The single-view pose solvers, the rig pose, the maps, the rectified points and the shared texts called directly: the builders
    of tests/test_{pnp,pnp_ransac,fisheye,fisheye_ransac,rectify,rigpose,pose_exact}_host.py"""
    import camera_exact as cx, fisheye_exact as fx, fisheye_rig_exact as frx, rig_exact as rx, rigpose_exact as px, stereo_exact as sx
    import test_fisheye_host as tf, test_fisheye_ransac_host as tfa, test_fisheye_rig_host as tfr, test_pnp_host as tp
    import test_pnp_ransac_host as tpa, test_pose_exact_host as tpe, test_rectify_host as trc, test_rigpose_host as trp
    from deepcharuco_amd import calib, fisheye as fe, pnp, rectify as rc, rig, stereo
    pin = lambda c: sx.cam_args(sx.Scene(*[None] * 5, c, c, ""))[:2]     # (K, dist) of a name, by a function both trees have
    # ---- pnp: 0 / 4 / 5 / 8 coefficients, clean, 0.5 px and 30 px noise, plain and behind the consensus search
    for name, dist in (("none", None), ("0", np.zeros(0)), ("4", tp.DIST5[:4]), ("5", tp.DIST5), ("8", tp.DIST8)):
        for j, sigma in enumerate((0.0, 0.5, 30.0)):
            for seed in range(3):
                kp = tp.make_frame(np.random.default_rng([len(name), j, seed]), dist=np.zeros(5) if dist is None else dist, sigma=sigma)[0]
                add(f"pnp/{name}/{sigma}/{seed}", lambda kp=kp, dist=dist: pnp.solve_pnp_host_full(kp, *tp.BOARD, tp.K, dist))
                add(f"pnp/ransac/{name}/{sigma}/{seed}", lambda kp=kp, dist=dist, seed=seed: pnp.solve_pnp_ransac_host_full(
                    kp, *tp.BOARD, tp.K, dist, reproj_error=tpa.REPROJ, seed=seed, with_margin=True))
    for i, f in enumerate(tpe.A.grid()[::5]):
        add(f"pnp/exact_grid/{i}", lambda f=f: pnp.solve_pnp_host_full(f.kp, *f.board, tpe.A.K_EDGE, tpe.A.MODELS[f.model]))
    planted = tpa.planted_frames(8)
    for i, (kp, good, _) in enumerate(planted):
        perm = np.random.default_rng(i).permutation(len(kp))
        add(f"pnp/planted/{i}", lambda kp=kp: tpa._ransac(kp, with_margin=True))
        add(f"pnp/planted/{i}/pool_order", lambda kp=kp, perm=perm: tpa._ransac(kp[perm], pool_order=True, with_margin=True))
        add(f"pnp/planted/{i}/plain", lambda kp=kp: pnp.solve_pnp_host_full(kp, *tp.BOARD, tp.K, tp.DIST5))
    kp, good, _ = planted[0]
    lines = [tp.make_frame(np.random.default_rng(5), ids=ids)[0] for ids in ([0, 1, 2, 3], [0, 5, 10, 15], [1, 5, 9, 13, 1])]
    bad_id, skew = kp.copy(), tp.K.copy()
    bad_id[0, 2], skew[0, 1] = 16, 1.0
    wild = [kp.copy() for _ in range(4)]
    wild[0][3, 0], wild[1][5, 1], wild[2][:, :2], wild[3][:, :2] = np.inf, np.nan, kp[:, :2] * 1e30, kp[:, :2] * 1e-30
    for n in (0, 1, 3):
        add(f"pnp/too_few/{n}", lambda n=n: (pnp.solve_pnp_host_full(kp[:n], *tp.BOARD, tp.K, tp.DIST5), tpa._ransac(kp[:n], with_margin=True)))
    add("pnp/too_few/empty", lambda: (pnp.solve_pnp_host(np.array([]), *tp.BOARD, tp.K, tp.DIST5), tpa._ransac(np.array([]))))
    add("pnp/no_consensus", lambda: tpa._ransac(kp, min_inliers=int(good.sum()) + 1, with_margin=True))
    add("pnp/one_iteration", lambda: tpa._ransac(kp, iterations=1))
    add("pnp/tight", lambda: tpa._ransac(kp, iterations=4096, reproj_error=1e-3, with_margin=True))
    for i, kpc in enumerate(lines):
        add(f"pnp/degenerate/{i}", lambda kpc=kpc: (pnp.solve_pnp_host_full(kpc, *tp.BOARD, tp.K, tp.DIST5), tpa._ransac(kpc),
                                                     pnp.solve_pnp_host(kpc, *tp.BOARD, tp.K, tp.DIST5), pnp.solve_pnp_ransac_host(kpc, *tp.BOARD, tp.K, tp.DIST5)))
    for i, w in enumerate(wild):             # pixels no camera gives: an inf, a NaN, all of them far out of range, all of them at the corner
        for name, dist in (("5", tp.DIST5), ("none", None)):
            add(f"pnp/wild/{i}/{name}", lambda w=w, dist=dist: pnp.solve_pnp_host_full(w, *tp.BOARD, tp.K, dist))
            add(f"pnp/wild/{i}/{name}/ransac", lambda w=w, dist=dist: pnp.solve_pnp_ransac_host_full(w, *tp.BOARD, tp.K, dist, with_margin=True))
    add("pnp/cv2", lambda: (pnp.solve_pnp_host(kp, *tp.BOARD, tp.K, tp.DIST5), pnp.solve_pnp_ransac_host(kp, *tp.BOARD, tp.K, tp.DIST5),
                            pnp.solve_pnp_ransac_host(kp[:3], *tp.BOARD, tp.K, tp.DIST5), pnp.solve_pnp_host(np.rint(kp).astype(np.int64), *tp.BOARD, tp.K, tp.DIST5)))
    for name, call in (("12", lambda f: f(kp, *tp.BOARD, tp.K, np.zeros(12))), ("skew", lambda f: f(kp, *tp.BOARD, skew, tp.DIST5)),
                       ("bad_id", lambda f: f(bad_id, *tp.BOARD, tp.K, tp.DIST5))):
        add(f"pnp/raises/{name}", lambda call=call: call(pnp.solve_pnp_host))
        add(f"pnp/raises/{name}/ransac", lambda call=call: call(pnp.solve_pnp_ransac_host))
    for name, kw in (("iterations0", dict(iterations=0)), ("iterations4097", dict(iterations=4097)), ("reproj0", dict(reproj_error=0.0)), ("reproj_nan", dict(reproj_error=np.nan))):
        add(f"pnp/raises/{name}", lambda kw=kw: tpa._ransac(kp, **kw))
    # ---- fisheye: the four test cameras, clean, 0.5 px and 30 px noise; exchanged ids; a pixel outside the model
    for cam, (K, k) in zip(tf.CAM_IDS, tf.CAMS):
        for sigma in (0.0, 0.5, 30.0):
            _, imgs, ids_l, _ = fx.make_views(11, 3, K, k, sigma=sigma)
            for i, fk in enumerate(fx.keypoints(imgs, ids_l)):
                add(f"fisheye/pnp/{cam}/{sigma}/{i}", lambda fk=fk, K=K, k=k: fe.solve_pnp_fisheye_host_full(fk, *fx.BOARD, K, k))
                add(f"fisheye/ransac/{cam}/{sigma}/{i}", lambda fk=fk, K=K, k=k: fe.solve_pnp_fisheye_ransac_host_full(
                    fk, *fx.BOARD, K, k, reproj_error=tfa.REPROJ, seed=tfa.SEED, with_margin=True))
    swapped = tfa.swapped_views(3)
    for i, (fk, fgood, _) in enumerate(swapped):
        perm = np.random.default_rng(i).permutation(len(fk))
        add(f"fisheye/swapped/{i}", lambda fk=fk: tfa._ransac(fk, with_margin=True))
        add(f"fisheye/swapped/{i}/pool_order", lambda fk=fk, perm=perm: tfa._ransac(fk[perm], pool_order=True, with_margin=True))
        add(f"fisheye/swapped/{i}/plain", lambda fk=fk, fgood=fgood: (fe.solve_pnp_fisheye_host_full(fk, *fx.BOARD, tfa.K, tfa.KD),
                                                                       fe.solve_pnp_fisheye_host_full(fk[fgood], *fx.BOARD, tfa.K, tfa.KD)))
    fk = swapped[0][0]
    ko, Kn, kn = tfa._outside_view()
    for seed in range(8):
        add(f"fisheye/outside/one_iteration/{seed}", lambda seed=seed: fe.solve_pnp_fisheye_ransac_host_full(ko, *fx.BOARD, Kn, kn, iterations=1, reproj_error=tfa.REPROJ, seed=seed))
    add("fisheye/outside/ransac", lambda: fe.solve_pnp_fisheye_ransac_host_full(ko, *fx.BOARD, Kn, kn, reproj_error=tfa.REPROJ, seed=tfa.SEED, with_margin=True))
    add("fisheye/outside/plain", lambda: (fe.solve_pnp_fisheye_host_full(ko, *fx.BOARD, Kn, kn), fe.solve_pnp_fisheye_host(ko, *fx.BOARD, Kn, kn)))
    far_imgs, far_ids = fx.make_views(11, 12, *tf.CAMS[1])[1:3]
    for i, fkf in enumerate(fx.keypoints(far_imgs, far_ids)[:6]):     # views beyond a 90 px camera's field among them
        add(f"fisheye/start_camera/{i}", lambda fkf=fkf: fe.solve_pnp_fisheye_host_full(fkf, *fx.BOARD, fx.camera(90.0), None))
    add("fisheye/too_few", lambda: (tfa._ransac(fk[:3]), fe.solve_pnp_fisheye_host_full(fk[:3], *fx.BOARD, tfa.K, tfa.KD),
                                    fe.solve_pnp_fisheye_ransac_host(fk[:3], *fx.BOARD, tfa.K, tfa.KD)))
    add("fisheye/no_consensus", lambda: tfa._ransac(fk, min_inliers=26, with_margin=True))
    add("fisheye/cv2", lambda: (fe.solve_pnp_fisheye_host(fk, *fx.BOARD, tfa.K, tfa.KD), fe.solve_pnp_fisheye_ransac_host(fk, *fx.BOARD, tfa.K, tfa.KD, seed=tfa.SEED)))
    add("fisheye/raises/5", lambda: fe.solve_pnp_fisheye_ransac_host_full(fk, *fx.BOARD, tfa.K, np.zeros(5)))
    add("fisheye/raises/iterations0", lambda: tfa._ransac(fk, iterations=0))
    add("fisheye/raises/plain5", lambda: fe.solve_pnp_fisheye_host(fk, *fx.BOARD, tfa.K, np.zeros(5)))
    # ---- rig pose: masks, models that mix the two cameras, every status test_rigpose_host reaches
    for name in ("fan3", "chain4", "two", "mixed fan3 F/P/F"):
        add(f"rigpose/truth/{name}", lambda name=name: trp._solve(trp.TRUTH[name](), with_margin=True))
    for name in trp.NOISY:
        add(f"rigpose/noisy/{name}", lambda name=name: trp._solve(trp.NOISY[name](), with_margin=True))
    s5 = rx.scene(33, 5, sigma=0.3, rows=[[20, 2, 3], [3, 2, 1], [12, 2, 9], [12, 0, 9], [12, 9, 10]], **trp.FAN3)
    kps = [[k.copy() for k in kl] for kl in s5.kps]
    kps[1][2][1, 2], kps[1][3] = cx.n_ids(s5.board), np.zeros((0, 3))
    s5 = s5._replace(kps=kps)
    add("rigpose/statuses", lambda: trp._solve(s5, with_margin=True))
    add("rigpose/cv2_raises_bad_id", lambda: rig.rig_pose_host(s5.kps, *s5.board, *rx.cam_args(s5), px.rig_rt(s5.X)))
    add("rigpose/cv2", lambda: rig.rig_pose_host([[kl[t] for t in (0, 1, 3, 4)] for kl in s5.kps], *s5.board, *rx.cam_args(s5), px.rig_rt(s5.X)))
    for case in ("1", "3", "collinear"):
        n = 0 if case == "collinear" else int(case)
        sc = rx.scene(7, 3, sigma=0.3, rows=[[20, max(n, 1), max(n, 1)]] * 3, **trp.FAN3)
        if case == "collinear":
            sc = sc._replace(kps=[sc.kps[0], [trp._collinear_view(sc, t, 1) for t in range(3)], [np.zeros((0, 3))] * 3])
        add(f"rigpose/weak_rows/{case}", lambda sc=sc: trp._solve(sc, with_margin=True))
    for seed in range(3):
        add(f"rigpose/weak_camera_0/{seed}", lambda seed=seed: trp._solve(trp.weak_scene(seed), with_margin=True))
    s_out = tfr.outside_scene(sigma=0.3)[0]
    add("rigpose/outside", lambda: trp._solve(s_out, with_margin=True))
    add("rigpose/outside/cv2_raises_view", lambda: rig.rig_pose_host(s_out.kps, *s_out.board, *frx.cam_args(s_out), px.rig_rt(s_out.X), models=frx.models(s_out)))
    sm = rx.scene(53, 4, sigma=0.3, rows=[[20, 12, 9]] * 4, **trp.FAN3)
    rng = np.random.default_rng(8)
    masks = [[rng.random(n) < 0.7 for _ in range(4)] for n in (20, 12, 9)]
    masks[1][2][:], masks[2][3][:] = False, False
    masks[1][2][:2] = True
    add("rigpose/masks", lambda: trp._solve(sm, masks=masks, with_margin=True))
    add("rigpose/masks/pool_order", lambda: trp._solve(sm, masks=masks, pool_order=True))
    add("rigpose/masks/mixed", lambda: trp._solve(trp.NOISY["mixed fan3 F/P/F"](), masks=[None, [np.arange(14) % 3 > 0] * 4, None]))
    sr = rx.scene(3, 5, sigma=0.3, **trp.FAN3)
    solved = rig.rig_calibrate_host_full(sr.kps, *sr.board, *rx.cam_args(sr))
    add("rigpose/from_result", lambda: rig.rig_pose_host_full(sr.kps, *sr.board, *rx.cam_args(sr), solved))
    add("rigpose/raises_unsolved", lambda: rig.rig_pose_host_full(sr.kps, *sr.board, *rx.cam_args(sr), solved._replace(status=rig.RIG_NO_STAMPS)))
    # ---- the maps (48 x 64), the rectified points (NaN rows among them) and the rectifications of both models
    R100 = cx.f64(cx.rotation([0.0, np.deg2rad(100.0), 0.0]))
    Pw = np.array([[20.0, 0, 32.0], [0, 20.0, 24.0], [0, 0, 1]])
    pix = np.concatenate([trc.rx.pixel_grid(37), [[40000.0, 30000.0], [np.nan, 5.0], [160.0, 120.0]]])
    for kind, c0, c1 in trc.MAP_CASES:
        r = trc._rectify(kind, c0, c1)[0]
        for c, Rc, P in ((c0, r.R1, r.P1), (c1, r.R2, r.P2)):
            K, d = pin(c)
            for q in (True, False):
                add(f"map/{kind}/{c}/{q}", lambda K=K, d=d, Rc=Rc, P=P, q=q: rc.undistort_rectify_map_host(K, d, Rc, P, 64, 48, quantised=q))
            add(f"points/{kind}/{c}", lambda K=K, d=d, Rc=Rc, P=P: rc.rectify_points_host(pix, K, d, Rc, P))
    for c in ("A", "B", "C", "A4"):
        K, d = pin(c)
        for q in (True, False):
            add(f"map/plain/{c}/{q}", lambda K=K, d=d, q=q: rc.undistort_rectify_map_host(K, d, None, None, 64, 48, quantised=q))
            add(f"map/behind/{c}/{q}", lambda K=K, d=d, q=q: rc.undistort_rectify_map_host(K, d, R100, Pw, 64, 48, quantised=q))
        add(f"points/plain/{c}", lambda K=K, d=d: (rc.rectify_points_host(pix, K, d), rc.rectify_points_host(pix, K, d, R100), rc.undistort_points_newton(pix, K, d)))
    add("map/ties", lambda: rc.undistort_rectify_map_host(np.eye(3), None, None, np.diag([64.0, 64.0, 1.0]), 8, 1))
    add("map/raises/P", lambda: rc.undistort_rectify_map_host(*pin("B"), None, np.eye(4), 8, 8))
    add("map/raises/size", lambda: rc.undistort_rectify_map_host(*pin("B"), None, None, 0, 8))
    add("points/raises/dist", lambda: rc.rectify_points_host(pix, sx.K_A, np.zeros(12)))
    fpix = np.concatenate([pix, [[250.0, 240.0], [400.0, 240.0], [319.5 + 150.0 * 1.6, 239.5]]])
    for cam, (K, k) in zip(tf.CAM_IDS, tf.CAMS):
        for q in (True, False):
            add(f"fisheye/map/plain/{cam}/{q}", lambda K=K, k=k, q=q: fe.undistort_rectify_map_fisheye_host(K, k, None, None, 64, 48, quantised=q))
            add(f"fisheye/map/behind/{cam}/{q}", lambda K=K, k=k, q=q: fe.undistort_rectify_map_fisheye_host(K, k, R100, Pw, 64, 48, quantised=q))
        add(f"fisheye/points/{cam}", lambda K=K, k=k: (fe.rectify_points_fisheye_host(fpix, K, k), fe.rectify_points_fisheye_host(fpix, K, k, R100, Pw),
                                                        fe.undistort_points_host(fpix, K, k)))
    add("fisheye/map/limit", lambda: fe.undistort_rectify_map_fisheye_host(fx.camera(1e6), None, None, fx.camera(100.0), 64, 48, quantised=False))
    add("fisheye/map/raises/size", lambda: fe.undistort_rectify_map_fisheye_host(*tf.CAMS[1], None, None, 8, 0))
    add("fisheye/points/raises/dist", lambda: fe.rectify_points_fisheye_host(fpix, tf.CAMS[1][0], np.zeros(5)))
    for kind, c0, c1 in trc.CASES[::3]:
        for alpha in (None, 0.0, 0.5, 1.0):
            if alpha is None or kind != "toe90":
                add(f"rectify/{kind}/{c0}{c1}/{alpha}", lambda a=(kind, c0, c1, alpha): trc._rectify(*a)[0])
        Rr, Tr = trc.rx.rig_RT(kind, c0, c1)
        add(f"fisheye/rectify/{kind}", lambda Rr=Rr, Tr=Tr: (fe.stereo_rectify_fisheye_host(*tf.CAMS[1], *tf.CAMS[3], fx.SIZE, Rr, Tr),
                                                             fe.stereo_rectify_fisheye_host(*tf.CAMS[0], *tf.CAMS[1], fx.SIZE, Rr, Tr, focal=120.0)))
    add("rectify/raises/T", lambda: rc.stereo_rectify_host(*pin("B"), *pin("B"), trc.rx.SIZE, np.eye(3), [0.0, 0.0, 0.0]))
    add("fisheye/rectify/raises/focal", lambda: fe.stereo_rectify_fisheye_host(*tf.CAMS[1], *tf.CAMS[3], fx.SIZE, np.eye(3), [0.1, 0, 0], focal=0.0))
    # ---- the texts that move, called directly with the Jacobian on 40 random points
    rng = np.random.default_rng(2718)
    obj = np.c_[rng.uniform(-0.2, 0.2, (40, 2)), np.zeros(40)]
    p = np.array([0.3, -0.2, 0.1, 0.02, -0.03, 0.6])
    Q = np.c_[rng.uniform(-0.5, 0.5, (40, 2)), rng.uniform(0.4, 2.0, 40)]
    img = rng.uniform(0, 300, (40, 2))
    for name, dist in (("none", None), ("4", tp.DIST5[:4]), ("5", tp.DIST5), ("8", tp.DIST8)):
        k8 = pnp._dist(dist)
        for jac in (False, True):
            add(f"text/pnp._project/{name}/{jac}", lambda k8=k8, jac=jac: pnp._project(obj, img, p, tp.K, k8, jac))
            add(f"text/stereo._project_q/{name}/{jac}", lambda k8=k8, jac=jac: stereo._project_q(Q, img, tp.K, k8, jac))
        add(f"text/pnp._project/{name}/behind", lambda k8=k8: pnp._project(obj, img, p * np.array([1, 1, 1, 1, 1, -1.0]), tp.K, k8, True))
        theta = np.r_[300.0, 302.0, 160.0, 120.0, k8[:5]]
        for jac in (False, True):
            add(f"text/calib._project_full/{name}/{jac}", lambda theta=theta, jac=jac: calib._project_full(obj, img, theta, p, jac))
        add(f"text/calib._project_full/{name}/behind", lambda theta=theta: calib._project_full(obj, img, theta, -p, True))
    on_axis = np.r_[obj[:36], [[0.0, 0.0, 0.0], [1e-13, 0.0, 0.0], [0.0, 0.6e-4, 0.0], [0.7e-4, 0.0, 0.0]]]
    p_axis = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
    for cam, (K, k) in zip(tf.CAM_IDS, tf.CAMS):
        for jac in (False, True):
            for intr in (False, True):
                add(f"text/fisheye._project/{cam}/{jac}/{intr}", lambda K=K, k=k, jac=jac, intr=intr: (fe._project(obj, img, p, K, k, jac, intr),
                                                                                                         fe._project(on_axis, img, p_axis, K, k, jac, intr)))
            add(f"text/fisheye._project_q/{cam}/{jac}", lambda K=K, k=k, jac=jac: (fe._project_q(Q, img, K, k, jac), fe._project_q(on_axis + [0, 0, 1.0], img, K, k, jac)))
            add(f"text/fisheye._project_full/{cam}/{jac}", lambda K=K, k=k, jac=jac: fe._project_full(obj, img, np.r_[K[0, 0], K[1, 1], K[0, 2], K[1, 2], k], p, jac))
        add(f"text/fisheye._project/{cam}/behind", lambda K=K, k=k: fe._project(obj, img, -p, K, k, True, True))
        add(f"text/fisheye.project_points_host/{cam}", lambda K=K, k=k: (fe.project_points_host(obj, p[:3], p[3:], K, k, jacobian=True),
                                                                          fe.project_points_host(np.r_[obj, [[0, 0, -9.0]]], p[:3], p[3:], K, k)))

def oracle_scenes():
    """The exact modules of tests/ themselves, which scenes() never calls: their scene builders on small scenes (three timestamps,
    8 rows), and residuals, cost, jacobian_fd and stationarity of every module at the scene's truth and at one perturbed point,
    long-double arrays by their bytes.  Only names and signatures that both trees have."""
    import camera_exact as cx, fisheye_rig_exact as frx, rig_exact as rx, rigpose_exact as px, stereo_exact as sx
    import test_fisheye_rig_host as tfr, test_rig_host as tr
    out = []
    add = lambda name, call: out.append((name, call))
    rng = np.random.default_rng(99)
    off = lambda v: v + 1e-3 * rng.uniform(-1, 1, np.shape(v)) * np.r_[1, 1, 1, [np.linalg.norm(np.reshape(v, (-1, 6))[0, 3:])] * 3]

    def costs(key, mod, views, s, X, P):
        for at, x, p in (("truth", X, P), ("off", off(X), off(P))):
            for f in ("residuals", "cost", "jacobian_fd", "stationarity"):
                add(f"{key}/{f}/{at}", lambda f=f, x=x, p=p: getattr(mod, f)(views, s, x, p))

    stereo = {"small": sx.scene(1, 3, "small", rows=8), "toe90": sx.scene(2, 3, "toe90", sx.BOARD_S, "B", "C", rows=8, disjoint=True),
              "r170": sx.scene(3, 3, "r170", sx.BOARD_L, "C", "A4", sigma=0.3, rows=[(8, 6), (7, 8), (8, 8)])}
    for name, s in stereo.items():
        masks = ([np.arange(len(k)) % 3 > 0 for k in s.kps0], None)
        views = sx.pool_views(s)
        add(f"stereo/{name}/scene", lambda s=s: s)
        add(f"stereo/{name}/pool_views", lambda s=s, masks=masks: (sx.pool_views(s), sx.pool_views(s, [2, 0], masks)))
        costs(f"stereo/{name}", sx, views, s, s.X, s.P)
        (o, i), (K, d) = views[1][:2], sx.cam_args(s)[:2]
        for at, p in (("truth", s.P[1]), ("off", off(s.P[1]))):
            for f in ("residuals", "cost", "jacobian_fd", "stationarity"):
                add(f"camera/{name}/{f}/{at}", lambda f=f, a=(o, i, p, K, d): getattr(cx, f)(*a))
    rigs = {"fan3": (rx, rx.scene(1, 3, rows=8, **tr.FAN3)),
            "chain4": (rx, rx.scene(2, 3, rows=8, visible=rx.chain_visibility(4, 1), **tr.CHAIN4)),
            "fan3/rows": (rx, rx.scene(3, 3, sigma=0.3, rows=[[8, 6, 7], [7, 8, 6], [6, 7, 8]], **tr.FAN3)),
            "models/rig=": (frx, frx.scene(4, 3, rows=8, rig=frx.make_rig((0, 20, -20), sx.BOARD_S, tfr.FAN3["cams"]), **tfr.FAN3))}
    for name, kw in tfr.CLASSES.items():
        rigs[f"models/{name}"] = (frx, tfr.class_scene(name, 1, n_stamps=3, rows=8, **({"visible": rx.chain_visibility(4, 1)} if "visible" in kw else {})))
    for name, (mod, s) in rigs.items():
        used = list(range(3))
        views = rx.pool_views(s, used)
        masks = [None] + [[np.arange(len(k)) % 3 > 0 for k in kl] for kl in s.kps[1:]]
        add(f"rig/{name}/scene", lambda s=s: s)
        add(f"rig/{name}/pool_views", lambda s=s, masks=masks: (rx.pool_views(s, [0, 1, 2]), rx.pool_views(s, [2, 0], masks)))
        costs(f"rig/{name}", mod, views, s, s.X, s.P)
        v1 = px.views_of(s, 1)
        add(f"rigpose/{name}/views_of", lambda s=s, masks=masks: (px.views_of(s, 1), px.views_of(s, 2, masks, keep=(0, 1))))
        for at, p in (("truth", s.P[1]), ("off", off(s.P[1]))):
            for f in ("residuals", "cost", "jacobian_fd", "stationarity"):
                add(f"rigpose/{name}/{f}/{at}", lambda f=f, a=(v1, s, s.X, p): getattr(px, f)(*a))
    s = rigs["models/fan3 F/P/F"][1]
    moved = frx.with_pose(s, 1, off(s.P[1]))
    add("rig/with_pose", lambda: moved)
    add("rig/on_axis", lambda: frx.on_axis(s, 2, 1, 3))
    add("rig/theta_max", lambda: [frx.theta_max(s, t, c) for t in range(3) for c in range(3)])
    return out

def host_worker(path):
    doc = {}
    for block, build in (("host", scenes), ("oracles", oracle_scenes)):
        got, names = {}, []
        for name, call in build():
            try:
                r = call()
            except Exception as e:                       # what a scene raises is part of what it returns
                r = ("raised", type(e).__name__, str(e))
            flat(name, r, got)
            names.append(name)
        doc[block] = {"scenes": names, "fields": got}
    json.dump(doc, open(path, "w"))

SUITE = ["tests/test_stereo_host.py", "tests/test_rig_host.py", "tests/test_fisheye_rig_host.py", "tests/test_rigpose_host.py",
         "tests/test_fisheye_ransac_host.py", "tests/test_rectify_host.py"]

def suite_seconds(trees, runs=3):
    """Wall seconds of the host tests that live on these oracles, ``runs`` of each tree, alternating -> block"""
    got = {n: [] for n in trees}
    for _ in range(runs):
        for name, tree in trees.items():
            t0 = time.perf_counter()
            r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", *SUITE], cwd=tree, capture_output=True, text=True)
            got[name].append(round(time.perf_counter() - t0, 2))
            print(name, got[name][-1], r.stdout.strip().splitlines()[-1], flush=True)
            assert r.returncode == 0, r.stdout[-2000:]
    p, t = got["parent"], got["this"]
    return {"parent_s": p, "this_s": t, "parent_spread_s": round(max(p) - min(p), 2),
            "inside": float(np.median(t)) <= float(np.median(p)) + (max(p) - min(p))}

def timed(call):
    import torch
    call(); ts = []
    for _ in range(REPS):
        torch.cuda.synchronize(); t0 = time.perf_counter(); call(); torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))

def time_worker(path):
    import torch
    from deepcharuco_amd import calib, corner_pool, fisheye as fe, pnp, rectify, rig, stereo
    rigs, frames, board, size, K, dist = pickle.load(open(path, "rb"))
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
    # the per-batch wrappers of a live stream, both models, with everything preallocated: the Python around the launch is what differs
    new = lambda dt, *shape: torch.empty(shape, dtype=dt, device=dev)
    pose_out = (new(torch.int32, b), new(torch.float64, b, 8))
    ransac_out = pose_out + (new(torch.int32, b, 2), torch.zeros(pool, dtype=torch.uint8, device=dev))
    ws = new(torch.uint8, pnp.ransac_workspace_bytes(b, pool, 100))
    xy, map_ = new(torch.float64, pool, 2), new(torch.int32, size[1], size[0], 2)
    for name, mod, pre, post in (("", pnp, "", ""), ("_fisheye", fe, "fisheye_", "_fisheye")):
        got[f"solve_pnp{name}_pool"] = timed(lambda: getattr(mod, f"solve_pnp_{pre}pool")(packed, b, pool, True, *board, K, dist, out=pose_out))
        got[f"solve_pnp{name}_ransac_pool"] = timed(lambda: getattr(mod, f"solve_pnp_{pre}ransac_pool")(packed, b, pool, True, *board, K, dist, out=ransac_out, workspace=ws))
        got[f"rectify_points{name}_pool"] = timed(lambda: getattr(fe if name else rectify, f"rectify_points{post}_pool")(packed, b, pool, True, K, dist, out=xy))
        got[f"undistort_rectify_map{name}_device"] = timed(lambda: getattr(fe if name else rectify, f"undistort_rectify_map{post}_device")(K, dist, None, None, size[0], size[1], out=map_))
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
    ap.add_argument("--suite", action="store_true", help="also time the host tests of the multi-camera oracles in both trees, three runs each")
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
        docs, blocks, moved = {}, {}, []
        for name, tree in trees.items():
            child(tree, "--host-worker", os.path.join(tmp, name + ".json"))
            docs[name] = json.load(open(os.path.join(tmp, name + ".json")))
        for key in ("host", "oracles"):
            got, names = {n: d[key]["fields"] for n, d in docs.items()}, {n: d[key]["scenes"] for n, d in docs.items()}
            assert names["parent"] == names["this"]
            keys = sorted(set(got["parent"]) | set(got["this"]))
            differ = [k for k in keys if got["parent"].get(k) != got["this"].get(k)]
            blocks[key] = {"scenes": len(names["this"]), "fields": len(keys),
                           "fields_moved": differ, "raised": sorted(k[:-2] for k in keys if k.endswith("/0") and got["this"].get(k) == "str 'raised'"),
                           "numpy": np.__version__}
            for k in differ:
                print("MOVED", k, got["parent"].get(k), got["this"].get(k))
            moved += differ
        if a.suite:
            blocks["oracles"]["host_tests"] = suite_seconds(trees)
            moved += [] if blocks["oracles"]["host_tests"]["inside"] else ["host_tests"]
        print(json.dumps(blocks, indent=1))
    else:
        sys.path[:0] = [REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tools")]
        import fisheye_probe as fp, rig_old_new as ron
        rigs = {k: v[:4] for k, v in ron.rig_scenes(None).items()}
        path = os.path.join(tmp, "scenes.pkl")
        pickle.dump((rigs, ron.calib_scenes(), fp.BOARD, fp.SIZE, fp.K, fp.DIST), open(path, "wb"))
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
        doc.update({"time": block} if a.time else blocks)
        json.dump(doc, open(a.out, "w"), indent=1)
    sys.exit(1 if moved else 0)

if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] in ("--host-worker", "--time-worker"):
        (host_worker if sys.argv[1] == "--host-worker" else time_worker)(sys.argv[2])
    else:
        main()
