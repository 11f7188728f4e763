"""CPU: host-side logic of the product package and the C-ABI surface (no compute calls)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, REPO
from deepcharuco_amd import weights as W


def test_library_loads_and_exports_every_declared_symbol():
    from deepcharuco_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(REPO, "include", "deepcharuco_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(dcx_[a-z0-9_]+)\s*\(", header))
    assert len(declared) >= 25
    for name in sorted(declared):
        assert hasattr(handle, name), f"{name} declared in the header but not exported"
    assert declared == set(_lib.SIGNATURES), "ctypes signature table and header disagree"
    lib = _lib.lib()
    assert b"gfx950" in lib.dcx_version()
    assert b"DCX_E_SHAPE" in lib.dcx_error_string(-2)


def test_null_arguments_are_rejected_without_a_gpu():
    from deepcharuco_amd import _lib
    lib = _lib.lib()
    assert lib.dcx_pre_image(None, None, 10, None) == -1
    assert lib.dcx_argmax2d(None, 1, 2, 2, None, None) == -1
    assert lib.dcx_detector_workspace_bytes(None, 1, 240, 320) == 0
    h = ctypes.c_void_p()
    assert lib.dcx_detector_create(ctypes.byref(h), None, 64, 16) == -1


def test_cpu_device_is_refused_loudly():
    from deepcharuco_amd.models.net import dcModel
    from deepcharuco_amd.inference import infer_image
    with pytest.raises(RuntimeError, match="no CPU fallback|no CPU path|MI355X"):
        dcModel(16).load_state_dict(W.synthetic_state_dict("detector", 0), device="cpu")
    with pytest.raises(RuntimeError):
        infer_image(np.zeros((16, 16, 3), np.uint8), 16, None, None, device="cpu")


def test_product_package_never_imports_the_oracle():
    pkg = os.path.join(REPO, "deepcharuco_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(root, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", src, flags=re.M), f"{f} imports the oracle"
                assert "F.conv2d" not in src and "torch.nn.functional" not in src, f"{f} uses stock torch ops"


def test_state_dict_layout_and_checkpoint_roundtrip(tmp_path):
    sd = W.synthetic_state_dict("detector", 11, 16)
    assert len(W.state_dict_keys("detector", 16)) == 64 and len(W.state_dict_keys("refinenet")) == 68
    n_params = sum(v.size for k, v in sd.items() if "running" not in k)
    assert n_params == 1_242_002   # detector parameter count
    rn = W.synthetic_state_dict("refinenet", 11)
    assert sum(v.size for k, v in rn.items() if "running" not in k) == 999_233
    p = str(tmp_path / "dc.ckpt")
    W.save_lightning_style_checkpoint(p, sd)
    back = W.state_dict_from_checkpoint(p, "detector", 16)
    assert list(back) == W.state_dict_keys("detector", 16)
    assert all(np.array_equal(back[k], sd[k]) for k in sd)
    with pytest.raises(KeyError):
        W.state_dict_from_checkpoint(p, "refinenet")
    assert W.state_dict_sha256(sd, "detector") == W.state_dict_sha256(W.synthetic_state_dict("detector", 11), "detector")
    assert W.state_dict_sha256(sd, "detector") != W.state_dict_sha256(W.synthetic_state_dict("detector", 12), "detector")


@pytest.mark.parametrize("pl_version", ["1.9.3", "2.1.0"])
def test_checkpoint_reader_on_a_full_lightning_checkpoint(tmp_path, pl_version):
    """VERDICT r2 missing #3: a Trainer.fit checkpoint also carries loops / callbacks (keyed by ModelCheckpoint{...} strings,
    holding paths and score tensors) / optimizer_states (Adam moments with the SAME shapes as the weights) / lr_schedulers /
    pytorch-lightning_version (/ hyper_parameters).  The reader must go through such a file on the weights_only=True path
    and return exactly the model tensors."""
    import torch
    for kind, n_ids in (("detector", 16), ("refinenet", 16)):
        sd = W.synthetic_state_dict(kind, 21, n_ids)
        p = str(tmp_path / f"{kind}.ckpt")
        W.save_lightning_style_checkpoint(p, sd, full=True, pl_version=pl_version)
        blob = torch.load(p, map_location="cpu", weights_only=True)                 # the file itself is weights_only-clean
        assert {"epoch", "global_step", "pytorch-lightning_version", "state_dict", "loops", "callbacks", "optimizer_states",
                "lr_schedulers"} <= set(blob)
        assert ("hyper_parameters" in blob) == (not pl_version.startswith("1."))
        assert any(k.startswith("ModelCheckpoint{") for k in blob["callbacks"])
        assert len(blob["optimizer_states"][0]["state"]) == sum(k.endswith((".weight", ".bias")) for k in sd)
        back = W.state_dict_from_checkpoint(p, kind, n_ids)                          # allow_unsafe stays False
        assert list(back) == W.state_dict_keys(kind, n_ids)
        assert W.state_dict_sha256(back, kind, n_ids) == W.state_dict_sha256(sd, kind, n_ids)
        assert all(v.dtype == np.float32 for v in back.values())


def test_synthetic_frames_are_per_frame_deterministic():
    a = W.synthetic_frames("board", 5, 3, 64, 96)
    b = W.synthetic_frames("board", 6, 2, 64, 96)
    assert a.dtype == np.uint8 and a.shape == (3, 64, 96)
    assert np.array_equal(a[1], b[0]) and np.array_equal(a[2], b[1])
    assert a.std() > 20


def test_unpack_results_sorting_and_dtypes():
    """The packed corner pool: counts[B] | starts[B] | rows[pool][4] | xy[pool][2] (| conf[pool][2]); frames sit in the pool in any
    order (starts[]), a frame may own any share of it, a frame that does not fit completely comes back as None."""
    from deepcharuco_amd.corner_pool import views
    from deepcharuco_amd.inference import packed_len, unpack_results
    b, pool = 4, 8
    assert packed_len(b, pool) == 56 and packed_len(b, pool, True) == 72
    packed = np.zeros(packed_len(b, pool, True), np.int32)
    counts_v, starts_v, rows, xy, cf = views(packed, b, pool)
    counts_v[:] = [3, 0, 4, 5]                # 12 corners > pool: the frame that was placed last does not fit
    starts_v[:] = [4, 7, 0, 7]                # frame 2 came first, then frame 0, then frame 3 (slots 7..11: only one exists)
    rows[4:7] = [[8, 9, 5, 1], [16, 17, 2, 2], [24, 25, 5, 3]]
    rows[0:4] = [[1, 1, 0, 0], [2, 2, 0, 1], [3, 3, 0, 2], [4, 4, 0, 3]]
    xy[4:7] = [[8.5, 9.25], [16.125, 17], [24, 25.5]]
    cf[4:7] = [[0.5, 0.25], [0.75, 0.125], [1.0, 0.0625]]
    res, counts, confs = unpack_results(packed, b, pool, True, conf=True)
    assert res[0].dtype == np.float64
    assert np.array_equal(res[0], [[16.125, 17, 2], [8.5, 9.25, 5], [24, 25.5, 5]])   # stable by id
    assert np.array_equal(confs[0], [[0.75, 0.125], [0.5, 0.25], [1.0, 0.0625]]) and confs[0].dtype == np.float32
    assert res[1].shape == (0,) and res[1].dtype == np.float64 and confs[1].shape == (0, 2)
    assert res[2].shape == (4, 3) and counts.tolist() == [3, 0, 4, 5]
    assert res[3] is None and confs[3] is None and int(counts.sum()) > pool            # the caller re-runs with pool >= 12
    res, _ = unpack_results(packed[:packed_len(b, pool)], b, pool, False)
    assert res[0].dtype == np.int64 and np.array_equal(res[0], [[16, 17, 2], [8, 9, 5], [24, 25, 5]])


def test_bench_dump_outputs_layout(tmp_path, monkeypatch):
    """bench.py --dump-outputs: the last timed step's per-frame corner rows as float64 .npy files (rows concatenated in frame
    order + the count of every frame, NaN for a frame that overflowed the pool); over the size limit, a fixed seeded sample."""
    import bench
    res = [np.array([[1.5, 2.25, 3.0], [4.0, 5.0, 7.0]]), np.array([]), None, np.array([[8.0, 9.5, 0.0]])]
    bench.dump_outputs(str(tmp_path / "a"), res)
    assert sorted(os.listdir(tmp_path / "a")) == ["corners.npy", "corners_per_frame.npy"]
    corners, counts = np.load(tmp_path / "a" / "corners.npy"), np.load(tmp_path / "a" / "corners_per_frame.npy")
    assert corners.dtype == np.float64 and np.array_equal(corners, [[1.5, 2.25, 3], [4, 5, 7], [8, 9.5, 0]])
    assert counts.dtype == np.float64 and np.array_equal(counts, [2, 0, np.nan, 1], equal_nan=True)
    big = [np.arange(3000, dtype=np.float64).reshape(1000, 3) + 3000 * i for i in range(4)]
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 24 * 100 + 4 * 8)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), big)
    s = np.load(tmp_path / "b" / "corners.npy")
    assert s.shape == (100, 3) and np.array_equal(s, np.load(tmp_path / "c" / "corners.npy"))       # fixed seed: same rows
    assert np.all(np.diff(s[:, 0]) > 0) and np.all(s[:, 0] % 3 == 0)                                 # whole rows, in order
    assert np.array_equal(np.load(tmp_path / "b" / "corners_per_frame.npy"), [1000] * 4)


def test_bgr2gray_host():
    from deepcharuco_amd.imgproc import bgr2gray
    d = np.load(os.path.join(REPO, "tests", "golden", "bgr2gray_formula.npz"))
    from deepcharuco_amd import imgproc
    from oracle import deepcharuco_oracle as O
    assert imgproc.BGR2GRAY_VARIANTS == O.BGR2GRAY_VARIANTS and imgproc.DEFAULT_BGR2GRAY == "opencv4"
    for v, key, keyd in (("opencv4", "gray", "gray_differ"), ("legacy14", "gray_legacy14", "gray_differ_legacy14")):
        assert np.array_equal(imgproc.bgr2gray_fixed_point(d["bgr"], v), d[key])
        assert np.array_equal(imgproc.bgr2gray_fixed_point(d["bgr_differ"], v), d[keyd])
    if imgproc._opencv():      # with OpenCV installed bgr2gray IS cv2.cvtColor: it must agree with the variant of that version
        v = imgproc.bgr2gray_variant_of_module(imgproc._opencv())          # asks the module itself, not its version string
        assert np.array_equal(bgr2gray(d["bgr_differ"]), imgproc.bgr2gray_fixed_point(d["bgr_differ"], v))
    else:
        assert np.array_equal(bgr2gray(d["bgr"]), d["gray"]) and np.array_equal(bgr2gray(d["bgr_differ"]), d["gray_differ"])
    assert [imgproc.bgr2gray_variant_of_opencv(x) for x in ("4.6.0", "4.11.0.86", "3.4.2", "2.4.13", "weird")] == \
        ["opencv4", "opencv4", "legacy14", "legacy14", "opencv4"]

    class FakeCv2:           # the probe recognises either generation by what it COMPUTES on 16 pixels where the variants differ
        COLOR_BGR2GRAY = 6

        def __init__(self, variant):
            self.variant = variant

        def cvtColor(self, img, code):
            return imgproc.bgr2gray_fixed_point(img, self.variant)
    assert imgproc._probe_pixels().shape == (1, 16, 3)
    assert [imgproc.bgr2gray_variant_of_module(FakeCv2(v)) for v in ("opencv4", "legacy14")] == ["opencv4", "legacy14"]


def test_checkpoint_reader_never_unpickles_code_silently(tmp_path):
    """weights_only=True is the default; a checkpoint that needs a full unpickle is refused unless the caller
    opts in; a missing / truncated file raises its own error and is not retried unsafely."""
    import pickle
    import torch
    sd = W.synthetic_state_dict("refinenet", 3)
    good = str(tmp_path / "good.ckpt")
    W.save_lightning_style_checkpoint(good, sd)
    assert W.state_dict_sha256(W.state_dict_from_checkpoint(good, "refinenet"), "refinenet") == W.state_dict_sha256(sd, "refinenet")

    class Evil:
        def __reduce__(self):
            return (os.system, ("echo pwned > " + str(tmp_path / "pwned"),))
    bad = str(tmp_path / "bad.ckpt")
    torch.save({"state_dict": {f"model.{k}": torch.from_numpy(v) for k, v in sd.items()}, "hyper_parameters": Evil()}, bad)
    with pytest.raises(RuntimeError, match="unsafe"):
        W.state_dict_from_checkpoint(bad, "refinenet")
    assert not os.path.exists(tmp_path / "pwned")
    with pytest.raises(FileNotFoundError):
        W.state_dict_from_checkpoint(str(tmp_path / "missing.ckpt"), "refinenet")
    trunc = str(tmp_path / "trunc.ckpt")
    open(trunc, "wb").write(open(good, "rb").read()[:1000])
    with pytest.raises(Exception) as ei:
        W.state_dict_from_checkpoint(trunc, "refinenet")
    assert not isinstance(ei.value, pickle.UnpicklingError) or "unsafe" not in str(ei.value)
    out = W.state_dict_from_checkpoint(bad, "refinenet", allow_unsafe=True)      # explicit opt-in works (and runs the payload)
    assert os.path.exists(tmp_path / "pwned") and "conv1a.weight" in out


def test_solve_pnp_short_circuit():
    from deepcharuco_amd.inference import solve_pnp
    assert solve_pnp(np.zeros((3, 3)), 5, 5, 0.01, None, None) == (False, None, None)


def test_solve_pnp_batch_on_host_threads_with_a_recording_backend(monkeypatch):
    """cv2 is absent in this image, so the PnP stage is tested with a recording stand-in for cv2.solvePnP (a fake
    backend, test-only): per-frame object/image points must equal the fixture written from the reference's own
    construction (inference.py:15-26), frames with < 4 corners short-circuit, order is preserved, several threads run."""
    import sys
    import threading
    import time
    import types
    from deepcharuco_amd import inference as I
    d = np.load(os.path.join(GOLDEN, "solve_pnp_points.npz"))
    calls, lock = [], threading.Lock()

    def solvePnP(obj, img, cam, dist):
        time.sleep(0.01)
        with lock:
            calls.append((threading.get_ident(), obj.copy(), img.copy()))
        return True, obj.sum(0, keepdims=True).T.astype(np.float64), img.sum(0, keepdims=True).T.astype(np.float64)
    monkeypatch.setitem(sys.modules, "cv2", types.SimpleNamespace(solvePnP=solvePnP))
    kp = d["kp"]
    frames = [kp, np.array([]), kp[:3], kp[::-1].copy()] + [kp] * 12
    cam, dist = np.eye(3), np.zeros(5)
    out = I.solve_pnp_batch(frames, 5, 5, 0.01, cam, dist, workers=4)
    assert len(out) == 16
    assert out[1] == (False, None, None) and out[2] == (False, None, None)            # inference.py:16-17
    single = I.solve_pnp(kp, 5, 5, 0.01, cam, dist)
    assert out[0][0] is True and np.array_equal(out[0][1], single[1]) and np.array_equal(out[0][2], single[2])
    assert np.array_equal(out[3][2], d["imgp"][::-1].sum(0, keepdims=True).T.astype(np.float64))
    first = [c for c in calls if np.array_equal(c[2], d["imgp"])][0]
    assert np.array_equal(first[1], d["objp"]) and first[1].dtype == np.float32 and first[2].dtype == np.float32
    assert len({c[0] for c in calls}) > 1                                               # really ran on several threads
    futs = I.solve_pnp_submit(frames[:2], 5, 5, 0.01, cam, dist)
    assert [f.result()[0] for f in futs] == [True, False]


def test_solve_pnp_hands_opencv_what_the_reference_does(monkeypatch):
    """Product solve_pnp vs the arguments the REFERENCE's solve_pnp (inference.py:15-29) passed to a recording
    cv2.solvePnP in oracle/make_golden.py: same object / image points (values and dtypes), camera matrix and distortion
    passed through untouched, return value handed back as is."""
    import sys
    import types
    from deepcharuco_amd import inference as I
    d = np.load(os.path.join(GOLDEN, "solve_pnp_points.npz"))
    seen = []

    def solvePnP(obj, img, cam, dist):
        seen.append((obj, img, cam, dist))
        return "ret", "rvec", "tvec"
    monkeypatch.setitem(sys.modules, "cv2", types.SimpleNamespace(solvePnP=solvePnP))
    cam, dist = d["cam"], d["dist"]
    for i in range(int(d["n_cases"])):
        cols, rows, sq = d[f"board{i}"]
        del seen[:]
        assert I.solve_pnp(d[f"kp{i}"], int(cols), int(rows), float(sq), cam, dist) == ("ret", "rvec", "tvec")
        (obj, img, c, k), = seen
        assert c is cam and k is dist
        assert obj.dtype == np.float32 and img.dtype == np.float32
        assert np.array_equal(obj, d[f"objp{i}"]) and np.array_equal(img, d[f"imgp{i}"]), i
        (f,) = I.solve_pnp_submit([d[f"kp{i}"]], int(cols), int(rows), float(sq), cam, dist)
        assert f.result() == ("ret", "rvec", "tvec") and np.array_equal(seen[-1][0], d[f"objp{i}"])


def test_solve_pnp_without_opencv_raises_clearly(monkeypatch):
    import sys
    from deepcharuco_amd import inference as I
    monkeypatch.setitem(sys.modules, "cv2", None)               # import cv2 -> ImportError
    kp = np.load(os.path.join(GOLDEN, "solve_pnp_points.npz"))["kp"]
    with pytest.raises(ImportError, match="OpenCV"):
        I.solve_pnp(kp, 5, 5, 0.01, np.eye(3), np.zeros(5))
    with pytest.raises(ImportError, match="OpenCV"):
        I.solve_pnp_batch([kp], 5, 5, 0.01, np.eye(3), np.zeros(5))


def test_bgr2gray_formula_against_opencv_when_available():
    """cv2.cvtColor is third-party and absent here ("parity unpinned" for that one step): wherever OpenCV IS importable
    this test pins the fixed-point restatement against it on a random colour image."""
    cv2 = pytest.importorskip("cv2")
    from oracle import deepcharuco_oracle as O
    from deepcharuco_amd.imgproc import bgr2gray_variant_of_module
    variant = bgr2gray_variant_of_module(cv2)       # what THIS OpenCV computes (4.6 ... 4.11, what the reference pins: 15-bit constants)
    rng = np.random.default_rng(5)
    bgr = rng.integers(0, 256, (97, 131, 3), dtype=np.uint8)
    assert np.array_equal(cv2.cvtColor(bgr, cv2.COLOR_BGR2GRAY), O.bgr2gray(bgr, variant))
    d = np.load(os.path.join(GOLDEN, "bgr2gray_formula.npz"))   # pixels on which the two variants disagree
    assert np.array_equal(cv2.cvtColor(d["bgr_differ"], cv2.COLOR_BGR2GRAY), O.bgr2gray(d["bgr_differ"], variant))


def test_shard_range_partition():
    from deepcharuco_amd.sharding import shard_range
    for n in (0, 1, 7, 32, 1024):
        for world in (1, 2, 3, 8):
            spans = [shard_range(n, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(spans[i][1] == spans[i + 1][0] for i in range(world - 1))
            sizes = [hi - lo for lo, hi in spans]
            assert max(sizes) - min(sizes) <= 1


def test_kernel_family_depends_on_the_layer_only():
    """the kernel FAMILY (= the fp32 summation order, i.e. the bits) of every layer of both networks is a
    function of the layer alone -- the same for 1 frame and 1,024, for 1 patch and 16,384 -- while the TILE may follow the
    launch size (all tiles of a family give identical bits: test_every_conv_instantiation_bit_exact)."""
    from deepcharuco_amd import _lib
    L = _lib.lib()
    # (dcx_conv_wino2hs.h is the wino2h FAMILY -- the same summation orders -- in the shape for launches that cannot fill the chip)
    fam = lambda nm: nm[nm.index("dcx_conv_") + 9:nm.index("_kernel")].replace("wino2hs", "wino2h").replace("wino2ps", "wino2p")
    det = [(64, 64, 1, 1), (64, 64, 2, 0), (64, 64, 2, 1), (64, 128, 4, 0), (128, 128, 4, 1), (128, 128, 8, 0), (128, 512, 8, 0)]
    ref = [(64, 64, 20, 0, 0, 0), (64, 128, 18, 0, 0, 0), (128, 128, 16, 1, 0, 0), (128, 128, 8, 0, 0, 0), (128, 128, 16, 0, 0, 1),
           (128, 128, 16, 0, 0, 0), (128, 64, 32, 0, 0, 1), (64, 64, 32, 0, 0, 0), (64, 64, 64, 0, 2, 1)]
    for h, w in ((240, 320), (480, 640), (960, 1280), (64, 96)):
        for cin, cout, div, pool in det:
            fams = {fam(L.dcx_conv_pick_name(n, cin, h // div, w // div, cout, 3, pool, 0).decode()) for n in (1, 2, 7, 32, 128, 1024)}
            assert fams == {"wino2h"}, (h, w, cin, cout, fams)
    for cin, cout, ho, pool, epi, ups in ref:
        fams = {fam(L.dcx_conv_pick_name_ups(n, cin, ho, ho, cout, 3, pool, epi, ups).decode()) for n in (1, 3, 16, 112, 512, 16384)}
        assert fams == ({"wino2p"} if ups else {"wino2h"}), (cin, cout, ho, fams)
    for n in (1, 32, 1024):
        assert "dcx_conv_mfma_kernel" in L.dcx_conv_pick_name(n, 256, 1, 1200, 65, 1, 0, 1).decode()      # 1x1 heads: direct, always


def test_tile_cost_model_choices():
    """The tile inside the family is a cost-model choice (csrc/dcx_conv_mfma.hip: pick); these are the ones the design relies
    on: 8x16 tiles for the big maps, 6x20 where they fit without padding (30x40 heads, RefineNet's 18/20-pixel maps), two whole
    8x8 maps per item after RefineNet's pool, phases x F(2x2,2x2) behind the up-samplings, the direct family for 1x1 layers
    and in deterministic mode."""
    from deepcharuco_amd import _lib
    L = _lib.lib()
    name = lambda *a: L.dcx_conv_pick_name(*a).decode()
    name_ups = lambda *a: L.dcx_conv_pick_name_ups(*a).decode()
    assert name(32, 64, 240, 320, 64, 3, 1, 0) == "dcx_conv_wino2h_kernel<DcxWino2hCfg<8,16,1,1>>"     # conv1b, bs=32
    assert name(128, 64, 480, 640, 64, 3, 1, 0) == "dcx_conv_wino2h_kernel<DcxWino2hCfg<8,16,1,1>>"    # conv1b, cfg3
    assert "DcxWino2hCfg<8,16,0,1>" in name(32, 64, 120, 160, 64, 3, 0, 0)                 # conv2a
    assert "DcxWino2hCfg<6,20,0,1>" in name(512, 64, 18, 18, 128, 3, 0, 0)                 # RefineNet conv2a: 18x18 map in 3 tiles of 6x20
    assert "DcxWino2hCfg<6,20,0,1>" in name(32, 128, 30, 40, 512, 3, 0, 0)                 # fused heads' 3x3 (512 couts): 30x40 = 5 x 2 tiles
    assert "DcxWino2hCfg<8,8,0,2>" in name(512, 128, 8, 8, 128, 3, 0, 0)                   # RefineNet conv3a/3b: two maps per item
    assert "DcxWino2hsCfg<0,1>" in name(16, 128, 8, 8, 128, 3, 0, 0)                       # ... at bs=1 (16 patches): positions split over waves, 16 couts per workgroup: 128 short chains (same bits)
    assert "DcxWino2hsCfg<0,1>" in name(1, 128, 30, 40, 128, 3, 0, 0)                      # conv4a for ONE frame: 160 quarter-length items instead of 40
    assert "DcxWino2hsCfg<0,4>" in name(1, 128, 30, 40, 512, 3, 0, 0)                      # the fused heads of one frame: 160 items of 64 couts, four waves per SIMD
    assert "DcxWino2hsCfg<1,2>" in name(16, 128, 16, 16, 128, 3, 1, 0)                     # RefineNet conv2b, 16 patches: 256 items of 32 couts
    assert "DcxWino2hCfg<8,16,0,1>" in name(16, 64, 18, 18, 128, 3, 0, 0)                  # ... conv2a (288 items even at 64 couts): more than one round -> the bs=32 kernels
    assert "DcxWino2hCfg<8,8,0,1,1>" in name(32, 128, 30, 40, 128, 3, 0, 0)                # ... and where 32-tile items quantise badly (768 items on 512 slots: measured 60 vs 63.5 us)
    assert "DcxWino2hCfg<8,16,0,1>" in name(32, 64, 60, 80, 128, 3, 0, 0)                  # ... but not where the chip is well filled (conv3a: 107 vs 121 us)
    assert "DcxWino2hCfg<8,16,0,1>" in name(128, 128, 60, 80, 128, 3, 0, 0)                # (conv4a of cfg3)
    assert name_ups(512, 64, 64, 64, 64, 3, 0, 2, 1) == "dcx_conv_wino2p_kernel<DcxWino2pCfg<8,16,DCX_EPI_HEAT,1>>"    # RefineNet head behind the x2 up-sampling
    assert name_ups(512, 128, 32, 32, 64, 3, 0, 0, 1) == "dcx_conv_wino2p_kernel<DcxWino2pCfg<8,16,DCX_EPI_BNRELU,1>>"  # conv5a
    assert name_ups(512, 128, 16, 16, 128, 3, 0, 0, 1) == "dcx_conv_wino2p_kernel<DcxWino2pCfg<8,8,DCX_EPI_BNRELU,2>>"   # conv4a: two 8x8 maps per item
    assert "<1,4,2,2,1,256,1,0,DCX_EPI_RAW>" in name(32, 256, 1, 1200, 65, 1, 0, 1)
    L.dcx_set_deterministic(1)
    try:
        assert "dcx_conv_mfma_kernel" in name(32, 64, 240, 320, 64, 3, 1, 0) and "dcx_conv_mfma_kernel" in name_ups(512, 128, 32, 32, 64, 3, 0, 0, 1)
        assert "DCX_EPI_HEAT" in name_ups(512, 64, 64, 64, 64, 3, 0, 2, 1) and "dcx_conv_mfma_kernel" in name_ups(512, 64, 64, 64, 64, 3, 0, 2, 1)
    finally:
        L.dcx_set_deterministic(0)
    assert name(32, 64, 30, 40, 64, 3, 0, 1) == ""                              # no raw 3x3 instantiation


def test_c_restatement_agrees_with_torch_fp32():
    """oracle/conv_exact.c (the bit-exact checker of the MFMA kernel) is itself checked against torch's fp32 conv
    on CPU: same maths, different summation order -> equal within fp32 re-ordering noise."""
    import torch
    import torch.nn.functional as F
    from oracle.conv_exact import conv_exact
    g = torch.Generator().manual_seed(5)
    for cin, cout, h, w, pad, ups, pool, ks, has_bn in [(64, 64, 12, 20, 1, False, True, 3, True),
                                                         (32, 48, 9, 7, 0, False, False, 3, True),
                                                         (64, 32, 5, 6, 1, True, False, 3, True),
                                                         (64, 17, 4, 5, 0, False, False, 1, False),
                                                         (1, 64, 10, 12, 1, False, False, 3, True)]:
        x = torch.randn(2, cin, h, w, generator=g)
        wt = torch.randn(cout, cin, ks, ks, generator=g) * (2.0 / (cin * ks * ks)) ** 0.5
        b = torch.randn(cout, generator=g) * 0.1
        bn = None
        if has_bn:
            bn = (torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1,
                  torch.randn(cout, generator=g) * 0.1, torch.rand(cout, generator=g) + 0.5)
        xr = F.interpolate(x, scale_factor=2, mode="nearest") if ups else x
        ref = F.conv2d(xr, wt, b, padding=pad)
        if bn is not None:
            ref = F.relu(F.batch_norm(ref, bn[2], bn[3], bn[0], bn[1], False, 0.0, 1e-5))
        if pool:
            ref = F.max_pool2d(ref, 2, 2)
        # the direct order, and for 3x3 + BN layers with cin % 16 == 0 also the 2-D F(2x2,3x3) Winograd order / behind an
        # up-sampling the phases x F(2x2,2x2) order
        fams = ["direct"]
        if ks == 3 and has_bn and cin % 16 == 0:
            fams = ["direct", "w2p"] if ups else ["direct", "w2h"]
        for fam in fams:
            got = conv_exact(x.numpy(), wt.numpy(), b.numpy(), None if bn is None else [t.numpy() for t in bn],
                             pad=pad, ups=ups, pool=pool, family=fam)
            assert got.shape == tuple(ref.shape)
            assert np.abs(got - ref.numpy()).max() <= 2e-5, (fam, cin, cout)


def test_conv_kernels_do_not_spill(tmp_path):
    """The Winograd kernels are written around hipcc's register allocation (accumulators pinned to AGPRs with inline asm,
    one basic block per unit): a change that makes hipcc shuffle accumulators or spill shows up as a large slowdown only
    on the GPU.  This guards the budget at build time: no VGPR spills in any MFMA kernel of the dispatch table, and no
    scratch / accumulator moves inside the unit loops of the Winograd kernels."""
    import re
    import subprocess
    src = os.path.join(REPO, "deepcharuco_amd", "csrc", "dcx_conv_mfma.hip")
    out = str(tmp_path / "dcx_conv_budget.s")      # per run: a fixed name in the shared temp dir may belong to another user
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-mllvm",
                    "-pragma-unroll-threshold=200000", "-S", src, "-o", out], check=True, capture_output=True)
    asm = open(out).read()
    spills = dict(re.findall(r"\.name:\s+(_Z2\ddcx_conv_\w+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", asm))
    assert len(spills) >= 14
    bad = {k: v for k, v in spills.items() if int(v) != 0}
    assert not bad, f"kernels with VGPR spills: {bad}"
    # half-tile and phase Winograd kernels (two / three workgroups per CU): no scratch in the unit loops; hipcc may park a few
    # loop invariants in spare AGPRs at three waves per SIMD (84 + 84 registers), which costs one move each per unit
    for m in re.finditer(r"^(_Z2\ddcx_conv_wino2[hp]_kernel\w+):[^\n]*\n", asm, re.M):
        body = asm[m.end():asm.index(".Lfunc_end", m.end())]
        loops = [b for b in re.split(r"\n\.LBB[0-9_]+:", body) if b.count("v_mfma") >= 64]
        assert loops, m.group(1)
        for b in loops:
            assert "scratch_" not in b and b.count("v_accvgpr") <= 8, f"{m.group(1)}: spill inside the unit loop"


def test_graph_cache_clear_is_reentrant():
    """A cached GraphedPipeline may hold the LAST reference to a model pair; dropping it (clear_graph_cache, e.g. from
    set_deterministic) then runs RefineNet._release -> drop_graphs_of, which comes back to the cache lock on the same
    thread.  Found as a hang of the GPU suite in round 3; reproduced here without a GPU, under a watchdog."""
    import threading
    from deepcharuco_amd import graph as G

    class Pipe:
        def __init__(self, ref):
            self.ref = ref

        def close(self):             # GraphedPipeline.close(): retire (lock-free); the buffers die under the device locks
            pass

        def __del__(self):
            G.drop_graphs_of(self.ref)

    class Det:
        pass
    det, cache = Det(), G._Cache()
    det._graph_cache = cache
    G._caches.add(cache)
    cache[((1, 2), 16, 8, 8, True, 64, 0)] = Pipe(object())
    done = []
    t = threading.Thread(target=lambda: (G.clear_graph_cache(), done.append(1)), daemon=True)
    t.start()
    t.join(20)
    assert done and len(cache) == 0, "clear_graph_cache dead-locked on its own lock"
    cache[((3, 4), 16, 8, 8, True, 64, 0)] = Pipe(object())
    t = threading.Thread(target=lambda: (G.clear_graph_cache(det), done.append(2)), daemon=True)
    t.start()
    t.join(20)
    assert done == [1, 2] and len(cache) == 0


def test_graph_weights_outlive_a_replay_in_flight():
    """a model reloaded or destroyed while another thread replays a graph captured with its weights must not free
    those weights under the replay.  The graph holds them; retiring it hands them to the graveyard, which is emptied only under
    the locks of all devices.  A model with no graph still frees its weights at once."""
    import ctypes
    import gc
    import threading
    from deepcharuco_amd import graph as G
    from deepcharuco_amd.models._handles import NativeModel, NativeWeights

    destroyed = []

    def model_with_weights(h):          # no GPU: the weights are a fake handle whose destroy records it
        m = NativeModel()
        m._weights = NativeWeights(ctypes.c_void_p(h), None, lambda hd: destroyed.append(hd.value))
        return m

    class Pipe(G.GraphedPipeline):
        def __init__(self, weights):    # what close() hands on, without a GPU: no graph, buffers or stream
            self.graph = object()
            self.ws = self.dev_in = self.out_dev = self.pin_in = self.pin_out = self.stream = None
            self._det_handle, self._ref_handle = weights, None
            G._live.add(self)

    # (a) thread B releases the weights (as a reload or the destructor does) while thread A holds the device lock, as a replay does
    m = model_with_weights(1)
    pipe = Pipe(m._weights)
    in_replay, replay_done = threading.Event(), threading.Event()

    def replay():
        with G._locks.device(0):
            in_replay.set()
            replay_done.wait(20)
    a = threading.Thread(target=replay, daemon=True)
    a.start()
    assert in_replay.wait(20)
    b = threading.Thread(target=lambda: (m._release(), destroyed.append("released")), daemon=True)
    b.start()
    b.join(20)
    assert destroyed == ["released"], "the model's release waited for the replay or destroyed the weights under it"
    assert pipe.graph is None                        # retired: a later run() refuses
    del m
    gc.collect()
    assert destroyed == ["released"]
    replay_done.set()
    a.join(20)
    assert not a.is_alive()
    G.clear_graph_cache()                            # drains the graveyard under every device lock
    assert destroyed == ["released", 1]
    G.clear_graph_cache()
    del pipe
    gc.collect()
    assert destroyed == ["released", 1]              # exactly once

    # (b) no graph holds them: freed right away, by a reload as by the destructor
    m = model_with_weights(2)
    m._release()
    assert destroyed[-1] == 2 and m._weights is None
    m = model_with_weights(3)
    del m
    assert destroyed[-1] == 3
    w = NativeWeights(ctypes.c_void_p(4), None, lambda hd: destroyed.append(hd.value))
    w.free()
    w.free()
    del w
    assert destroyed == ["released", 1, 2, 3, 4]


def test_missing_native_library_fails_loudly(monkeypatch, tmp_path):
    """No fallback: without libdeepcharuco_amd.so every entry into the library raises (nothing is computed on the
    CPU or through stock PyTorch operators instead)."""
    from deepcharuco_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "libdeepcharuco_amd.so"))
    with pytest.raises(RuntimeError, match="no CPU / stock-PyTorch fallback"):
        _lib.lib()


def test_bench_gpus_n_from_a_bare_shell_refuses_rccl_without_enough_gpus():
    """`python bench.py --gpus 2` with no launcher variables: bench.py is its own launcher; with fewer GPUs than ranks and the
    default backend (RCCL) it exits 2 with a clear message -- never a silent gloo run, never 'launch with torch.distributed.run'."""
    import subprocess
    import sys
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("two GPUs visible: the refusal does not apply")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "GPU(s) visible" in r.stderr and "torch.distributed.run" not in r.stderr


def test_diverse_ids_fixture_fires_every_id():
    """tests/golden/diverse_ids_240x320.npz (reference run, make_golden.py): the 16 firing cells carry >= 12 distinct ids, so the
    17-way ids arg-max and the id column of the result are exercised on diverse winners (the random-init heads fire 1-3 ids)."""
    fx = np.load(os.path.join(GOLDEN, "diverse_ids_240x320.npz"))
    ids = fx["ids_found"]
    assert ids.shape == (16,) and len(set(ids.tolist())) >= 12 and int(fx["distinct_ids"]) == len(set(ids.tolist()))
    assert np.array_equal(np.sort(fx["final_rn"][:, 2]), np.sort(ids.astype(np.float64)))
    # the solver itself on synthetic logits: 3 classes dominate -> after the shift the top-16 carry >= 12 ids
    rng = np.random.default_rng(0)
    z = rng.standard_normal((17, 40, 30)) + np.array([3.0, 2.5, 2.0] + [0.0] * 14)[:, None, None]
    la = rng.integers(0, 65, (40, 30))
    before = z[:16].reshape(16, -1)[:, la.ravel() != 64]
    top = np.argsort(-(before.max(0) - z[16].ravel()[la.ravel() != 64]))[:16]
    assert len(set(before.argmax(0)[top].tolist())) <= 6
    shift, d = W.diverse_ids_bias_shift(z, la, 16, 16)
    assert shift.dtype == np.float32 and shift.shape == (16,) and d >= 12 and abs(float(shift.mean())) < 1e-5


def test_lds_bank_model_of_the_raw_tile_layouts():
    """tools/lds_sim.py restates the LDS banking rules of gfx950 (lane groups / bank modulus per instruction) and the raw-tile
    layouts of the Winograd kernels.  It reproduced round 3's SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE per kernel to the digit
    (8x16: 2.8 %, 6x20: 17.0 %, 16-tile items: 3.8 %), which is how round 4's layouts were found; this pins the model's verdict on
    them: the planar 6x20 tile is at 2.2 % (measured: 2.24 %), no transform read of any layout conflicts."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("lds_sim", os.path.join(REPO, "tools", "lds_sim.py"))
    sim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sim)
    pct = lambda r: 100.0 * sum(v[1] for v in r.values()) / sum(v[0] for v in r.values())
    old_6x20 = sim.wino2h(6, 20)                                         # rounds 2-3: pitch 23 + row-pair shift
    planar = sim.wino2h(6, 20, slot_of=lambda img, cq, hy, hx: cq * 216 + (hx & 1) * 108 + hy * 13 + (hx >> 1))
    assert abs(pct(old_6x20) - 17.0) < 0.1 and old_6x20["xform_read"][1] == 192
    assert pct(planar) < 2.5 and planar["xform_read"][1] == 0 and planar["load_b"][1] == 0
    for r in (sim.wino2h(8, 16), sim.wino2h(8, 8, G=2), sim.wino2h(8, 8, TB=1), sim.wino2p(8, 16), sim.wino2p(8, 8, 2)):
        assert r["xform_read"][1] == 0 and r["load_b"][1] == 0 and r["xform_write"][1] == 0
    # the split-position shape (csrc/dcx_conv_wino2hs.h): with its own row shift no transform read conflicts (measured: 18 % -> 6.5 % of
    # the 16-cout variant's LDS cycles, what is left are raw-tile stores across a row end); with wino2h's shift a third of them did
    for cg in (4, 2, 1):
        r = sim.wino2hs(cg)
        assert r["xform_read"][1] == 0 and r["load_b"][1] == 0 and r["xform_write"][1] == 0 and r["exchange_read(item)"][1] == 0
        assert sim.wino2hs(cg, shift=lambda hy: (hy >> 2) & 1)["xform_read"][1] > 0
    assert "hx + ((hy >> 1) & 1)" in open(os.path.join(REPO, "deepcharuco_amd", "csrc", "dcx_conv_wino2hs.h")).read()
    # the constants the header uses for the planar tile (csrc/dcx_conv_wino2h.h)
    src = open(os.path.join(REPO, "deepcharuco_amd", "csrc", "dcx_conv_wino2h.h")).read()
    assert "PRP = 13, PODD = 108, PCQ = 216" in src


class _RecordingCv2:
    """Stand-in for the three drawing calls of OpenCV (cv2 is not installable here): records what it is asked to draw."""
    FONT_HERSHEY_COMPLEX_SMALL = 5

    def __init__(self):
        self.calls = []

    def circle(self, img, center, radius, color, thickness):
        self.calls.append(("circle", center, radius, color, thickness))
        img[min(center[1], img.shape[0] - 1), min(center[0], img.shape[1] - 1)] = color

    def getTextSize(self, text, font, scale, thickness):
        return (8 * len(text), 10), 3

    def putText(self, img, text, pos, font, scale, color, thickness):
        self.calls.append(("text", text, pos, color))


def test_draw_inner_corners_semantics(monkeypatch):
    """draw_pred=True (inference.py:47-50,63-66 -> aruco_utils.draw_inner_corners:135-192): drawing happens on a COPY, corners are
    rounded to the nearest pixel, corners beyond the right / bottom edge are skipped, ids are drawn in green only when asked."""
    import sys
    from deepcharuco_amd import inference as I
    rec = _RecordingCv2()
    monkeypatch.setitem(sys.modules, "cv2", rec)
    img = np.zeros((20, 30, 3), np.uint8)
    corners = np.array([[3.4, 4.6], [29.5, 19.49], [31.0, 5.0], [5.0, 21.0]])
    out = I.draw_inner_corners(img, corners, np.array([7, 12, 1, 2]), draw_ids=True, radius=3, color=(0, 0, 255))
    assert out is not img and not img.any() and out.any()
    circles = [c for c in rec.calls if c[0] == "circle"]
    assert [c[1] for c in circles] == [(3, 5), (30, 19)] and all(c[2] == 3 and c[3] == (0, 0, 255) and c[4] == 1 for c in circles)
    texts = [c for c in rec.calls if c[0] == "text"]
    assert [t[1] for t in texts] == ["7", "12"] and texts[0][2] == (3 - 4 - 7, 5 + 5 - 3) and all(t[3] == (0, 255, 0) for t in texts)
    rec.calls.clear()
    I.draw_inner_corners(img, corners[:1], np.array([7]), draw_ids=False, radius=1, color=(0, 255, 255))
    assert rec.calls == [("circle", (3, 5), 1, (0, 255, 255), 1)]
    monkeypatch.setitem(sys.modules, "cv2", None)
    with pytest.raises(ImportError, match="OpenCV"):
        I.draw_inner_corners(img, corners, np.array([7, 12, 1, 2]))


def test_loc_nocorner_bias_shift_window_margin_and_refusal():
    """weights.loc_nocorner_bias_shift: after the shift class 64 wins on a share of cells inside the window, every cell's loc top-2
    margin is >= min_margin, and it refuses when no gap can give that margin."""
    rng = np.random.default_rng(5)
    loc = rng.standard_normal((2, 65, 30, 40)).astype(np.float32)
    d = W.loc_nocorner_bias_shift(loc)
    z = loc.astype(np.float64).copy()
    z[:, 64] += d
    win = z.argmax(1) == 64
    assert 0.85 <= win.mean() <= 0.95
    top = np.sort(z, axis=1)
    assert (top[:, -1] - top[:, -2]).min() >= 1e-4
    one = W.loc_nocorner_bias_shift(loc[0], 0.5, 0.6, 0.0)               # (65, h, w): one frame
    assert 0.5 <= ((loc[0, :64].max(0) - loc[0, 64]) < one).mean() <= 0.6
    flat = np.zeros((65, 8, 8), np.float32)                               # every cell ties: no gap anywhere
    with pytest.raises(ValueError):
        W.loc_nocorner_bias_shift(flat)
