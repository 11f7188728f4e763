"""Device time of the resize (resize.resize_device, csrc/dcx_resize.hip's dcx_resize_u8) in front of the detector: 32 x 960 x 1280 BGR
and 32 x 1440 x 1920 BGR -> 240 x 320, "nearest", "linear" and "area", against two yardsticks run in the same process,
alternating with it round by round:

(a) a device copy of as many bytes as the resize must read plus write (torch's copy_ of a u8 buffer of half that size): the
    ceiling.  Must read: the source rows an output row takes its taps from, whole -- all of them for "area", the two tap rows of
    each output row for "linear", one for "nearest" (a row's pixels in between share the taps' cache lines);
(b) what a user would write without this kernel: torch.nn.functional.interpolate ("nearest", "bilinear" without align_corners,
    "area") on a float copy of the frames, the u8 -> float and float -> u8 conversions and the NHWC <-> NCHW views included.  Its
    result is NOT the resize's bits (float weights; another nearest rule); the largest difference in gray levels is reported.

Timing: device events around `inner` back-to-back calls, rounds repeated until the resize alone has run for --seconds (default
0.5 s) after three warm-up calls of each; the figure is the median round's time per call.  Each shape is also checked against
resize_host on its first two frames.  Prints one JSON object and writes it to --out.

The 1080p case ("window_1080p"): 32 x 1080 x 1920 BGR frames whose 1440 x 1080 window is read in place (rows of 1,440 * 3 bytes at
a 5,760-byte pitch) -> 240 x 320 with "area_any" (a factor of 4.5, dcx_resize_area_u8), alternating with a device copy of the
bytes that call must read plus write (every row of the window), with "linear" on the same window (what such a user had before)
and with "area" 4 x from dense 960 x 1280 frames; two frames of each are compared with resize_host.

    python tools/resize_probe.py --out profiles/resize_probe.json
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from rectify_probe import alternate  # noqa: E402

TORCH_MODE = {"nearest": dict(mode="nearest"), "linear": dict(mode="bilinear", align_corners=False), "area": dict(mode="area")}


def rows_read(mode, sh, dh):
    """Source rows the output rows take their taps from (the definition's own tables)."""
    from deepcharuco_amd import resize as rz
    if mode == "area" or (mode == "linear" and sh == 2 * dh):
        return sh
    if mode == "nearest":
        return len(set(rz._nearest_axis(dh, sh).tolist()))
    y0, y1, _, _ = rz._linear_axis(dh, sh, False)
    return len(set(y0.tolist()) | set(y1.tolist()))


def window_1080p(torch, rz, weights, dev, batch, dh, dw, seconds):
    """The 1080p case of the module docstring -> its figures."""
    def frames_of(sh, sw):
        base = torch.from_numpy(weights.synthetic_frames("board", 21, 4, sh, sw)).to(dev)
        gray = base.repeat(-(-batch // 4), 1, 1)[:batch] + torch.arange(batch, device=dev, dtype=torch.uint8)[:, None, None]
        return torch.stack([gray, 255 - gray, gray // 2], 3).contiguous()

    full = frames_of(1080, 1920)
    window = full[:, :, 240:1680]                                              # 1440 x 1080, read in place
    dense = frames_of(960, 1280)
    assert not window.is_contiguous() and window.stride(1) == 5760
    out = {k: torch.empty((batch, dh, dw, 3), dtype=torch.uint8, device=dev) for k in ("area_any", "linear", "area_4x")}
    need = batch * (1080 * 1440 * 3 + dh * dw * 3)
    cs, cd = torch.zeros(need // 2, dtype=torch.uint8, device=dev), torch.empty(need // 2, dtype=torch.uint8, device=dev)
    fns = {"area_any": lambda: rz.resize_device(window, (dh, dw), "area_any", out=out["area_any"]),
           "copy": lambda: cd.copy_(cs),
           "linear": lambda: rz.resize_device(window, (dh, dw), "linear", out=out["linear"]),
           "area_4x": lambda: rz.resize_device(dense, (dh, dw), "area", out=out["area_4x"])}
    ms, inner, rounds = alternate(fns, seconds)
    host_ok = {}
    for k, src, mode in (("area_any", window, "area_any"), ("linear", window, "linear"), ("area_4x", dense, "area")):
        fns[k]()
        host_ok[k] = bool(np.array_equal(out[k][:2].cpu().numpy(), rz.resize_host(src[:2].cpu().numpy(), (dh, dw), mode)))
    res = {"case": f"{batch}x1080x1920x3[:, :, 240:1680]->{dh}x{dw}", "area_any_ms": ms["area_any"], "copy_ms": ms["copy"],
           "linear_ms": ms["linear"], "area_4x_960x1280_ms": ms["area_4x"], "bytes_needed": need,
           "area_any_GBps": need / ms["area_any"] / 1e6, "copy_GBps": 2 * (need // 2) / ms["copy"] / 1e6,
           "area_any_over_copy": ms["area_any"] / ms["copy"], "area_any_over_linear": ms["area_any"] / ms["linear"],
           "inner": inner, "rounds": rounds, "equals_resize_host": host_ok}
    print("window_1080p", json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import torch.nn.functional as TF
    from deepcharuco_amd import resize as rz, weights
    assert torch.cuda.is_available(), "resize_probe measures the GPU kernel: no GPU visible"
    dev = torch.device("cuda", 0)
    batch, dh, dw = a.batch, 240, 320
    result = {"device": torch.cuda.get_device_name(dev), "seconds": a.seconds, "resize": {}}
    for sh, sw in ((960, 1280), (1440, 1920)):
        base = torch.from_numpy(weights.synthetic_frames("board", 21, 4, sh, sw)).to(dev)
        gray = base.repeat(-(-batch // 4), 1, 1)[:batch]
        gray = gray + torch.arange(batch, device=dev, dtype=torch.uint8)[:, None, None]          # (wraps: `batch` different frames)
        frames = torch.stack([gray, 255 - gray, gray // 2], 3).contiguous()
        del gray, base
        out = torch.empty((batch, dh, dw, 3), dtype=torch.uint8, device=dev)
        for mode in ("nearest", "linear", "area"):
            key = f"{batch}x{sh}x{sw}x3->{dh}x{dw}/{mode}"
            need = batch * (rows_read(mode, sh, dh) * sw * 3 + dh * dw * 3)
            n_copy = need // 2
            cs, cd = torch.zeros(n_copy, dtype=torch.uint8, device=dev), torch.empty(n_copy, dtype=torch.uint8, device=dev)

            def resize():
                return rz.resize_device(frames, (dh, dw), mode, out=out)

            def copy():
                return cd.copy_(cs)

            def interpolate():
                y = TF.interpolate(frames.permute(0, 3, 1, 2).float(), size=(dh, dw), **TORCH_MODE[mode])
                return y.round_().clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()

            ms, inner, rounds = alternate({"resize": resize, "copy": copy, "interpolate": interpolate}, a.seconds)
            gap = int((interpolate().to(torch.int16) - resize().to(torch.int16)).abs().max())
            host_ok = bool(np.array_equal(resize()[:2].cpu().numpy(), rz.resize_host(frames[:2].cpu().numpy(), (dh, dw), mode)))
            result["resize"][key] = {
                "resize_ms": ms["resize"], "copy_ms": ms["copy"], "interpolate_ms": ms["interpolate"], "bytes_needed": need,
                "resize_GBps": need / ms["resize"] / 1e6, "copy_GBps": 2 * n_copy / ms["copy"] / 1e6,
                "resize_over_copy": ms["resize"] / ms["copy"], "interpolate_over_resize": ms["interpolate"] / ms["resize"],
                "inner": inner, "rounds": rounds, "interpolate_max_gray_level_gap": gap, "equals_resize_host": host_ok}
            print(key, json.dumps(result["resize"][key]), flush=True)
            del cs, cd
        del frames, out
    result["window_1080p"] = window_1080p(torch, rz, weights, dev, batch, dh, dw, a.seconds)
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f)


if __name__ == "__main__":
    main()
