"""resize.resize_host(..., "area_any") on the host -- cv2's general INTER_AREA, a box filter with fractional end taps: the numpy
definition against a float64 box integral written here on its own, the 1e-3 rule against a tap table derived by hand, the routing
rule against the definition written out here, the layouts and the identities that hold, what Python refuses, and the refusals of
the C entry dcx_resize_area_u8 (which come before anything is launched, so they need no GPU)."""
import ctypes
import math

import numpy as np
import pytest

import resize_any_cases as ac
from deepcharuco_amd import resize as rz


def _frames(shape, kind, seed):
    return ac.noise(shape, seed) if kind == "noise" else ac.extremes(shape, seed)


def _overlap(sn, dn):
    """(dn, sn) float64: the share of the cell [d sn / dn, (d + 1) sn / dn) that source pixel [s, s + 1) covers."""
    d, s = np.arange(dn, dtype=np.float64)[:, None], np.arange(sn, dtype=np.float64)[None, :]
    lo, hi = d * sn / dn, (d + 1) * sn / dn
    return np.clip(np.minimum(hi, s + 1) - np.maximum(lo, s), 0, None) / (sn / dn)


def _box_f64(img, dh, dw):
    """The float64 box integral of (H, W): every source pixel weighted by the share of the output pixel's cell it covers."""
    sh, sw = img.shape
    return _overlap(sh, dh) @ img.astype(np.float64) @ _overlap(sw, dw).T


def _taps_written_out(d, dn, sn):
    """The tap table of output index d as the module docstring states it, in python floats: [(index, float32 weight), ...]."""
    scale = 1.0 / (dn / sn)
    f1 = d * scale
    f2 = f1 + scale
    cell = min(scale, sn - f1)
    s1, s2 = math.ceil(f1), min(math.floor(f2), sn - 1)
    s1 = min(s1, s2)
    taps = []
    if s1 - f1 > 1e-3:
        taps.append((s1 - 1, np.float32((s1 - f1) / cell)))
    for s in range(s1, s2):
        taps.append((s, np.float32(1.0 / cell)))
    if f2 - s2 > 1e-3:
        taps.append((s2, np.float32(min(min(f2 - s2, 1.0), cell) / cell)))
    return taps


def _general_written_out(img, dh, dw):
    """The general path on BOTH axes for (H, W), pixel by pixel in float32: horizontal first, then vertical."""
    sh, sw = img.shape
    ytaps, xtaps = [_taps_written_out(d, dh, sh) for d in range(dh)], [_taps_written_out(d, dw, sw) for d in range(dw)]
    out = np.zeros((dh, dw), np.uint8)
    for y in range(dh):
        for x in range(dw):
            v = None
            for sy, b in ytaps[y]:
                h = None
                for sx, a in xtaps[x]:
                    prod = np.float32(img[sy, sx]) * a
                    h = prod if h is None else np.float32(h + prod)
                v = np.float32(b * h) if v is None else np.float32(v + np.float32(b * h))
            out[y, x] = np.clip(np.rint(v), 0, 255)
    return out


def _table(dn, sn):
    """rz's own table of an axis as lists of (index, weight) per output index."""
    index, weight, count = rz._area_any_axis(dn, sn)
    assert index.shape == weight.shape and weight.dtype == np.float32
    return [[(int(index[d, k]), weight[d, k]) for k in range(count[d])] for d in range(dn)]


@pytest.mark.parametrize("shape", ac.EXACT_SHAPES, ids=ac.shape_id)
def test_area_any_is_the_rounded_box_integral(shape):
    """|out - exact| <= 0.5 + 255 n 2^-23 with n = (ceil(scale_x) + 1)(ceil(scale_y) + 1): 0.5 is the final rounding, the rest n
    float32 roundings of values up to 255.  Holds where no true sliver is dropped (dn < 1000 on both axes).  The largest excess
    over 0.5 observed on these shapes is printed (5.7e-14, on 8x8 -> 8x5: the float64 reference's own rounding on an exact
    tie)."""
    sh, sw, dh, dw = shape
    assert dh < 1000 and dw < 1000
    n = (math.ceil(sw / dw) + 1) * (math.ceil(sh / dh) + 1)
    gate = 0.5 + 255 * n * 2.0 ** -23
    for kind in ("noise", "extremes"):
        img = _frames((sh, sw), kind, sh * 7 + sw)
        got = rz.resize_host(img, (dh, dw), "area_any")
        assert got.shape == (dh, dw) and got.dtype == np.uint8
        gap = float(np.abs(got.astype(np.float64) - _box_f64(img, dh, dw)).max())
        print(f"area_any {ac.shape_id(shape)} {kind}: worst {gap:.6f} (gate {gate:.6f}, over 0.5 by {max(gap - 0.5, 0):.2e})")
        assert gap <= gate, (shape, kind, gap, gate)


def test_the_1e_3_rule_on_2003_to_2002():
    """scale = 2003/2002 = 1 + 1/2002: cell d is [d + d/2002, d + 1 + (d + 1)/2002).  Its first tap covers 1 - d/2002 of pixel d
    (a whole pixel for d = 0) and its last (d + 1)/2002 of pixel d + 1: 0.0004995 for d = 0 and 0.000999 for d = 1, both at most
    1e-3 and dropped WITHOUT renormalising the other tap; 0.0014985 for d = 2 and 0.001998 for d = 3, kept.  The last cell
    [2001 + 2001/2002, 2003) has a first tap of 1/2002 of pixel 2001, dropped, and pixel 2002 whole (taken as the last tap,
    since s2 is clipped to sn - 1)."""
    sn, dn = 2003, 2002
    cell = sn / dn
    f32 = np.float32
    expected = {
        0: [(0, f32(1.0 / cell))],
        1: [(1, f32((1 - 1 / 2002) / cell))],
        2: [(2, f32((1 - 2 / 2002) / cell)), (3, f32((3 / 2002) / cell))],
        3: [(3, f32((1 - 3 / 2002) / cell)), (4, f32((4 / 2002) / cell))],
        dn - 1: [(2002, f32(1.0 / cell))],
    }
    table = _table(dn, sn)
    for d, taps in expected.items():
        got = table[d]
        assert [i for i, _ in got] == [i for i, _ in taps], (d, got)
        for (_, w), (_, e) in zip(got, taps):
            assert abs(float(w) - float(e)) <= 2.0 ** -22, (d, got, taps)      # (the hand value's fractions are rounded differently)
        assert got == _taps_written_out(d, dn, sn), d
    assert sum(float(w) for _, w in table[0]) < 0.9996 and sum(float(w) for _, w in table[2]) == pytest.approx(1.0, abs=1e-6)
    sh, sw, dh, dw = ac.SLIVER_SHAPE
    img = ac.noise((sh, sw), 9)
    assert np.array_equal(rz.resize_host(img, (dh, dw), "area_any"), _general_written_out(img, dh, dw))


@pytest.mark.parametrize("dn,sn", [(2, 9), (3, 10), (16, 72), (52, 53), (7, 31), (2, 127), (1, 13), (4, 9), (5, 8), (400, 900), (5, 15)])
def test_tap_tables_are_the_definition_written_out(dn, sn):
    """Every row of the vectorised table equals the scalar definition; the taps of a cell are consecutive pixels inside the frame,
    they do not decrease along the axis, and (no sliver dropped here) their weights sum to 1 within float32."""
    table = _table(dn, sn)
    first_prev, last_prev = 0, 0
    for d in range(dn):
        assert table[d] == _taps_written_out(d, dn, sn), d
        idx = [i for i, _ in table[d]]
        assert len(idx) >= 1 and idx == list(range(idx[0], idx[0] + len(idx))) and idx[0] >= 0 and idx[-1] <= sn - 1
        assert idx[0] >= first_prev and idx[-1] >= last_prev
        first_prev, last_prev = idx[0], idx[-1]
        assert len(idx) <= math.ceil(sn / dn) + 2
        assert sum(float(w) for _, w in table[d]) == pytest.approx(1.0, abs=len(idx) * 2.0 ** -24 + 1e-3 / (sn / dn))


@pytest.mark.parametrize("shape", ac.INTEGER_SHAPES, ids=ac.shape_id)
def test_integer_factors_on_both_axes_are_area(shape):
    """cv2's fast-path rule, against "area"'s definition written out: the integer sum of the block, (sum + 2) >> 2 for 2 x 2, else
    rint(float32(sum) * float32(1 / (fx fy)))."""
    sh, sw, dh, dw = shape
    fy, fx = sh // dh, sw // dw
    for kind in ("noise", "extremes"):
        for lead in ((), (2,)):
            for tail in ((), (3,)):
                img = _frames(lead + (sh, sw) + tail, kind, sh + sw)
                s = img.reshape((lead or (1,)) + (dh, fy, dw, fx) + (tail or (1,))).astype(np.int64).sum(axis=(2, 4))
                if (fy, fx) == (2, 2):
                    exp = (s + 2) >> 2
                else:
                    exp = np.rint(s.astype(np.float32) * np.float32(1.0 / (fx * fy)))
                exp = exp.astype(np.uint8).reshape(lead + (dh, dw) + tail)
                got = rz.resize_host(img, (dh, dw), "area_any")
                assert np.array_equal(got, exp)
                assert np.array_equal(got, rz.resize_host(img, (dh, dw), "area"))


def test_an_integer_factor_on_one_axis_takes_the_general_path_on_both():
    """(15, 31, 5, 7): 3 in y, 31/7 in x.  The result is the general path on both axes, written out here pixel by pixel -- and is
    not "area"'s integer row sums followed by one rounding: in y every weight is float32(1/3) and every row's horizontal sum is
    rounded before it is weighted."""
    sh, sw, dh, dw = 15, 31, 5, 7
    assert _taps_written_out(1, dh, sh) == [(s, np.float32(1.0 / 3.0)) for s in (3, 4, 5)]
    for kind in ("noise", "extremes"):
        img = _frames((sh, sw), kind, 4)
        assert np.array_equal(rz.resize_host(img, (dh, dw), "area_any"), _general_written_out(img, dh, dw))
    for shape in ((9, 9, 2, 2), (10, 10, 3, 3), (8, 8, 8, 5), (1, 9, 1, 4), (7, 13, 1, 1)):
        img = ac.noise(shape[:2], 11)
        assert np.array_equal(rz.resize_host(img, shape[2:], "area_any"), _general_written_out(img, *shape[2:])), shape


def test_layouts_channels_and_frames():
    sh, sw, dh, dw = 27, 36, 6, 8
    x = ac.noise((3, sh, sw, 3), 8)
    got = rz.resize_host(x, (dh, dw), "area_any")
    assert got.shape == (3, dh, dw, 3) and got.dtype == np.uint8 and got.flags.c_contiguous
    for b in range(3):
        assert np.array_equal(rz.resize_host(x[b], (dh, dw), "area_any"), got[b])                # (H, W, 3): one colour frame
        for c in range(3):
            assert np.array_equal(rz.resize_host(np.ascontiguousarray(x[b, :, :, c]), (dh, dw), "area_any"), got[b, :, :, c])
    gray = np.ascontiguousarray(x[..., 0])
    assert np.array_equal(rz.resize_host(gray, (dh, dw), "area_any"), got[..., 0])               # (B, H, W)


def test_identities_that_hold():
    """A constant image stays constant: the weights of a cell sum to 1 within a few float32 ulps, far from the rounding boundary
    of an integer level.  A flipped input does NOT give the flipped output as an identity in bits, even where the table is
    symmetric (9 -> 2: cells [0, 4.5) and [4.5, 9) mirror each other, with the same weights in mirrored order): the float32 sums
    run from the left and from the top, so the mirrored cell adds the same products in the other order, and where the table is
    not symmetric (10 -> 3: f1 = d * scale is measured from the left edge only, and the last cell's f2 may land a hair under 10)
    the weights differ in their last bits as well.  Before the final rounding the two differ by float32 roundings of values up
    to 255 (the gate of the exact-math test), so what holds, and is asserted, is that they are within one gray level; how many
    pixels differ is printed."""
    for level in (0, 1, 77, 128, 254, 255):
        for sh, sw, dh, dw in ac.EXACT_SHAPES:
            img = np.full((sh, sw), level, np.uint8)
            assert np.array_equal(rz.resize_host(img, (dh, dw), "area_any"), np.full((dh, dw), level, np.uint8)), (level, sh, sw)
    for sh, sw, dh, dw in ((9, 9, 2, 2), (10, 10, 3, 3), (54, 72, 12, 16)):
        img = ac.noise((4, sh, sw), 2)
        a = rz.resize_host(img[:, ::-1, ::-1], (dh, dw), "area_any").astype(int)
        b = rz.resize_host(img, (dh, dw), "area_any")[:, ::-1, ::-1].astype(int)
        print(f"flip {sh}x{sw} -> {dh}x{dw}: {int((a != b).sum())} of {a.size} pixels differ")
        assert np.abs(a - b).max() <= 1


def test_python_refusals():
    img = ac.noise((10, 10), 1)
    assert rz.resize_host(img, (3, 3), "area_any").shape == (3, 3)
    with pytest.raises(ValueError):
        rz.resize_host(img, (11, 5), "area_any")                             # area does not enlarge, on either axis
    with pytest.raises(ValueError):
        rz.resize_host(img, (5, 11), "area_any")
    with pytest.raises(ValueError):
        rz.resize_host(ac.noise((129, 7), 1), (2, 7), "area_any")            # a factor of 64.5
    with pytest.raises(ValueError):
        rz.resize_host(ac.noise((7, 65), 1), (7, 1), "area_any")             # 65, an integer beyond the cap: not routed either
    assert rz.resize_host(ac.noise((128, 7), 1), (2, 3), "area_any").shape == (2, 3)             # 64 and 2.33
    with pytest.raises(ValueError):
        rz.resize_host(img.astype(np.float32), (5, 5), "area_any")
    with pytest.raises(ValueError):
        rz.resize_host(ac.noise((2, 4, 4, 2), 1), (2, 2), "area_any")        # two channels
    with pytest.raises(ValueError):
        rz.resize_host(np.zeros((0, 4), np.uint8), (2, 2), "area_any")
    with pytest.raises(ValueError):
        rz.resize_host(img, (0, 5), "area_any")
    with pytest.raises(ValueError):
        rz.resize_host(img, (3, 3), "area-any")
    with pytest.raises(ValueError):
        rz.resize_host(img, (3, 3), "area")                                  # the old mode still refuses a fractional factor
    assert "area_any" not in rz.INTERPOLATIONS and sorted(rz.INTERPOLATIONS.values()) == [0, 1, 2]


def test_c_entry_refuses_before_it_launches():
    """Every call here is refused, so nothing is launched and the pointers (never read) need not be device memory."""
    from deepcharuco_amd import _lib
    lib = _lib.lib()
    E_ARG, E_SHAPE = -1, -2
    p = ctypes.c_void_p(4096)

    def call(src=p, stride=0, pitch=64, sh=9, sw=9, ch=1, dh=2, dw=2, batch=1, out=p):
        return lib.dcx_resize_area_u8(src, stride, pitch, sh, sw, ch, dh, dw, batch, out, None)

    assert call(src=None) == E_ARG and call(out=None) == E_ARG
    assert call(ch=2) == E_ARG and call(ch=0) == E_ARG and call(ch=4) == E_ARG
    assert call(stride=-1) == E_ARG
    assert call(ch=2, sh=0) == E_ARG                                         # a bad argument is named before a bad shape
    for name in ("sh", "sw", "dh", "dw", "batch"):
        for v in (0, -1, 32769):
            assert call(**{name: v, "pitch": 40000}) == E_SHAPE, (name, v)
    assert call(pitch=8) == E_SHAPE and call(ch=3, pitch=26) == E_SHAPE      # a short pitch
    assert call(pitch=70000, sh=32768, dh=32767) == E_SHAPE                  # pitch * src_h beyond an int32
    assert call(sh=9, sw=9, dh=10, dw=2) == E_SHAPE                          # an enlargement, on either axis
    assert call(sh=9, sw=9, dh=2, dw=10) == E_SHAPE
    assert call(sh=8, sw=8, dh=16, dw=16) == E_SHAPE
    assert call(sh=65, sw=9, dh=1, dw=2) == E_SHAPE                          # a factor of 65
    assert call(sh=9, sw=130, pitch=130, dh=2, dw=2) == E_SHAPE
    assert call(sh=129, sw=9, dh=2, dw=2) == E_SHAPE                         # 64.5
    assert lib.dcx_resize_u8(p, 0, 64, 8, 8, 1, 4, 4, 1, 3, p, None) == E_ARG                    # the old entry has no code 3
