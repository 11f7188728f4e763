"""A numpy restatement of the three index-only contracts of the staged C ABI (include/deepcharuco_amd.h): the decode of dense
label maps into capped per-frame rows, the patch table over a batch, and the 24x24 gather out of u8 frames.

Written from the header's words and from the reference's functions they cite (model_utils.py:19-36, :46-50, :91-124), not from
csrc/dcx_misc.hip or the device headers it calls (dcx_cell_dev.h, dcx_first_dev.h): plain loops and slices over the cells in raster order, no scan, no ballot, no clamped addressing.  tests/test_staged_abi_host.py pins each
function to the oracle's stage functions; tests/test_gpu_staged_abi.py compares the kernels with it by exact equality.

Everything is integer arithmetic except gather_u8, whose one float32 expression ((float32(g) - 128) / 255, IEEE division) is
pre_bgr_image's.
"""
import numpy as np

SENTINEL = -7777          # what decode_rows leaves in rows it does not fill (the GPU tests prefill their buffers with it too)


def decode_rows(loc_argmax, ids_argmax, dust_bin, kmax, sentinel=SENTINEL):
    """Label maps [B][Hc][Wc] (ids already masked by loc == 64, as pred_argmax returns them) -> (counts [B] int32, never capped;
    rows [B][kmax][4] int32 = (x, y, id, cell)).  A cell fires when its id != dust_bin; rows in raster order (torch.nonzero's);
    x = 8*cx + loc % 8, y = 8*cy + loc // 8, cell = cy*Wc + cx.  The first min(count, kmax) rows of a frame are filled, the rest
    keep ``sentinel``."""
    loc = np.asarray(loc_argmax, dtype=np.int64)
    ids = np.asarray(ids_argmax, dtype=np.int64)
    assert loc.ndim == 3 and loc.shape == ids.shape and kmax >= 1
    b, hc, wc = loc.shape
    counts = np.zeros(b, np.int32)
    rows = np.full((b, kmax, 4), sentinel, np.int32)
    for f in range(b):
        fired = np.flatnonzero(ids[f].reshape(-1) != dust_bin)          # raster order: cell = cy*Wc + cx ascending
        counts[f] = fired.size
        for k, cell in enumerate(fired[:kmax]):
            cy, cx = divmod(int(cell), wc)
            l = int(loc[f, cy, cx])
            rows[f, k] = (8 * cx + l % 8, 8 * cy + l // 8, ids[f, cy, cx], cell)
    return counts, rows


def patch_table(counts, rows, kmax):
    """(counts [B], rows [B][kmax][4]) -> (table [total][4] int32 = (frame, x, y, frame*kmax + k), total = sum_b min(counts[b],
    kmax)): frames in order, each frame's stored rows in order."""
    counts = np.asarray(counts, dtype=np.int64)
    rows = np.asarray(rows)
    assert rows.shape == (counts.shape[0], kmax, 4)
    out = []
    for f, c in enumerate(counts):
        for k in range(min(int(c), kmax)):
            out.append((f, int(rows[f, k, 0]), int(rows[f, k, 1]), f * kmax + k))
    table = np.array(out, np.int32).reshape(-1, 4)
    return table, int(table.shape[0])


def gather_u8(frames, table):
    """frames: sequence of [H][W] uint8 arrays (all the same size); table rows (frame, x, y, slot) -> [P][24][24] float32,
    patch[p][i][j] = (float32(g) - 128) / 255 of pixel (y - 12 + i, x - 12 + j) of frame table[p][0] inside the image, 0.0f
    outside."""
    table = np.asarray(table).reshape(-1, 4)
    out = np.zeros((table.shape[0], 24, 24), np.float32)
    for p, (f, x, y, _) in enumerate(table):
        img = np.asarray(frames[int(f)])
        assert img.dtype == np.uint8 and img.ndim == 2
        h, w = img.shape
        for i in range(24):
            iy = int(y) - 12 + i
            if iy < 0 or iy >= h:
                continue
            for j in range(24):
                ix = int(x) - 12 + j
                if 0 <= ix < w:
                    out[p, i, j] = (np.float32(img[iy, ix]) - np.float32(128)) / np.float32(255)
    return out
