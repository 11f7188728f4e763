"""Disparity maps for the speckle filter's tests (tests/test_speckle_host.py, tests/test_gpu_speckle.py).  Nothing here imports
deepcharuco_amd.  A case is (name, disp16 int16 (H, W) or (B, H, W), new_val, max_speckle_size, max_diff, expected or None)."""
import numpy as np

NV = -16                                     # the matcher's invalid value at min_disparity = 0


def _a(rows):
    return np.array(rows, np.int16)


def hand_cases():
    """Cases small enough to state the answer: -> list of (name, disp16, new_val, max_speckle_size, max_diff, expected)."""
    n = NV
    cases = []

    def add(name, disp, new_val, size, diff, expected):
        cases.append((name, _a(disp), new_val, size, diff, _a(expected)))

    add("1x1 removed", [[5]], n, 1, 0, [[n]])
    add("1x1 kept", [[5]], n, 0, 0, [[5]])
    row, row_out = [3, 3, 3, 9, 9, n, 3], [3, 3, 3, n, n, n, n]
    add("1xW", [row], n, 2, 0, [row_out])
    add("Hx1", [[v] for v in row], n, 2, 0, [[v] for v in row_out])
    # a component of exactly max_speckle_size pixels goes, one of a pixel more stays
    six_seven = [[40, 40, 40, n, 56, 56, 56],
                 [40, 40, 40, n, 56, 56, 56],
                 [n, n, n, n, n, 56, n]]
    add("size and size + 1", six_seven, n, 6, 0, [[n, n, n, n, 56, 56, 56], [n, n, n, n, 56, 56, 56], [n, n, n, n, n, 56, n]])
    add("size 0 is the identity", six_seven, n, 0, 0, six_seven)
    add("max_diff 0 joins equal values only", [[1, 1, 2, 2, 2, 1]], n, 2, 0, [[n, n, 2, 2, 2, n]])
    add("max_diff 1 joins them all", [[1, 1, 2, 2, 2, 1]], n, 5, 1, [[1, 1, 2, 2, 2, 1]])
    ramp = [[4 * i for i in range(20)]]
    add("a ramp in steps of max_diff is one component: kept at 19", ramp, n, 19, 4, ramp)
    add("a ramp in steps of max_diff is one component: removed at 20", ramp, n, 20, 4, [[n] * 20])
    add("a ramp in steps above max_diff is 20 components", ramp, n, 1, 3, [[n] * 20])
    add("new_val separates two equal regions", [[7, 7, 7, n, 7, 7, 7]], n, 3, 0, [[n] * 7])
    add("new_val separates two equal regions, column", [[7], [7], [n], [7], [7]], n, 2, 100, [[n]] * 5)
    # new_val = 0 is a value of the data too: those pixels are no component and join nothing
    add("a data value equal to new_val", [[5, 5, 0, 5, 5], [0, 0, 0, 0, 5]], 0, 2, 5, [[0, 0, 0, 5, 5], [0, 0, 0, 0, 5]])
    add("int16 extremes apart at 65534", [[-32768, 32767]], 0, 1, 65534, [[0, 0]])
    add("int16 extremes joined at 65535", [[-32768, 32767]], 0, 1, 65535, [[-32768, 32767]])
    add("a row's end and the next row's start are not neighbours", [[n, n, 7], [7, n, n]], n, 1, 0, [[n] * 3] * 2)
    # frame 0 ends in the row that frame 1 starts with: 3 pixels each unless frames leak
    cases.append(("frames do not leak", _a([[[n] * 3, [7] * 3], [[7] * 3, [n] * 3]]), n, 3, 0, np.full((2, 2, 3), n, np.int16)))
    return cases


def serpentine(h, w, step=4):
    """A one-pixel-wide path: every even row in full, joined alternately at the right and at the left end, on new_val; the values
    along the path are a triangle wave in steps of ``step`` (one component at max_diff = step, however far its ends are apart).
    -> (disp16, path length)."""
    a = np.full((h, w), NV, np.int16)
    k = 0
    for y in range(0, h, 2):
        xs = range(w) if (y // 2) % 2 == 0 else range(w - 1, -1, -1)
        cells = [(y, x) for x in xs]
        if y + 2 < h:
            cells.append((y + 1, cells[-1][1]))
        for cy, cx in cells:
            a[cy, cx] = step * abs(k % 100 - 50)
            k += 1
    return a, k


def spiral(h, w, value=48):
    """A one-pixel-wide rectangular spiral from the corner inwards, a free pixel between its turns.  -> (disp16, path length)."""
    a = np.full((h, w), NV, np.int16)
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))

    def free(y, x):
        return not (0 <= y < h and 0 <= x < w) or a[y, x] == NV

    y = x = d = 0
    a[0, 0] = value
    n = 1
    while True:
        for turn in (0, 1):
            dy, dx = dirs[(d + turn) % 4]
            if 0 <= y + dy < h and 0 <= x + dx < w and free(y + dy, x + dx) and free(y + 2 * dy, x + 2 * dx):
                d = (d + turn) % 4
                y, x = y + dy, x + dx
                a[y, x] = value
                n += 1
                break
        else:
            return a, n


def comb(h, w, value=48):
    """The top row and every other column below it.  -> (disp16, pixels)."""
    a = np.full((h, w), NV, np.int16)
    a[0, :] = value
    a[:, ::2] = value
    return a, int((a != NV).sum())


def checkerboard(h, w):
    """0 and 100 in turn: at max_diff < 100 every pixel is a component."""
    ys, xs = np.mgrid[0:h, 0:w]
    return (100 * ((ys + xs) & 1)).astype(np.int16)


def random_map(seed, shape, share_new_val=0.25, values=(0, 40, 80)):
    """Values from a small set and a share of new_val: at max_diff below the values' spacing the components have a few pixels
    each, on both sides of a max_speckle_size of 3."""
    rng = np.random.default_rng([97, seed] + list(shape))
    a = rng.choice(np.array(values, np.int16), size=shape)
    a[rng.random(shape) < share_new_val] = NV
    return a.astype(np.int16)
