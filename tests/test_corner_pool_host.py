"""The packed corner pool's word layout, pinned by literal numbers that nothing here computes from ``corner_pool``: ``views`` and
``ptrs`` cannot be wrong together unnoticed.  counts[B] | starts[B] | rows[pool][4] | xy[pool][2] | conf[pool][2]."""
import numpy as np
import torch

from deepcharuco_amd import corner_pool as cp


def test_offsets_lengths_and_addresses_for_batch_3_pool_5():
    at = cp.layout(3, 5)
    assert (at.counts, at.starts, at.rows, at.xy, at.conf) == (0, 3, 6, 26, 36) and all(type(w) is int for w in at)
    assert cp.packed_len(3, 5) == 36 and cp.packed_len(3, 5, True) == 46
    A = 0x7F0000001000
    assert cp.ptrs(A, 3, 5) == (A, A + 12, A + 24, A + 104, A + 144)
    from deepcharuco_amd import inference, sharding
    assert inference.packed_len is cp.packed_len and sharding.packed_len is cp.packed_len          # the re-exports


def test_views_are_views_at_the_literal_offsets():
    packed = np.arange(46, dtype=np.int32)
    counts, starts, rows, xy, conf = cp.views(packed, 3, 5)
    assert counts.tolist() == [0, 1, 2] and starts.tolist() == [3, 4, 5]
    assert rows.shape == (5, 4) and rows.dtype == np.int32 and rows[0].tolist() == [6, 7, 8, 9] and rows[4, 3] == 25
    assert xy.shape == (5, 2) and xy.dtype == np.float32 and xy.view(np.int32)[0].tolist() == [26, 27] and xy.view(np.int32)[4, 1] == 35
    assert conf.shape == (5, 2) and conf.dtype == np.float32 and conf.view(np.int32).ravel().tolist() == list(range(36, 46))
    for v in (counts, starts, rows, xy, conf):
        assert np.shares_memory(v, packed)
    rows[2, 1], xy[1, 0], conf[0, 1] = -4, 1.5, 0.25
    assert packed[15] == -4 and packed[28] == 0x3FC00000 and packed[37] == 0x3E800000
    # a section the buffer ends before is None
    assert cp.views(packed[:36], 3, 5)[4] is None and cp.views(packed[:36], 3, 5)[3] is not None
    short = cp.views(packed[:26], 3, 5)
    assert short[3] is None and short[4] is None and short[2].shape == (5, 4)
    head = cp.views(packed[:6], 3, 5)
    assert head[0].tolist() == [0, 1, 2] and head[1].tolist() == [3, 4, 5] and head[2:] == (None, None, None)


FRAMES = [np.array([[10.5, 20.25, 5], [1.5, 2.5, 2], [3.0, 4.0, 7]]),               # not id-sorted
          np.array([[8.0, 9.0, 0], [16.5, 17.5, 1], [24.0, 25.0, 3]])]
PACKED = np.array([3, 3, 0, 3,                                                         # counts | starts
                   0, 0, 2, 0, 0, 0, 5, 0, 0, 0, 7, 0,                                 # rows: the id word only, x = y = cell = 0
                   0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 3, 0,
                   0x3FC00000, 0x40200000, 0x41280000, 0x41A20000, 0x40400000, 0x40800000,   # xy: 1.5 2.5 | 10.5 20.25 | 3 4
                   0x41000000, 0x41100000, 0x41840000, 0x418C0000, 0x41C00000, 0x41C80000],  # 8 9 | 16.5 17.5 | 24 25
                  np.int32)


def test_pack_keypoints_gives_the_literal_buffer():
    packed, b, pool = cp.pack_keypoints(FRAMES, "cpu")
    assert (b, pool) == (2, 6) and packed.dtype == torch.int32 and packed.shape == (40,)
    assert np.array_equal(packed.numpy(), PACKED)
    # non-finite keypoints never pass through an integer: the bits arrive, the integer x, y words stay 0
    nan, _, _ = cp.pack_keypoints([np.array([[np.nan, np.inf, 1]])], "cpu")
    assert nan.numpy().tolist() == [1, 0, 0, 0, 1, 0, 0x7FC00000, 0x7F800000]
    empty, b, pool = cp.pack_keypoints([np.array([])], "cpu")
    assert (b, pool) == (1, 1) and not empty.numpy().any() and empty.shape == (8,)


def test_round_trip_returns_the_id_sorted_input():
    from deepcharuco_amd.inference import unpack_results
    packed, b, pool = cp.pack_keypoints(FRAMES, "cpu")
    counts, starts, rows, xy, conf = cp.views(packed.numpy(), b, pool)
    assert conf is None and counts.tolist() == [3, 3] and starts.tolist() == [0, 3]
    kp, order = cp.frame_keypoints(rows, xy, 0, 3, True)
    assert kp.dtype == np.float64 and np.array_equal(kp, FRAMES[0][[1, 0, 2]]) and order.tolist() == [0, 1, 2]
    res, n = unpack_results(packed.numpy(), b, pool, True)
    assert n.tolist() == [3, 3] and all(r.dtype == np.float64 for r in res)
    assert np.array_equal(res[0], FRAMES[0][[1, 0, 2]]) and np.array_equal(res[1], FRAMES[1])
    ints, _ = unpack_results(packed.numpy(), b, pool, False)             # the integer rows: x = y = 0
    assert ints[0].dtype == np.int64 and np.array_equal(ints[0], [[0, 0, 2], [0, 0, 5], [0, 0, 7]])


def test_pad_packed_moves_each_section_to_the_literal_offsets():
    from deepcharuco_amd.sharding import pad_packed
    packed = torch.arange(1, 23, dtype=torch.int32)                      # batch 2, pool 3: counts 1 2 | starts 3 4 | rows 5..16 | xy 17..22
    assert pad_packed(packed, 2, 3, 2) is packed
    out = pad_packed(packed, 2, 3, 4)
    assert out.dtype == torch.int32 and out.tolist() == [1, 2, 0, 0, 3, 4, 0, 0] + list(range(5, 23))
