"""CPU: the guard checker of tests/guarded.py checks what it says -- a byte written just outside the buffer, or at the far end of
either guard, is reported at its offset; a byte written at the buffer's first or last byte is not; the address has the alignment
asked for; a byte pattern reproduces its element through every dtype view."""
import numpy as np
import pytest
import torch

from guarded import GUARD_BYTES, Arena, Guarded, element_bytes, pattern_bytes

SIZES = [1, 8, 24, 1000, 4096, 70001]


def _poke(a, offset):
    """Flip one byte at ``offset`` relative to the buffer."""
    a.full[a.start + offset] ^= 0x5A


@pytest.mark.parametrize("nbytes", SIZES)
@pytest.mark.parametrize("guards", [b"\xc3", b"\x00", element_bytes(-12345.5, torch.float32), element_bytes(-7, torch.int32)],
                         ids=["c3", "zero", "f32", "i32"])
def test_one_damaged_guard_byte_is_reported_at_its_offset(nbytes, guards):
    a = Arena(nbytes, guards=guards)
    assert a.guards_ok() is None
    front, back = a.start, a.full.numel() - a.end
    assert front >= GUARD_BYTES and back >= GUARD_BYTES
    for offset in (-1, nbytes, -GUARD_BYTES, nbytes + GUARD_BYTES - 1, -front, nbytes + back - 1):
        _poke(a, offset)
        assert a.guards_ok() == offset
        _poke(a, offset)
        assert a.guards_ok() is None
    _poke(a, -1)                  # damage on both sides: the first in address order
    _poke(a, nbytes)
    assert a.guards_ok() == -1
    a.fill_guards(guards)
    assert a.guards_ok() is None


@pytest.mark.parametrize("nbytes", SIZES)
def test_writes_inside_the_buffer_are_not_reported(nbytes):
    a = Arena(nbytes, body=b"\x7f")
    _poke(a, 0)
    _poke(a, nbytes - 1)
    assert a.guards_ok() is None
    a.body.fill_(0)
    assert a.guards_ok() is None
    assert a.body.numel() == nbytes and a.ptr == a.body.data_ptr()


def test_a_zero_byte_buffer_still_has_both_guards():
    a = Arena(0)
    assert a.guards_ok() is None and a.body.numel() == 0
    _poke(a, 0)                                   # the first byte of the back guard
    assert a.guards_ok() == 0


@pytest.mark.parametrize("align,offset", [(256, 0), (8, 0), (16, 8), (8, 4), (256, 1), (256, 255), (4096, 0), (64, 13)])
def test_alignment_requests_are_honoured(align, offset):
    for nbytes in (24, 1001):
        a = Arena(nbytes, align=align, offset=offset)
        assert a.ptr % align == offset
        assert a.start >= GUARD_BYTES and a.full.numel() - a.end >= GUARD_BYTES
        assert a.guards_ok() is None
    a = Arena(24, align=16, offset=8)             # 8-byte aligned and not 16-byte aligned
    assert a.ptr % 8 == 0 and a.ptr % 16 == 8
    assert a.view(torch.float64).shape == (3,)
    with pytest.raises(ValueError):
        Arena(24, align=8, offset=4).view(torch.float64)
    assert Arena(24, align=8, offset=4).view(torch.float32).shape == (6,)
    with pytest.raises(ValueError):
        Arena(8, align=8, offset=8)
    with pytest.raises(ValueError):
        Arena(8, guard=GUARD_BYTES - 1)


VIEWS = [(torch.uint8, np.uint8), (torch.int16, np.int16), (torch.int32, np.int32), (torch.float32, np.float32),
         (torch.float64, np.float64)]


@pytest.mark.parametrize("tdtype,ndtype", VIEWS, ids=[str(n.__name__) for _, n in VIEWS])
def test_byte_patterns_reproduce_through_every_dtype_view(tdtype, ndtype):
    size = np.dtype(ndtype).itemsize
    # one element's bytes give that element everywhere, whatever the value
    for value in (0, 1, -7 if ndtype is not np.uint8 else 249, 12345 % 256 if ndtype is np.uint8 else 12345):
        pat = np.array(value, ndtype).tobytes()
        assert pat == element_bytes(value, tdtype)
        a = Arena(40 * size, body=pat)
        got = a.view(tdtype).numpy()
        assert got.dtype == ndtype and got.shape == (40,) and np.all(got == np.array(value, ndtype))
        assert a.untouched() and a.untouched(dtype=tdtype)
    # the four poison patterns read as the header's numbers
    for byte, check in ((0x00, lambda v: np.all(v == 0)), (0x7F, None), (0xFF, None)):
        a = Arena(16 * size, body=bytes([byte]))
        v = a.view(tdtype).numpy()
        assert v.tobytes() == bytes([byte]) * (16 * size)
        if ndtype is np.float32 and byte == 0x7F:
            assert np.all(np.isfinite(v)) and np.all(v > 3.3e38)
        if ndtype is np.float64 and byte == 0x7F:
            assert np.all(np.isfinite(v)) and np.all(v > 1.3e306)
        if ndtype in (np.float32, np.float64) and byte == 0xFF:
            assert np.all(np.isnan(v))
        if ndtype in (np.int16, np.int32) and byte == 0xFF:
            assert np.all(v == -1)
    # a pattern longer than an element keeps its phase from the buffer's first byte on, in the body and in both guards
    pat = bytes(range(1, 13))
    a = Arena(5 * 12, body=pat, guards=pat)
    whole = a.full.numpy()
    for i in (-a.start, -13, -1, 0, 1, 59, 60, 61, a.full.numel() - a.start - 1):
        assert whole[a.start + i] == pat[i % 12], i


def test_untouched_selects_by_slice_index_and_mask():
    a = Arena(64, body=element_bytes(-7, torch.int32))
    v = a.view(torch.int32)
    assert a.untouched(dtype=torch.int32)
    v[5] = 0
    v[9] = -7                                      # the sentinel written again is not a change
    assert not a.untouched(dtype=torch.int32) and not a.untouched()
    assert a.untouched(slice(0, 5), torch.int32) and a.untouched(slice(6, None), torch.int32)
    assert not a.untouched(slice(5, 6), torch.int32) and not a.untouched(5, torch.int32)
    mask = np.ones(16, bool)
    mask[5] = False
    assert a.untouched(mask, torch.int32) and a.untouched(torch.from_numpy(mask), torch.int32)
    assert not a.untouched(~mask, torch.int32)
    assert a.untouched(slice(0, 20)) and not a.untouched(slice(20, 24))      # bytes 20..23 are element 5
    assert int(a.changed().sum()) == 4             # -7 = f9 ff ff ff -> 0: every byte of element 5 differs
    v[0] = -8                                      # f8 ff ff ff: one byte
    assert int(a.changed().sum()) == 5
    a.refill()
    assert a.untouched() and a.guards_ok() is None


def test_guarded_output_buffer_keeps_the_staged_tests_interface():
    g = Guarded("cpu", (3, 4), torch.float32, -12345.5)
    assert g.t.shape == (3, 4) and g.n == 12 and g.ptr == g.t.data_ptr() and g.ptr % 256 == 0
    assert np.all(g.cpu() == np.float32(-12345.5)) and g.guard_ok()
    g.t[2, 3] = 1.0
    assert g.guard_ok()
    g.full[g.end] ^= 1
    assert not g.guard_ok() and g.guards_ok() == g.nbytes
    g.refill()
    assert g.guard_ok() and np.all(g.cpu() == np.float32(-12345.5))
    g.full[g.start - 1] ^= 1                      # in front of the buffer, which the staged tests' own class could not see
    assert not g.guard_ok() and g.guards_ok() == -1
    one = Guarded("cpu", (1,), torch.int32, -7)
    assert one.cpu().tolist() == [-7]


def test_pattern_bytes_forms():
    assert pattern_bytes(0xA5) == b"\xa5" and pattern_bytes(b"\x01\x02") == b"\x01\x02"
    assert pattern_bytes(np.float32(1.0)) == np.float32(1.0).tobytes()
    assert pattern_bytes(np.arange(3, dtype=np.int16)) == np.arange(3, dtype=np.int16).tobytes()
    with pytest.raises(ValueError):
        pattern_bytes(b"")
