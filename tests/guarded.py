"""Guarded arenas: a buffer of EXACTLY ``nbytes`` bytes at a chosen alignment inside one larger tensor, with a guard region in
front of it and one behind it.  What the C ABI promises about memory -- a call writes nothing outside its workspace and its output
buffers, and what a workspace held at entry does not matter -- is checked by handing the entries such buffers: the guards show a
store on either side, an exact-size body leaves no slack for one to hide in, and the body can be poisoned with any byte pattern.

Plain helper module: no fixtures.  Works on CPU tensors (tests/test_guarded_host.py tests the checker itself there) and on device
tensors alike.

    a = Arena(nbytes, dev)                       # 256-byte aligned, zero body, 4 KiB guards of 0xC3
    a = Arena(nbytes, dev, align=16, offset=8)   # address = 8 (mod 16): 8-byte aligned, not 16-byte aligned
    a.fill_body(b"\\xff")                         # a byte pattern, tiled from the buffer's first byte on
    lib.dcx_...(a.ptr, a.nbytes, ...)
    assert a.guards_ok() is None                 # else: the first damaged offset relative to the buffer (negative: front guard)
"""
import numpy as np
import torch

GUARD_BYTES = 4096
GUARD_FILL = b"\xc3"


def pattern_bytes(pattern):
    """A fill given as bytes, an int (one byte) or a numpy scalar / array (its bytes) -> a non-empty ``bytes``."""
    if isinstance(pattern, (bytes, bytearray)):
        out = bytes(pattern)
    elif isinstance(pattern, int):
        out = bytes([pattern])
    else:
        out = np.ascontiguousarray(pattern).tobytes()
    if not out:
        raise ValueError("an empty fill pattern")
    return out


def element_bytes(value, dtype):
    """One element ``value`` of a torch ``dtype`` as a byte pattern (the sentinel of an output buffer)."""
    return torch.tensor([value], dtype=dtype).numpy().tobytes()


def _tiled(pattern, first, n, device):
    """``n`` bytes of ``pattern`` tiled over the whole line of addresses, beginning with the byte at position ``first`` (which may be
    negative: the front guard continues the phase of the buffer)."""
    p = np.frombuffer(pattern_bytes(pattern), np.uint8)
    if len(p) == 1:
        return torch.full((n,), int(p[0]), dtype=torch.uint8, device=device)
    return torch.from_numpy(np.resize(np.roll(p, -(first % len(p))), n)).to(device)


class Arena:
    """``nbytes`` bytes whose address is ``offset`` modulo ``align``, between two guards of at least ``guard`` bytes each.

    ``body`` and ``guards`` are byte patterns and are filled independently; both are tiled from the buffer's first byte, so a
    pattern of one element's bytes reproduces that element through a view of the element's dtype."""

    def __init__(self, nbytes, device="cpu", align=256, offset=0, guard=GUARD_BYTES, body=b"\x00", guards=GUARD_FILL):
        if nbytes < 0 or align < 1 or not 0 <= offset < align or guard < GUARD_BYTES:
            raise ValueError("nbytes >= 0, align >= 1, 0 <= offset < align, guard >= 4096")
        self.nbytes, self.align, self.offset, self.guard = int(nbytes), int(align), int(offset), int(guard)
        self.full = torch.empty(self.guard + self.align + self.nbytes + self.guard, dtype=torch.uint8, device=device)
        base = self.full.data_ptr()
        self.start = self.guard + (self.offset - (base + self.guard)) % self.align
        assert (base + self.start) % self.align == self.offset and self.start >= self.guard
        self.end = self.start + self.nbytes                      # the back guard is full[end:], at least ``guard`` bytes
        self.body = self.full[self.start:self.end]
        self._guards = pattern_bytes(guards)
        self._body = pattern_bytes(body)
        self.fill_guards(guards)
        self.fill_body(body)

    # ---- addresses and views
    @property
    def ptr(self):
        return self.full.data_ptr() + self.start

    @property
    def device(self):
        return self.full.device

    def view(self, dtype, *shape):
        """The buffer as ``dtype`` (and ``shape``); the address must be a multiple of the element size."""
        size = torch.empty(0, dtype=dtype).element_size()
        if self.ptr % size or self.start % size or self.nbytes % size:
            raise ValueError(f"a buffer of {self.nbytes} bytes at {self.ptr % self.align} mod {self.align} has no {dtype} view")
        v = self.body.view(dtype)
        return v.view(*shape) if shape else v

    # ---- fills
    def fill_body(self, pattern):
        self._body = pattern_bytes(pattern)
        if self.nbytes:
            self.body.copy_(_tiled(self._body, 0, self.nbytes, self.device))

    def fill_guards(self, pattern):
        self._guards = pattern_bytes(pattern)
        self.full[:self.start].copy_(_tiled(self._guards, -self.start, self.start, self.device))
        back = self.full.numel() - self.end
        self.full[self.end:].copy_(_tiled(self._guards, self.nbytes, back, self.device))

    def refill(self):
        self.fill_guards(self._guards)
        self.fill_body(self._body)

    # ---- checks
    def guards_ok(self):
        """None while both guards hold their fill; else the offset, relative to the buffer, of the first damaged byte: negative in
        the front guard (-1 is the byte in front of the buffer), ``nbytes`` or more in the back guard."""
        front = self.full[:self.start] != _tiled(self._guards, -self.start, self.start, self.device)
        if bool(front.any()):
            return int(torch.nonzero(front)[0, 0]) - self.start
        back_len = self.full.numel() - self.end
        back = self.full[self.end:] != _tiled(self._guards, self.nbytes, back_len, self.device)
        if bool(back.any()):
            return int(torch.nonzero(back)[0, 0]) + self.nbytes
        return None

    def changed(self):
        """A bool tensor over the buffer's bytes: True where a byte no longer holds the body's fill."""
        return self.body != _tiled(self._body, 0, self.nbytes, self.device)

    def untouched(self, where=slice(None), dtype=torch.uint8):
        """Do the elements (of ``dtype``) that ``where`` -- a slice, an index or a bool mask over the buffer's ``dtype`` view --
        selects still hold the body's fill?  For the places where the header says a word is not written."""
        size = torch.empty(0, dtype=dtype).element_size()
        if self.nbytes % size:
            raise ValueError("the buffer is no whole number of such elements")
        diff = self.changed().view(-1, size).any(dim=1)
        if isinstance(where, np.ndarray):
            where = torch.from_numpy(where)
        if isinstance(where, torch.Tensor):
            where = where.to(self.device).reshape(-1)
        return not bool(diff[where].any())


class Guarded(Arena):
    """An output buffer of ``shape`` elements of ``dtype`` prefilled with the sentinel ``fill``, guards of the same sentinel on
    both sides: ``.t`` is the tensor, ``.ptr`` its address."""

    def __init__(self, dev, shape, dtype, fill, align=256, offset=0):
        self.n = int(np.prod(shape)) if len(shape) else 1
        self.fill = fill
        pat = element_bytes(fill, dtype)
        super().__init__(self.n * len(pat), dev, align=align, offset=offset, body=pat, guards=pat)
        self.t = self.view(dtype, *shape) if len(shape) else self.view(dtype)

    def guard_ok(self):
        return self.guards_ok() is None

    def cpu(self):
        return self.t.cpu().numpy()
