"""Where a call writes and what it reads back: buffers carved out of one patterned allocation, so that a store outside the bytes a
caller owns -- in front of them or behind -- lands in the test's own memory and is seen, and so that the owned bytes can be handed
over holding anything (zeros, or 0xFF bytes: NaN in fp32 and in fp16) to show that a result does not depend on them.

A plain helper module (no fixtures): tests/test_gpu_footprint.py is its user.

    view, h = carve(need, 0xFF, dev)                # `need` bytes of 0xFF between two guards of 1 MiB of 0xA5
    ...the call under test writes through view.data_ptr()...
    assert_guards_intact(h, "workspace")            # names the offset of the first changed guard byte

Offsets are signed distances from the owned region: -k is the k-th byte in front of its first byte, +k the k-th byte behind its
last one.
"""
import contextlib
import math
from unittest import mock

import torch

PATTERN = 0xA5
WS_GUARD = 1 << 20              # bytes on either side of a workspace
FLOAT_GUARD = 4096              # floats on either side of a float tensor (x, y, taps, losses, gradients)


class Carved:
    """One allocation `buf` = guard | owned | guard (bytes); `view` is the owned part as the caller's dtype."""

    def __init__(self, buf, guard, nbytes, view):
        self.buf, self.guard, self.nbytes, self.view = buf, guard, nbytes, view

    def owned_bytes(self):
        return self.buf[self.guard:self.guard + self.nbytes]


def carve(nbytes, fill, dev, guard=WS_GUARD, dtype=torch.uint8):
    """`nbytes` bytes of the byte `fill` between two guards of `guard` bytes of 0xA5, in ONE allocation.  Returns (view, handle):
    the owned bytes as a flat tensor of `dtype`, and what assert_guards_intact / keeps_fill take.  Guards are multiples of 256
    bytes, so the view is aligned as the allocation is (the 16 bytes adn_unet_forward demands of a workspace included)."""
    assert guard > 0 and guard % 256 == 0, "guards are multiples of 256 bytes (alignment of the owned view)"
    item = torch.empty((), dtype=dtype).element_size()
    assert nbytes % item == 0
    buf = torch.full((guard + nbytes + guard,), PATTERN, dtype=torch.uint8, device=dev)
    owned = buf[guard:guard + nbytes]
    owned.fill_(fill)
    view = owned if dtype == torch.uint8 else owned.view(dtype)
    return view, Carved(buf, guard, nbytes, view)


def carve_tensor(shape, fill, dev, dtype=torch.float32, guard_elems=FLOAT_GUARD):
    """A contiguous tensor of `shape` between guards of `guard_elems` elements, every byte of it `fill`."""
    item = torch.empty((), dtype=dtype).element_size()
    view, h = carve(math.prod(shape) * item, fill, dev, guard=guard_elems * item, dtype=dtype)
    h.view = view.reshape(shape)
    return h.view, h


def carve_copy(src, dev, guard_elems=FLOAT_GUARD):
    """`src` (any device) copied between guards on `dev`: an input whose neighbourhood is watched as well."""
    view, h = carve_tensor(tuple(src.shape), 0x00, dev, dtype=src.dtype, guard_elems=guard_elems)
    view.copy_(src)
    return view, h


def first_guard_hit(h):
    """None if both guards still hold 0xA5, else (signed offset, byte found) of the first changed byte, the front guard first."""
    front = h.buf[:h.guard] != PATTERN
    if bool(front.any()):
        i = int(front.nonzero()[0])
        return i - h.guard, int(h.buf[i])
    back = h.buf[h.guard + h.nbytes:] != PATTERN
    if bool(back.any()):
        i = int(back.nonzero()[0])
        return i + 1, int(h.buf[h.guard + h.nbytes + i])
    return None


def assert_guards_intact(h, what):
    hit = first_guard_hit(h)
    if hit is not None:
        off, val = hit
        where = f"{-off} bytes in front of" if off < 0 else f"{off} bytes behind the end of"
        raise AssertionError(f"{what}: guard byte at offset {off:+d} changed from 0xA5 to {val:#04x} ({where} the {h.nbytes} owned bytes)")


def keeps_fill(h, fill):
    """True if every owned byte still holds `fill` (a refused call wrote nothing)."""
    return bool((h.owned_bytes() == fill).all())


@contextlib.contextmanager
def carved_outputs(dev, fill=0xFF, guard_elems=FLOAT_GUARD):
    """While active, every `torch.empty(shape, dtype=torch.float32, device=<the GPU>)` -- how the package's wrappers allocate the
    tensors a library call writes -- is a carved tensor holding `fill` bytes (NaN: an element that is never written shows).  Yields
    the list of handles, in allocation order."""
    made = []
    real = torch.empty

    def empty(*size, **kw):
        device = kw.get("device")
        if kw.get("dtype") is torch.float32 and set(kw) == {"dtype", "device"} and device is not None \
                and torch.device(device).type == dev.type:
            shape = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(size)
            view, h = carve_tensor(shape, fill, torch.device(device), guard_elems=guard_elems)
            made.append(h)
            return view
        return real(*size, **kw)

    with mock.patch.object(torch, "empty", empty):
        yield made
