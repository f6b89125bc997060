"""Red zones and poison for the buffers a kernel is handed: the instrument of tests/test_buffer_discipline.py.

A kernel here can be wrong in two ways that no parity test sees: it reads a slot that nothing has written (the memory
of a test box is zeros or finite leftovers, so the result is right by luck), or it writes a byte that is not its own
(a few rows past the end land in the caching allocator's slack).  `guarded` makes both visible without a sanitizer:

  body    filled with "zero", "nan" or "big".  A result that depends on an unwritten slot has different bits under
          the three fills, and NaN under the second.
  zones   ZONE bytes of ZONE_BYTE on either side of the body, inside the same allocation: an overrun of up to one
          node's edge block (32 KiB) or one 32-node tile of 128-float rows (16 KiB) changes zone bytes and stays
          inside the allocation.  `zones_intact` names the buffer and the byte offset.

Floating types get a pattern that is NaN (or large and finite) under every width a kernel may read it at; integer and
byte buffers get 0 / 1 / 0 only, so that a stale INDEX is another valid element (different bits) and never a fault:
every indexed table of a case has two entries or more, and `guarded` refuses to poison a one-element integer buffer
with 1.

`patched_allocations` puts guarded tensors under torch.empty / empty_like / zeros / zeros_like / ones / full (and
Tensor.new_empty / new_zeros) for the named devices, so the package's own allocations come poisoned.  This module
imports nothing from the package and is no conftest: a test imports it by name.
"""
import contextlib

import torch

ZONE = 64 * 1024
ZONE_BYTE = 0xA5
ALIGN = 16
FILLS = ("zero", "nan", "big")

# dtype -> (integer view of the same width, the "nan" pattern, the "big" pattern); None: fill_ with the float below
_FLOAT_PATTERNS = {
    torch.float32: (torch.int32, 0x7FC07FC0, 0x7BFF7BFF),     # NaN as one float and as two halves | 2.7e36, 65504 twice
    torch.float16: (torch.int16, 0x7E00, 0x7BFF),             # NaN | 65504
    torch.bfloat16: (torch.int16, 0x7FC0, 0x7F7F),            # NaN | 3.4e38
    torch.float64: (torch.int64, 0x7FF87FF87FF87FF8, None),   # NaN as a double, as two floats and as four halves | 1e300
}
BIG_F64 = 1e300
INT_POISON = {"zero": 0, "nan": 1, "big": 0}
INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}

_NAMES = ("empty", "empty_like", "zeros", "zeros_like", "ones", "full")
_ORIG = {n: getattr(torch, n) for n in _NAMES}
_ORIG_METHODS = {n: getattr(torch.Tensor, n) for n in ("new_empty", "new_zeros")}

_registry = []      # [name, raw uint8 allocation, body offset, body bytes]: strong references, so that a guarded block is
#                     never handed out again (and its zones rewritten) before zones_intact() has looked at it


def _itemsize(dtype):
    return _ORIG["empty"](0, dtype=dtype).element_size()


def guarded(shape, dtype=torch.float32, device="cpu", fill="nan", name=None):
    """A contiguous `dtype` tensor of `shape` on `device`: a view into a larger uint8 allocation, its first byte on a
    16-byte boundary, ZONE bytes of ZONE_BYTE before and after it, the body filled by `fill` ("zero", "nan", "big")."""
    if fill not in FILLS:
        raise ValueError(f"fill must be one of {FILLS}, got {fill!r}")
    if dtype.is_complex:
        raise TypeError("no poison pattern for complex types")
    shape = tuple(int(s) for s in ((shape,) if isinstance(shape, int) else shape))
    numel = 1
    for s in shape:
        numel *= s
    integer = dtype not in _FLOAT_PATTERNS
    if integer and dtype.is_floating_point:
        raise TypeError(f"no poison pattern for {dtype}")
    if integer and INT_POISON[fill] == 1 and numel == 1:
        raise ValueError(f"a one-element {dtype} buffer is not poisoned with 1: as an index it would need a table of two "
                         "entries, which nothing guarantees (keep every indexed table of a case at two entries or more)")
    nbytes = numel * _itemsize(dtype)
    raw = _ORIG["empty"](ZONE + ALIGN + nbytes + ZONE, dtype=torch.uint8, device=device)
    raw.fill_(ZONE_BYTE)
    off = ZONE + (-(raw.data_ptr() + ZONE)) % ALIGN
    body = raw[off:off + nbytes]
    assert body.data_ptr() % ALIGN == 0 and off + nbytes + ZONE <= raw.numel()
    if numel:
        if integer:
            body.view(dtype).fill_(INT_POISON[fill])
        elif fill == "zero":
            body.zero_()
        else:
            view, nan, big = _FLOAT_PATTERNS[dtype]
            if fill == "big" and big is None:
                body.view(dtype).fill_(BIG_F64)
            else:
                body.view(view).fill_(nan if fill == "nan" else big)
    t = body.view(dtype).view(shape)
    _registry.append([name or f"#{len(_registry)} {str(dtype).replace('torch.', '')}{list(shape)}", raw, off, nbytes])
    return t


def guard_copy(src, fill="nan", name=None, device=None):
    """A guarded tensor with the values of `src` (an input of the caller's: the body is all written)."""
    t = guarded(tuple(src.shape), src.dtype, device or src.device, "zero" if src.numel() == 1 else fill, name)
    t.copy_(src)
    return t


def zone_violations():
    """Every changed zone byte's buffer -> [(name, "before" | "after", offset of the first changed byte relative to the
    body's first byte (negative: before it), its value, the number of changed bytes on that side)]."""
    found = []
    pending = []
    for name, raw, off, nbytes in _registry:
        lo, hi = raw[:off], raw[off + nbytes:]
        pending.append((name, raw, off, nbytes, (lo != ZONE_BYTE).sum(), (hi != ZONE_BYTE).sum()))
    for name, raw, off, nbytes, n_lo, n_hi in pending:
        for side, n, start in (("before", int(n_lo), 0), ("after", int(n_hi), off + nbytes)):
            if n:
                zone = raw[:off] if side == "before" else raw[off + nbytes:]
                first = int((zone != ZONE_BYTE).nonzero()[0])
                found.append((name, side, start + first - off, int(zone[first]), n))
    return found


def zones_intact():
    """True, or an AssertionError that names every buffer with a changed zone byte and the byte's offset."""
    found = zone_violations()
    if found:
        raise AssertionError("write outside a buffer: " + "; ".join(
            f"{name}: {n} byte(s) {side} the body, first at body offset {o:+d} (value {v:#04x})" for name, side, o, v, n in found))
    return True


def release():
    """Forget every registered allocation (after zones_intact(): the memory goes back to the allocator)."""
    del _registry[:]


def registered():
    return len(_registry)


# ------------------------------------------------------------------------------------------------- the patch --
def _wanted(device, devices):
    d = torch.device(device)
    for w in devices:
        w = torch.device(w)
        if d.type == w.type and (w.index is None or d.index is None or d.index == w.index):
            return True
    return False


def _size_of(args, kwargs):
    if "size" in kwargs:
        return kwargs.pop("size"), ()
    if len(args) == 1 and not isinstance(args[0], int):
        return tuple(args[0]), ()
    return tuple(args), ()


_PASS = ("out", "layout", "pin_memory", "names")


def _plain(kwargs):
    """The keyword arguments that the guarded forms understand (anything else goes to the original function)."""
    if any(kwargs.get(k) not in (None, False, torch.strided) for k in _PASS):
        return False
    mf = kwargs.get("memory_format")
    return mf in (None, torch.contiguous_format, torch.preserve_format)


def _default_device():
    return _ORIG["empty"](0).device


def _make(fill, devices, shape, dtype, device, kwargs, value=None):
    t = guarded(shape, dtype, device, fill if value is None else "zero")
    if value is not None and value != 0:
        t.fill_(value)
    if kwargs.get("requires_grad"):
        t.requires_grad_(True)
    return t


@contextlib.contextmanager
def patched_allocations(fill, devices=("cuda",)):
    """torch.empty / empty_like on `devices` return guarded tensors filled by `fill`; zeros / zeros_like / ones / full (and
    Tensor.new_empty / new_zeros) come with their value and with zones.  Other devices, and forms that ask for an `out`,
    a layout, pinned memory or a channels-last format, go to the original functions.  Everything is restored on exit."""
    if fill not in FILLS:
        raise ValueError(f"fill must be one of {FILLS}, got {fill!r}")
    devices = (devices,) if isinstance(devices, (str, torch.device)) else tuple(devices)

    def sized(name, value):
        orig = _ORIG[name]

        def f(*args, **kwargs):
            kw = dict(kwargs)
            if name == "full":
                if "fill_value" in kw:
                    val = kw.pop("fill_value")
                    shape = kw.pop("size") if "size" in kw else args[0]
                else:
                    shape, val = (kw.pop("size"), args[0]) if "size" in kw else (args[0], args[1])
                shape = tuple(shape)
            else:
                shape, _ = _size_of(args, kw)
                val = value
            device = kw.get("device")
            device = _default_device() if device is None else device
            if not _wanted(device, devices) or not _plain(kw) or isinstance(val, torch.Tensor):
                return orig(*args, **kwargs)
            dtype = kw.get("dtype")
            if dtype is None:
                dtype = torch.get_default_dtype()
                if name == "full" and not isinstance(val, float):
                    dtype = torch.bool if isinstance(val, bool) else torch.int64 if isinstance(val, int) else dtype
            return _make(fill, devices, shape, dtype, device, kw, val)
        return f

    def like(name, value):
        orig = _ORIG[name]

        def f(t, **kwargs):
            device = kwargs.get("device") or t.device
            if not _wanted(device, devices) or not _plain(kwargs) or t.layout != torch.strided:
                return orig(t, **kwargs)
            return _make(fill, devices, tuple(t.shape), kwargs.get("dtype") or t.dtype, device, kwargs, value)
        return f

    def method(name, value):
        orig = _ORIG_METHODS[name]

        def f(self, *args, **kwargs):
            kw = dict(kwargs)
            shape, _ = _size_of(args, kw)
            device = kw.get("device") or self.device
            if not _wanted(device, devices) or not _plain(kw):
                return orig(self, *args, **kwargs)
            return _make(fill, devices, shape, kw.get("dtype") or self.dtype, device, kw, value)
        return f

    new = {"empty": sized("empty", None), "zeros": sized("zeros", 0), "ones": sized("ones", 1), "full": sized("full", None),
           "empty_like": like("empty_like", None), "zeros_like": like("zeros_like", 0)}
    new_methods = {"new_empty": method("new_empty", None), "new_zeros": method("new_zeros", 0)}
    try:
        for n, f in new.items():
            setattr(torch, n, f)
        for n, f in new_methods.items():
            setattr(torch.Tensor, n, f)
        yield
    finally:
        for n, f in _ORIG.items():
            setattr(torch, n, f)
        for n, f in _ORIG_METHODS.items():
            setattr(torch.Tensor, n, f)


# ------------------------------------------------------------------------------------------------ comparison --
def same_bits(a, b):
    """a and b have the same shape, type and bits (through an integer view: NaN equals NaN of the same payload)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.bool or not (a.dtype.is_floating_point or a.dtype.is_complex):
        return bool(torch.equal(a, b.to(a.device)))
    view = INT_VIEW[a.element_size()]
    return bool(torch.equal(a.contiguous().view(view), b.to(a.device).contiguous().view(view)))
