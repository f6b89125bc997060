"""CPU: tests/memcheck.py held on CPU tensors - the instrument of tests/test_buffer_discipline.py has to be right before
what it reports means anything."""
import math
import struct

import numpy as np
import pytest
import torch

from tests import memcheck as mc

# every dtype the package allocates (a grep of codlad_amd/ for dtype=): fp32 throughout, fp64 in the ensemble metrics and the
# ODE norm, int32 tables, int64 VQ indices and timesteps, uint8 images / flags / state blocks; fp16 is what the split
# modes read fp32 buffers as
DTYPES = (torch.float32, torch.float64, torch.float16, torch.int32, torch.int64, torch.uint8)
SHAPES = ((0,), (1,), (7,), (5, 3), (2, 3, 5), (33, 128))


@pytest.fixture(autouse=True)
def _clean_registry():
    mc.release()
    yield
    mc.release()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fill", mc.FILLS)
def test_shape_contiguity_alignment_dtype(dtype, fill):
    for shape in SHAPES:
        if not dtype.is_floating_point and fill == "nan" and math.prod(shape) == 1:
            continue
        t = mc.guarded(shape, dtype, "cpu", fill)
        assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous() and t.device.type == "cpu"
        assert t.data_ptr() % 16 == 0
        base = t.untyped_storage()
        assert base.nbytes() >= t.numel() * t.element_size() + 2 * mc.ZONE
        assert t.storage_offset() * t.element_size() >= mc.ZONE           # a whole zone before the body ...
        assert base.nbytes() - (t.storage_offset() + t.numel()) * t.element_size() >= mc.ZONE     # ... and one after it
    assert mc.zones_intact()
    assert mc.guarded(4, dtype, "cpu", fill).shape == (4,)                # an int for a shape


def _as(fmt, value, n):
    return struct.unpack("<" + fmt * n, value)


def test_float32_patterns_at_both_widths():
    nan = mc.guarded((6,), torch.float32, "cpu", "nan")
    big = mc.guarded((6,), torch.float32, "cpu", "big")
    assert bool(torch.isnan(nan).all()) and bool(torch.isnan(nan.view(torch.float16)).all())
    assert nan.view(torch.int32).tolist() == [0x7FC07FC0] * 6
    assert bool(torch.isfinite(big).all()) and float(big.min()) > 2.6e36
    assert big.view(torch.float16).tolist() == [65504.0] * 12
    assert mc.guarded((6,), torch.float32, "cpu", "zero").view(torch.int32).tolist() == [0] * 6


def test_float16_and_float64_patterns():
    h_nan, h_big = (mc.guarded((5,), torch.float16, "cpu", f) for f in ("nan", "big"))
    assert bool(torch.isnan(h_nan).all()) and h_nan.view(torch.int16).tolist() == [0x7E00] * 5
    assert h_big.tolist() == [65504.0] * 5
    d_nan, d_big = (mc.guarded((5,), torch.float64, "cpu", f) for f in ("nan", "big"))
    assert bool(torch.isnan(d_nan).all())
    assert bool(torch.isnan(d_nan.view(torch.float32)).all()) and bool(torch.isnan(d_nan.view(torch.float16)).all())
    assert d_big.tolist() == [1e300] * 5
    b_nan, b_big = (mc.guarded((5,), torch.bfloat16, "cpu", f) for f in ("nan", "big"))
    assert bool(torch.isnan(b_nan).all()) and bool(torch.isfinite(b_big).all()) and float(b_big.float().min()) > 3e38


@pytest.mark.parametrize("dtype", (torch.int32, torch.int64, torch.uint8, torch.int16, torch.bool))
def test_integer_buffers_hold_only_zero_one_zero(dtype):
    for fill, want in (("zero", 0), ("nan", 1), ("big", 0)):
        t = mc.guarded((3, 4), dtype, "cpu", fill)
        assert t.to(torch.int64).tolist() == [[want] * 4] * 3


@pytest.mark.parametrize("dtype", (torch.int32, torch.int64, torch.uint8))
def test_a_one_element_integer_buffer_is_not_poisoned_with_one(dtype):
    with pytest.raises(ValueError, match="two entries"):
        mc.guarded((1,), dtype, "cpu", "nan")
    with pytest.raises(ValueError, match="two entries"):
        mc.guarded((), dtype, "cpu", "nan")
    assert mc.guarded((1,), dtype, "cpu", "zero").tolist() == [0]         # 0 is in range of any table
    assert mc.guarded((1,), dtype, "cpu", "big").tolist() == [0]
    assert mc.guarded((0,), dtype, "cpu", "nan").numel() == 0             # nothing to poison
    assert mc.guarded((2,), dtype, "cpu", "nan").tolist() == [1, 1]
    with mc.patched_allocations("nan", "cpu"):
        with pytest.raises(ValueError, match="two entries"):
            torch.empty(1, dtype=dtype)
        assert torch.zeros(1, dtype=dtype).tolist() == [0]                # a written value is no poison


def _raw_of(t):
    """The whole allocation behind a guarded tensor, as bytes, and the body's first byte in it."""
    raw = torch.empty(0, dtype=torch.uint8).set_(t.untyped_storage())
    return raw, t.storage_offset() * t.element_size()


@pytest.mark.parametrize("dtype", (torch.float32, torch.float64, torch.int32, torch.uint8))
def test_a_one_byte_write_in_a_zone_is_found_with_its_offset(dtype):
    t = mc.guarded((5, 3), dtype, "cpu", "nan", name="victim")
    other = mc.guarded((4,), dtype, "cpu", "zero", name="bystander")
    raw, off = _raw_of(t)
    nbytes = t.numel() * t.element_size()
    assert raw.numel() - off - nbytes >= mc.ZONE and off >= mc.ZONE
    first_after, last_after = off + nbytes, raw.numel() - 1
    for pos, side in ((0, "before"), (off - 1, "before"), (first_after, "after"), (last_after, "after")):
        assert mc.zones_intact()
        keep = int(raw[pos])
        assert keep == mc.ZONE_BYTE
        raw[pos] = 0
        found = mc.zone_violations()
        assert found == [("victim", side, pos - off, 0, 1)], (pos, found)
        with pytest.raises(AssertionError, match=rf"victim: 1 byte\(s\) {side} the body, first at body offset \{pos - off:+d}"):
            mc.zones_intact()
        raw[pos] = keep
    assert mc.zones_intact()
    del other


def test_a_write_inside_the_body_is_not_reported():
    t = mc.guarded((7, 3), torch.float32, "cpu", "nan")
    t.fill_(3.0)
    t.view(torch.uint8)[0] = 1
    t.view(torch.uint8)[-1] = 1
    assert mc.zones_intact() and mc.zone_violations() == []
    z = mc.guarded((0,), torch.float32, "cpu", "nan")                     # an empty body between two whole zones
    assert z.numel() == 0 and mc.zones_intact()


def test_patch_forms_and_values():
    x = torch.arange(6, dtype=torch.float32).reshape(2, 3)
    n0 = mc.registered()
    with mc.patched_allocations("nan", devices=["cpu"]):
        a = torch.empty(2, 3)
        b = torch.empty((2, 3), dtype=torch.float64)
        c = torch.empty_like(x)
        d = torch.zeros(4, dtype=torch.int32)
        e = torch.zeros_like(x)
        f = torch.empty(size=(3,), dtype=torch.int64, device="cpu")
        g = torch.ones(3)
        h = torch.full((2, 2), -1, dtype=torch.int32)
        i = x.new_empty(5)
        j = x.new_zeros((2, 2))
        k = torch.empty_like(x, dtype=torch.int32)
        m = torch.full((2,), 2.5)
        assert mc.registered() == n0 + 12
    assert bool(torch.isnan(a).all()) and a.shape == (2, 3) and a.dtype == torch.float32
    assert bool(torch.isnan(b).all()) and b.dtype == torch.float64
    assert bool(torch.isnan(c).all()) and c.shape == x.shape
    assert d.tolist() == [0] * 4 and e.tolist() == [[0.0] * 3] * 2 and f.tolist() == [1, 1, 1]
    assert g.tolist() == [1.0] * 3 and h.tolist() == [[-1, -1]] * 2 and h.dtype == torch.int32
    assert bool(torch.isnan(i).all()) and i.shape == (5,) and j.tolist() == [[0.0, 0.0]] * 2
    assert k.tolist() == [[1] * 3] * 2 and m.tolist() == [2.5, 2.5]
    for t in (a, b, c, d, e, f, g, h, i, j, k, m):
        assert t.is_contiguous() and t.data_ptr() % 16 == 0 and t.untyped_storage().nbytes() >= 2 * mc.ZONE
    assert mc.zones_intact()
    with mc.patched_allocations("big", "cpu"):
        assert torch.empty(3).view(torch.int32).tolist() == [0x7BFF7BFF] * 3
    with mc.patched_allocations("zero", "cpu"):
        assert torch.empty(3).tolist() == [0.0] * 3
    # the package's results do not change type or shape under the patch: the same forms unpatched
    assert torch.empty(2, 3).shape == a.shape and torch.full((2, 2), -1, dtype=torch.int32).dtype == h.dtype


def test_the_patch_is_undone_after_an_exception():
    before = {n: getattr(torch, n) for n in ("empty", "empty_like", "zeros", "zeros_like", "ones", "full")}
    methods = {n: getattr(torch.Tensor, n) for n in ("new_empty", "new_zeros")}
    with pytest.raises(RuntimeError, match="boom"):
        with mc.patched_allocations("nan", "cpu"):
            assert torch.empty is not before["empty"]
            raise RuntimeError("boom")
    assert all(getattr(torch, n) is f for n, f in before.items())
    assert all(getattr(torch.Tensor, n) is f for n, f in methods.items())
    assert torch.empty(3).untyped_storage().nbytes() < mc.ZONE
    with pytest.raises(ValueError):
        with mc.patched_allocations("stale", "cpu"):
            pass
    assert torch.empty is before["empty"]


def test_a_cpu_tensor_under_a_cuda_only_patch_is_an_ordinary_one():
    n0 = mc.registered()
    with mc.patched_allocations("nan", devices=["cuda"]):
        a = torch.empty(5)
        b = torch.zeros(5, device="cpu")
        c = torch.empty_like(a)
        d = np.zeros(3)
    assert mc.registered() == n0
    for t in (a, b, c):
        assert t.device.type == "cpu" and t.untyped_storage().nbytes() == 20
    assert b.tolist() == [0.0] * 5 and d.tolist() == [0.0] * 3


def test_same_bits():
    nan = torch.tensor([1.0, float("nan"), -0.0])
    assert mc.same_bits(nan, nan.clone()) and not torch.equal(nan, nan.clone())
    assert not mc.same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))            # equal values, other bits
    other = nan.clone()
    other.view(torch.int32)[1] += 1                                                # another NaN payload
    assert not mc.same_bits(nan, other)
    assert not mc.same_bits(nan, nan.double()) and not mc.same_bits(nan, nan[:2])
    assert mc.same_bits(torch.tensor([1, 2]), torch.tensor([1, 2])) and not mc.same_bits(torch.tensor([1, 2]), torch.tensor([1, 3]))
    d = torch.tensor([float("nan"), 2.0], dtype=torch.float64)
    assert mc.same_bits(d, d.clone()) and mc.same_bits(nan[::2], nan[::2].clone())
