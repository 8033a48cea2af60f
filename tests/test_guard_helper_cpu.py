"""The exact guard-zone allocator of the GPU guard tests (tests/guarded_alloc.py), exercised on the CPU: a write of one byte past
either end of a buffer is reported, a write of every byte inside it is not.  This keeps the property the GPU tests rely on -- a
buffer one element too short for what a kernel writes makes them fail -- under test on every machine."""
import pytest

torch = pytest.importorskip("torch")

from tests.guarded_alloc import FILL, GUARD, GuardedAllocator  # noqa: E402

SIZES = [1, 15, 16, 511, 512, 513]
P_PLUS_8 = 12934 + 8     # the 5x5 actor-critic's parameter count + the eight loss sums of ewn_a2c_grad
TYPED = [((3, 5, 5), torch.int8), ((5, 7), torch.float64), ((P_PLUS_8,), torch.float32), ((4, 3, 32), torch.uint8)]


def _cases():
    return [((n,), torch.uint8) for n in SIZES] + TYPED


def _alloc(shape, dtype, offset=0):
    a = GuardedAllocator(device_type="cpu")
    t = a.zeros(shape, dtype=dtype, device="cpu", tag="t", offset=offset)
    return a, t, a.record(t)


@pytest.mark.parametrize("shape,dtype", _cases(), ids=str)
def test_view_is_exact_zeroed_and_aligned(shape, dtype):
    a, t, r = _alloc(shape, dtype)
    assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous()
    assert t.data_ptr() % 16 == 0
    assert r.view_end - r.view_start == t.numel() * t.element_size()
    assert r.view_start >= GUARD and r.parent.numel() - r.view_end >= GUARD
    assert bool((t == 0).all())
    # every byte outside the view is guard: nothing rounds the buffer up
    assert bool((r.parent[:r.view_start] == FILL).all()) and bool((r.parent[r.view_end:] == FILL).all())
    a.check()


@pytest.mark.parametrize("shape,dtype", _cases(), ids=str)
def test_writing_every_byte_of_the_view_is_not_reported(shape, dtype):
    a, t, r = _alloc(shape, dtype)
    t.view(-1).view(torch.uint8).fill_(0xFF)
    assert bool((r.parent[r.view_start:r.view_end] == 0xFF).all())
    a.check()


@pytest.mark.parametrize("shape,dtype", _cases(), ids=str)
@pytest.mark.parametrize("where", ["end", "start-1", "end+4095", "start-4096"])
def test_one_byte_outside_the_view_is_reported(shape, dtype, where):
    a, t, r = _alloc(shape, dtype)
    pos = {"end": r.view_end, "start-1": r.view_start - 1, "end+4095": r.view_end + GUARD - 1, "start-4096": r.view_start - GUARD}[where]
    r.parent[pos] = 0
    with pytest.raises(AssertionError) as ei:
        a.check()
    msg = str(ei.value)
    assert "t shape=%s" % (shape,) in msg and str(dtype) in msg, msg
    if where == "end":
        assert "back guard: first corrupted byte at end+0 (1 bytes)" in msg and "front guard" not in msg, msg
    elif where == "start-1":
        assert "front guard: first corrupted byte at -1 (1 bytes)" in msg and "back guard" not in msg, msg
    elif where == "end+4095":
        assert "end+4095" in msg, msg
    else:
        assert "at -4096" in msg, msg


def test_offset_view_keeps_exact_guards():
    """the misaligned views of the scalar-path tests: one float past a 16-byte boundary, guards directly around it"""
    a, t, r = _alloc((12934,), torch.float32, offset=4)
    assert t.data_ptr() % 16 == 4
    t.fill_(1.0)
    a.check()
    r.parent[r.view_end] = 0
    with pytest.raises(AssertionError, match="back guard"):
        a.check()


def test_patch_guards_zeros_and_zeros_like_and_restores_them():
    a = GuardedAllocator(device_type="cpu")
    real = torch.zeros, torch.zeros_like
    with a.patch(tag="env"):
        x = torch.zeros((4, 3), dtype=torch.float64, device="cpu")
        y = torch.zeros(7, dtype=torch.int8, device=torch.device("cpu"))
        z = torch.zeros_like(x)
        w = torch.zeros(5)                 # no device: left to torch
    assert (torch.zeros, torch.zeros_like) == real
    assert a.owns(x) and a.owns(y) and a.owns(z) and not a.owns(w)
    assert [b.tag for b in a.buffers] == ["env"] * 3
    assert x.shape == (4, 3) and x.dtype == torch.float64 and y.shape == (7,) and z.shape == (4, 3)
    a.record(y).parent[a.record(y).view_end] = 1
    with pytest.raises(AssertionError, match=r"env shape=\(7,\) dtype=torch.int8"):
        a.check("ctx")
