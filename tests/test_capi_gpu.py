"""The two views of libngp_amd.so on the device: a call through the checked
view with tensors launches what the raw view launches with hand-made
pointers, and a tensor the header's pointee type does not allow never
reaches the kernel (capi.POINTER_TO, vren.kernels)."""
import ctypes

import pytest
import torch

import vren

pytestmark = pytest.mark.gpu


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def test_checked_view_with_tensors_equals_raw_view_with_pointers():
    L, K = vren.lib(), vren.kernels()
    hits = L.ngp_guard_hits()
    coords = torch.randint(0, 128, (64, 3), dtype=torch.int32, generator=torch.Generator().manual_seed(3)).cuda()
    raw, chk = (torch.full((64,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    assert L.ngp_morton3d(_p(coords), 64, _p(raw), vren._stream()) == 0
    assert K.ngp_morton3d(coords, 64, chk, vren._stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(raw, chk) and int(raw.min()) >= 0 and raw.unique().numel() > 1
    # an int64 tensor where the header says float*, and a strided view: refused before the launch
    grid, bits = torch.zeros(64, device="cuda"), torch.zeros(8, dtype=torch.uint8, device="cuda")
    with pytest.raises(ctypes.ArgumentError, match="torch.float32.*torch.int64"):
        K.ngp_packbits(grid.long(), 8, 0.5, None, bits, vren._stream())
    with pytest.raises(ctypes.ArgumentError, match="contiguous"):
        K.ngp_packbits(torch.zeros(128, device="cuda")[::2], 8, 0.5, None, bits, vren._stream())
    with pytest.raises(ctypes.ArgumentError, match="contiguous"):
        K.ngp_morton3d(coords.t(), 64, chk, vren._stream())
    K.ngp_packbits(grid, 8, 0.5, None, bits, vren._stream())  # (the same call with what the header asks for)
    torch.cuda.synchronize()
    assert int(bits.sum()) == 0 and L.ngp_guard_hits() == hits
