"""Host side of the region encoder's native backward: the workspace query and the argument checks of the three entry points run
without a device (a refused call launches nothing), and the test inputs' construction is what the GPU tests' bounds assume."""
import ctypes

import pytest
import torch

import region_train_inputs as RT
from visionllm_amd import _lib
from visionllm_amd import region_encoder as A


def _err():
    return _lib.lib().vllm_last_error().decode()


def test_backward_entry_points_are_declared_and_exported():
    protos = _lib.parse_header()
    for name in ("vllm_point_sample_backward_workspace_bytes", "vllm_point_sample_mean_backward_f32",
                 "vllm_point_sample_mean_backward_bf16", "vllm_point_sample_backward_f32"):
        assert name in protos and hasattr(_lib.lib(), name), name
    assert protos["vllm_point_sample_backward_workspace_bytes"][0] is ctypes.c_long
    assert len(protos["vllm_point_sample_mean_backward_f32"][1]) == 12 and len(protos["vllm_point_sample_backward_f32"][1]) == 11
    assert _lib.header_abi_version() == 2


def test_workspace_query_is_a_host_function():
    L = _lib.lib()
    for shape in [(16, 3072, 24, 24, 2304), (16, 384, 24, 24, 2304), (3, 100, 5, 7, 300), (1, 3, 1, 1, 7), (3, 8, 6, 4, 0), (0, 8, 80, 80, 5)]:
        assert L.vllm_point_sample_backward_workspace_bytes(*shape) == 0, shape        # the accumulators fit on chip
    assert L.vllm_point_sample_backward_workspace_bytes(2, 9, 80, 80, 500) >= 2 * 80 * 80 * 8
    assert L.vllm_point_sample_backward_workspace_bytes(5, 1, 300, 200, 0) >= 5 * 300 * 200 * 8
    assert L.vllm_point_sample_backward_workspace_bytes(2, 0, 80, 80, 5) == -1 and "bad sizes" in _err()


def test_entry_points_refuse_bad_arguments_without_a_device():
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)
    mean = [L.vllm_point_sample_mean_backward_f32, L.vllm_point_sample_mean_backward_bf16]
    for fn in mean:
        assert fn(odd, p, p, 1, 3, 4, 4, 5, p, None, 0, None) == -1 and "coords must be 8-byte aligned" in _err()
        assert fn(p, p, p, 65536, 3, 4, 4, 5, p, None, 0, None) == -1 and "too many regions / too large a map for one launch" in _err()
        assert fn(p, p, p, 1, 3, 4096, 4096, 5, p, None, 0, None) == -1 and "too large a map" in _err()
        assert fn(p, p, p, 1, 0, 4, 4, 5, p, None, 0, None) == -1 and "bad sizes" in _err()
        assert fn(p, p, None, 1, 3, 4, 4, 5, p, None, 0, None) == -1 and "null pointer" in _err()
        assert fn(p, None, p, 1, 3, 4, 4, 5, p, None, 0, None) == -1 and "null pointer" in _err()
        assert fn(p, p, p, 2, 9, 80, 80, 500, p, None, 0, None) == -1 and "workspace" in _err()       # large map: A needs the workspace
        assert fn(p, p, p, 2, 9, 80, 80, 500, p, p, 64, None) == -1 and "workspace" in _err()
        assert fn(None, None, None, 0, 3, 4, 4, 5, None, None, 0, None) == 0                           # N * C == 0: nothing to do
    fn = L.vllm_point_sample_backward_f32
    assert fn(odd, p, 1, 3, 4, 4, 5, p, None, 0, None) == -1 and "coords must be 8-byte aligned" in _err()
    assert fn(p, p, 65536, 3, 4, 4, 5, p, None, 0, None) == -1 and "too many regions / too large a map for one launch" in _err()
    assert fn(p, None, 1, 3, 4, 4, 5, p, None, 0, None) == -1 and "null pointer" in _err()
    assert fn(p, p, 1, 3, 4, 4, 5, None, None, 0, None) == -1 and "null pointer" in _err()
    assert fn(None, None, 0, 3, 4, 4, 5, None, None, 0, None) == 0


def test_coordinate_gradients_are_refused_by_name():
    """point_coords.requires_grad raises NotImplementedError naming it.  The public functions check the device first, so the check
    itself is called here (test_region_train_gpu.py goes through the public functions), with the dtype rule of the differentiable path."""
    c = torch.rand(2, 3, 2, requires_grad=True)
    with pytest.raises(NotImplementedError, match="point_coords"):
        A._no_coord_grad("point_sample", c)
    A._no_coord_grad("point_sample", c.detach())
    x = torch.zeros(1, 2, 3, 3, dtype=torch.float16)
    assert A._train_map(x).dtype == torch.float32 and A._train_map(x.bfloat16()).dtype == torch.bfloat16


def test_built_coordinates_floor_to_the_same_cell_in_fp32_and_fp64():
    """What the GPU tests' bounds assume of their inputs: the kernel's fp32 pixel position ((2c - 1 + 1) * size - 1) / 2 floors to
    the cell fp64 gives, for every point of every shape, so no case needs excluding."""
    for (H, W, P) in [(24, 24, 2304), (5, 7, 300), (80, 80, 500), (24, 24, 64), (1, 1, 7), (5, 9, 1)]:
        c = RT.make_coords(16, P, H, W, torch.Generator().manual_seed(H * 100 + W + P))
        for k, size in ((0, W), (1, H)):
            f32 = ((2.0 * c[..., k] - 1.0 + 1.0) * float(size) - 1.0) * 0.5
            assert f32.dtype == torch.float32
            f64 = ((2 * c[..., k].double() - 1 + 1) * size - 1) / 2
            assert torch.equal(f32.floor().double(), f64.floor())
            frac = f64 - f64.floor()
            assert frac.min() > 0.015 and frac.max() < 0.985
        assert (c.min() < 0) and (c.max() > 1)                     # points outside the map are covered
