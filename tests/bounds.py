"""What the GPU tests and the ``*_train_inputs`` modules share: the project's per-element bound for a bf16 result against an fp64
reference, a relative RMS, and the two ctypes shorthands of a test that calls the C ABI directly."""
import torch

from visionllm_amd import _lib

DEV = "cuda:0"
P = _lib.ptr   # device pointer of a tensor (None stays None)


def stream():
    return _lib.current_stream(torch.device(DEV))


def bf16_ulp(x):
    """Spacing of bf16 numbers at |x| (8 significand bits): 2^(floor(log2 |x|) - 7); the smallest normal's for |x| -> 0."""
    e = torch.floor(torch.log2(x.abs().double().clamp_min(2.0 ** -126)))
    return torch.pow(2.0, e - 7)


def _excess(out, ref, mag, rel_mag):
    err = (out.double() - ref.double()).abs()
    return (err - rel_mag * mag).clamp_min(0) / bf16_ulp(ref)


def excess_ulp(out, ref, mag, rel_mag=2.0 ** -17):
    """max over elements of (|out - ref| - rel_mag * mag) / ulp(ref): the bound holds when this is <= 1."""
    return _excess(out, ref, mag, rel_mag).max().item()


def assert_bound(out, ref, mag, what, rel_mag=2.0 ** -17):
    """|out - ref| <= 1 bf16 ulp(ref) + rel_mag * sum|terms| (the GEMM tests' bound); the worst element's figure is printed first."""
    u = _excess(out, ref, mag, rel_mag)
    print(f"{what}: max excess {u.max().item():.3f} bf16 ulp")
    assert u.max().item() <= 1.0, f"{what}: {u.max().item():.2f} bf16 ulp at {int(u.argmax())}"


def rel_rms(got, ref, clamp=False):
    """rms(got - ref) / rms(ref) in fp64.  An all-zero reference is kept from dividing by zero by adding 1e-300 to the denominator, or
    (``clamp``, the attention tests' form) by raising it to 1e-300."""
    ref = ref.double()
    num = (got.double() - ref).pow(2).mean().sqrt().item()
    den = ref.pow(2).mean().sqrt().item()
    return num / (max(den, 1e-300) if clamp else den + 1e-300)
