"""ctypes loader of libpinnjet_probe.so (tests/probe/jet_device_probe.hip): the inline functions of csrc/jet_device.h behind
element-wise kernels.  Test infrastructure only; fails loudly when the library is absent (it is built by
`make -C pinns-rl-pde_amd/csrc` beside libpinnjet.so), never skips.

Every wrapper takes and returns contiguous float32 CUDA tensors, K x n stream-major, and launches on the current stream.
"""

from __future__ import annotations

import ctypes
import os

import torch  # before the library: both bind to the HIP runtime torch has loaded

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(_ROOT, "pinns-rl-pde_amd", "libpinnjet_probe.so")
ACT = {"tanh": 0, "sin": 1, "gelu": 2, "sigmoid": 3, "relu": 4, "leaky_relu": 5, "identity": 6}
# the stream sets csrc/Makefile compiles: SETS, then ASETS
STREAM_SETS = ((0, 0), (1, 0), (1, 1), (1, 2), (1, 3), (1, 4), (2, 0), (2, 2), (0, 1), (0, 2), (0, 3), (0, 4))
MAX_LAUNCH = 1 << 21

_lib = None


class ProbeError(RuntimeError):
    """The probe library is missing or a launch returned a HIP error."""


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ProbeError(f"{LIB_PATH} not found: build it with `make -C pinns-rl-pde_amd/csrc` (the `all` target)")
    lib = ctypes.CDLL(LIB_PATH)
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float
    for name, args in (
        ("probe_sincos", [vp, vp, vp, vp, vp, i64, vp]),
        ("probe_tanh", [vp, vp, vp, i64, vp]),
        ("probe_act_derivs", [i32, i32, f32, i32, vp, vp, i64, vp]),
        ("probe_act_fwd", [i32, i32, i32, f32, i32, vp, vp, i64, vp]),
        ("probe_act_bwd", [i32, i32, i32, f32, i32, vp, vp, vp, i64, vp]),
        ("probe_act_merged", [i32, f32, f32, i32, vp, vp, vp, vp, vp, i64, vp]),
        ("probe_fourier_coef_partial", [vp, vp, vp, i64, vp]),
    ):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = ctypes.c_int, args
    _lib = lib
    return lib


def _check(rc, what):
    if rc != 0:
        raise ProbeError(f"{what}: HIP error {rc}")


def _in(t):
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), (t.device, t.dtype)
    return t


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nan(shape, like):
    """Outputs start as NaN: a value a kernel should have written but did not cannot pass."""
    return torch.full(shape, float("nan"), dtype=torch.float32, device=like.device)


def sincos(x):
    """(fast sin, fast cos, library sinf, library cosf) of a 1-D tensor of at most MAX_LAUNCH elements."""
    n = _in(x).numel()
    assert x.dim() == 1 and n <= MAX_LAUNCH
    out = [_nan((n,), x) for _ in range(4)]
    _check(load().probe_sincos(x.data_ptr(), *(o.data_ptr() for o in out), n, _stream()), "probe_sincos")
    return tuple(out)


def tanh(z):
    """(fast_tanhf, library tanhf)."""
    n = _in(z).numel()
    assert z.dim() == 1 and n <= MAX_LAUNCH
    y, y_lib = _nan((n,), z), _nan((n,), z)
    _check(load().probe_tanh(z.data_ptr(), y.data_ptr(), y_lib.data_ptr(), n, _stream()), "probe_tanh")
    return y, y_lib


def act_derivs(act, ord_, param, tape, z):
    """f[0 .. ord] at z as an (ord + 1, n) tensor; tape: act_derivs_tape on the slot-0 value the forward kernels store."""
    n = _in(z).numel()
    assert z.dim() == 1
    f = _nan((ord_ + 1, n), z)
    _check(load().probe_act_derivs(ACT[act], ord_, param, int(tape), z.data_ptr(), f.data_ptr(), n, _stream()), "probe_act_derivs")
    return f


def act_fwd(act, nt, nx, param, tape, z):
    K, n = _in(z).shape
    assert K == 1 + nt + nx
    a = _nan((K, n), z)
    _check(load().probe_act_fwd(ACT[act], nt, nx, param, int(tape), z.data_ptr(), a.data_ptr(), n, _stream()), "probe_act_fwd")
    return a


def act_bwd(act, nt, nx, param, tape, z, ab):
    K, n = _in(z).shape
    assert K == 1 + nt + nx and _in(ab).shape == z.shape
    zb = _nan((K, n), z)
    _check(load().probe_act_bwd(ACT[act], nt, nx, param, int(tape), z.data_ptr(), ab.data_ptr(), zb.data_ptr(), n, _stream()),
           "probe_act_bwd")
    return zb


def act_merged(act, param, cc, tape, z, ab):
    """(a, zb, part) of the merged stream set [value, w, d/dx]: forward jets, adjoint and the coefficient partial."""
    K, n = _in(z).shape
    assert K == 3 and _in(ab).shape == z.shape
    a, zb, part = _nan((3, n), z), _nan((3, n), z), _nan((n,), z)
    _check(load().probe_act_merged(ACT[act], param, cc, int(tape), z.data_ptr(), ab.data_ptr(), a.data_ptr(), zb.data_ptr(),
                                   part.data_ptr(), n, _stream()), "probe_act_merged")
    return a, zb, part


def fourier_coef_partial(bx, value):
    n = _in(bx).numel()
    assert _in(value).numel() == n
    out = _nan((n,), bx)
    _check(load().probe_fourier_coef_partial(bx.data_ptr(), value.data_ptr(), out.data_ptr(), n, _stream()),
           "probe_fourier_coef_partial")
    return out
