"""The bar and the buffers every native-kernel case module shares.

The bar, for every element: |native - fp64| <= 4 e_ref + spacing(float32(max|fp64|)), e_ref the max deviation of CPU fp32 torch from
the same CPU fp64 result, per tensor - the project's standing rule and factor (tests/test_encoders_cpu.py, the train-loss tests).
The buffers: one driver of a C ABI runs on host arrays (the emulator build) and on device tensors (the product library) alike.
"""
import ctypes

import numpy as np
import torch
from torch.utils._python_dispatch import TorchDispatchMode

FACTOR = 4.0
CANARY = -7.25


def ratio(native, f64, e_ref):
    """(max|native - fp64| - 1 ulp of max|fp64|) / e_ref, floored at 0: the bar is ratio <= FACTOR"""
    err = float(np.abs(np.asarray(native, np.float64) - f64).max())
    over = max(0.0, err - float(np.spacing(np.float32(np.abs(f64).max()))))
    if over == 0.0:
        return 0.0
    return over / e_ref if e_ref > 0.0 else float("inf")


def check(label, native, f64, e_ref, tag="conv"):
    assert np.isfinite(np.asarray(native)).all(), label
    r = ratio(native, f64, e_ref)
    print(f"[{tag} parity] {label}: ratio {r:.3f} (e_ref {e_ref:.3e}, bar {FACTOR:g})")
    assert r <= FACTOR, (label, r, e_ref)
    return r


def fp64_and_e_ref(run):
    """run(dtype) -> {tensor: numpy array}, called in fp64 and in fp32 -> ({tensor: fp64 array, read-only}, {tensor: e_ref})"""
    r64, r32 = run(torch.float64), run(torch.float32)
    e_ref = {k: float(np.abs(r32[k].astype(np.float64) - r64[k]).max()) for k in r64}
    for v in r64.values():
        v.setflags(write=False)
    return r64, e_ref


def nhwc(t):
    """NCHW torch / numpy -> contiguous NHWC numpy fp32"""
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1), dtype=np.float32)


def nchw(a):
    return np.asarray(a).transpose(0, 3, 1, 2)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class HostArrays:
    """numpy buffers: the emulator build"""
    stream = None

    def put(self, a):
        return np.ascontiguousarray(a, dtype=np.float32)

    def full(self, shape, value, dtype=np.float32):
        return np.full(shape, value, dtype)

    def ptr(self, a):
        return None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def get(self, a):
        return None if a is None else a.copy()


class DeviceArrays:
    """torch tensors on the GPU: the product library"""

    @property
    def stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def put(self, a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()

    def full(self, shape, value, dtype=np.float32):
        return torch.full(tuple(int(v) for v in np.atleast_1d(shape)), value, dtype={np.float32: torch.float32, np.uint8: torch.uint8}[dtype],
                          device="cuda")

    def ptr(self, a):
        return None if a is None else ctypes.c_void_p(a.data_ptr())

    def get(self, a):
        return None if a is None else a.cpu().numpy()


class Spy(TorchDispatchMode):
    """the names of the operators that run under it, and for aten::add the largest tensor argument"""

    def __init__(self):
        super().__init__()
        self.names, self.adds = [], []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.names.append(func.name())
        if func.name().startswith("aten::add"):
            self.adds.append(max([a.numel() for a in args if isinstance(a, torch.Tensor)] + [0]))
        return func(*args, **(kwargs or {}))
