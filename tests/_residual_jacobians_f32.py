"""Shared by tests/test_residual_jacobians_f32_abi.py (CPU) and tests/test_gpu_residual_jacobians_f32.py: the cast of the FP32
residual-Jacobian transport (kpilqr_upload_residual_jacobians_f32, include/kpilqr.h) and the twin of a synthetic problem that carries
the DECODED Jacobians -- what the library's exact widening leaves on the device, as doubles -- so that the FP64 calls, the numpy
restatement (oracle/crosscheck.py) and the FP32 calls can be run on the same numbers."""
import numpy as np


def cast(a):
    """The caller's side: a plain round-to-nearest-even cast to float32 (nothing is encoded)"""
    return np.ascontiguousarray(a, dtype=np.float32)


def decode(a32):
    """The library's side restated: the exact widening"""
    a32 = np.asarray(a32)
    assert a32.dtype == np.float32
    return a32.astype(np.float64)


def decoded_twin(p):
    """The problem with r_x, r_u replaced by the doubles the FP32 transport delivers; everything else is shared with p"""
    q = dict(p)
    q["r_x"], q["r_u"] = decode(cast(p["r_x"])), decode(cast(p["r_u"]))
    return q
