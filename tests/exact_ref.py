"""CPU restatement of az_gemm_exact_f32's arithmetic contract (include/az_hip.h): per output, one
fp32 fmaf chain per segment of az_gemm_exact_plan in ascending k from +0, the segment sums added in
ascending order, then the bias, then the activation.

numpy has no fp32 fma and an fp64 round trip rounds twice, so the chain runs in a few lines of C++
compiled when first used (std::fmaf, -O2 -ffp-contract=off: no contraction of the plain adds); its
fmaf is itself checked against exact rational arithmetic by tests/test_exact_host.py."""
import ctypes
import os
import shutil
import subprocess
import tempfile
from fractions import Fraction

import numpy as np

SRC = r"""
#include <cmath>
extern "C" float fma32(float a, float b, float c) { return std::fmaf(a, b, c); }
extern "C" void exact_gemm(const float* A, long lda, const float* W, long ldw, const float* bias,
                           int relu, float* C, int M, int N, int S, const int* seg) {
  for (int i = 0; i < M; ++i)
    for (int j = 0; j < N; ++j) {
      float total = 0.f;
      for (int s = 0, k = 0; s < S; ++s) {
        float acc = 0.f;
        for (int e = k + seg[s]; k < e; ++k) acc = std::fmaf(A[i * lda + k], W[j * ldw + k], acc);
        total = s == 0 ? acc : total + acc;
      }
      if (bias) total = total + bias[j];
      C[(long)i * N + j] = relu && !(total > 0.f) ? 0.f : total;
    }
}
"""

_LIB = None
_DIR = None


def lib():
    """The helper, compiled once per process into a temporary directory (None: no C++ compiler)."""
    global _LIB, _DIR
    if _LIB is None:
        cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
        if cxx is None:
            return None
        _DIR = tempfile.TemporaryDirectory(prefix="exact_ref_")
        src, so = os.path.join(_DIR.name, "exact_ref.cpp"), os.path.join(_DIR.name, "exact_ref.so")
        with open(src, "w") as f:
            f.write(SRC)
        subprocess.run([cxx, "-O2", "-ffp-contract=off", "-fPIC", "-shared", src, "-o", so],
                       check=True)
        L = ctypes.CDLL(so)
        L.fma32.restype = ctypes.c_float
        L.fma32.argtypes = [ctypes.c_float] * 3
        L.exact_gemm.restype = None
        L.exact_gemm.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long,
                                 ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                 ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        _LIB = L
    return _LIB


def fma32(a, b, c):
    return np.float32(lib().fma32(float(np.float32(a)), float(np.float32(b)), float(np.float32(c))))


def round_f32(x, with_tie=False):
    """The float32 nearest to the rational x, ties to even (finite, no overflow handling);
    with_tie: (value, whether x lay exactly half way between two floats)."""
    x = Fraction(x)
    if x == 0:
        return (np.float32(0.0), False) if with_tie else np.float32(0.0)
    sign, m = (-1 if x < 0 else 1), abs(x)
    e = m.numerator.bit_length() - m.denominator.bit_length()
    if Fraction(2) ** e > m:
        e -= 1
    assert Fraction(2) ** e <= m < Fraction(2) ** (e + 1)
    q = Fraction(2) ** (max(e, -126) - 23)          # spacing of float32 at m (subnormals: 2^-149)
    n, rem = divmod(m, q)
    n = int(n)
    if rem * 2 > q or (rem * 2 == q and n % 2 == 1):
        n += 1
    v = np.float32(sign * float(n * q))             # n q has <= 24 significant bits: exact
    return (v, rem * 2 == q) if with_tie else v


def plan(N, K):
    """az_gemm_exact_plan(N, K): the segment lengths (the library loads without a GPU)."""
    from azhip import ops
    return ops.gemm_exact_plan(N, K)


def linear(x, w, b=None, relu=False, segments=None):
    """act(x w^T + b) by the contract; x [M][K], w [N][K] float32 arrays -> float32 [M][N]."""
    x = np.ascontiguousarray(x, np.float32)
    w = np.ascontiguousarray(w, np.float32)
    M, K = x.shape
    N = w.shape[0]
    seg = np.asarray(plan(N, K) if segments is None else segments, np.int32)
    assert seg.sum() == K and w.shape[1] == K
    out = np.empty((M, N), np.float32)
    bias = None if b is None else np.ascontiguousarray(b, np.float32)
    lib().exact_gemm(x.ctypes.data, K, w.ctypes.data, K, None if bias is None else bias.ctypes.data,
                     int(relu), out.ctypes.data, M, N, len(seg), seg.ctypes.data)
    return out
