"""The yardstick of tests/test_gpu_accuracy.py, checked on the CPU.

oracle.fft_hp is a radix-2 FFT in 80-bit long double (oracle/fft_hp.c); the GPU
accuracy tests bound a kernel's error by a multiple of the ORACLE's error
against it.  That is only as good as the two references, so here:

* fft_hp itself against directly summed long-double DFT bins and numpy's fp64 FFT;
* the oracle's error against fft_hp inside an envelope from its rounding count:
  a condition, not a measurement -- an oracle that grew less accurate would
  widen every kernel bound with it, and must fail here first;
* the three inputs whose transform is exact in any precision, through the
  oracle, bit for bit (the GPU tests run the same three through every plan
  structure).

No GPU: this file runs under -m "not gpu".
"""
import functools
import math

import numpy as np
import pytest

import pifft_oracle as oracle

# fails (does not skip) where long double is not the x87 80-bit format: without
# it there is no yardstick, and the accuracy tests must not pass by default
assert np.finfo(np.longdouble).nmant >= 63, \
    "tests/test_hp_reference.py needs an 80-bit long double (x86-64); np.longdouble has a %d-bit mantissa here" % \
    np.finfo(np.longdouble).nmant

DT = {"f32": np.complex64, "f64": np.complex128}
U = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
TWO_PI = np.longdouble("6.283185307179586476925286766559005768")


def norm_ld(v):
    v = np.asarray(v, dtype=np.clongdouble)
    return np.sqrt(np.sum(v.real * v.real + v.imag * v.imag))


def rel_l2_ld(a, b):
    """||a - b|| / ||b|| in long double."""
    return float(norm_ld(np.asarray(a, dtype=np.clongdouble) - b) / norm_ld(b))


def worst_bin_ld(a, b):
    """max |a - b| / rms(b) in long double."""
    d = np.asarray(a, dtype=np.clongdouble) - b
    return float(np.sqrt(np.max(d.real * d.real + d.imag * d.imag)) / (norm_ld(b) / math.sqrt(len(b))))


def dft_bin_ld(x, k):
    """X[k] summed directly in long double: the exponent (j k mod N) / N is exact."""
    n = len(x)
    a = TWO_PI * (((np.arange(n, dtype=np.uint64) * np.uint64(k)) % np.uint64(n)).astype(np.longdouble) / np.longdouble(n))
    w = np.cos(a) - 1j * np.sin(a)
    return np.sum(x.astype(np.clongdouble) * w)


@functools.lru_cache(maxsize=None)
def generated(suf, logn):
    x = oracle.generate(1 << logn, DT[suf], seed=0xACC0 + logn)
    H = oracle.fft_hp(x)
    x.setflags(write=False)
    H.setflags(write=False)
    return x, H


def test_fft_hp_returns_long_double_and_keeps_its_input():
    x = oracle.generate(64, np.complex64)
    keep = x.copy()
    H = oracle.fft_hp(x)
    assert H.dtype == np.clongdouble and H.shape == x.shape and np.array_equal(x, keep)
    with pytest.raises(ValueError):
        oracle.fft_hp(x.astype(np.clongdouble))
    with pytest.raises(RuntimeError):
        oracle.fft_hp(x[:48])


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("logn", [4, 10, 14])
def test_fft_hp_against_direct_dft_bins(suf, logn):
    n = 1 << logn
    x, H = generated(suf, logn)
    nx = float(norm_ld(x))
    for k in (0, 1, n // 2 + 3, n - 1):
        err = float(abs(H[k] - dft_bin_ld(x, k)))
        print(f"{suf} 2^{logn} bin {k}: |fft_hp - DFT| = {err:.2e} (bound {1e-17 * nx:.2e})")
        assert err <= 1e-17 * nx


@pytest.mark.parametrize("suf,logn", [(suf, logn) for logn in (1, 4, 10, 14, 20) for suf in ("f64", "f32")] +
                         [("f32", 22)])  # (2^22: the largest size tests/test_gpu_accuracy.py takes numpy for fp32 data at)
def test_fft_hp_against_numpy(suf, logn):
    x, H = generated(suf, logn)
    err = rel_l2_ld(np.fft.fft(x.astype(np.complex128)), H)
    print(f"{suf} 2^{logn}: rel-L2(np.fft.fft, fft_hp) = {err:.2e}")
    assert err <= 1e-15


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("logn,P", [(4, 2), (10, 4), (16, 8)])
def test_tree_hp_is_the_tree_stage(suf, logn, P):
    """tree_hp(x, P)[q M : (q+1) M] is the oracle's tree_segment(x, P, q) in
    exact arithmetic.  Per level the oracle rounds a sum or difference (u), a
    twiddle (u) and a complex product (sqrt(5) u at worst): under 5 u a level,
    adding linearly at worst over the log2 P levels."""
    n, lp = 1 << logn, P.bit_length() - 1
    x, _ = generated(suf, logn)
    T = oracle.tree_hp(x, P)
    m = n // P
    for q in range(P):
        err = rel_l2_ld(oracle.tree_segment(x, P, q), T[q * m:(q + 1) * m])
        assert err <= 5 * U[suf] * lp, (q, err)
    # ... and finishing the levels gives fft_hp: worker q's bins are X[bitrev(q) + P k]
    H = oracle.fft_hp(x)
    for q in (0, P - 1):
        seg = oracle.fft_hp(T[q * m:(q + 1) * m].astype(np.complex128))
        want = H[oracle.bit_reverse(q, lp)::P]
        # the segment's twiddles are w_N^{P k} = w_M^k: the same DIF levels; the
        # only difference is the segment rounded to fp64 on the way in
        assert rel_l2_ld(seg, want) <= 4 * 2.0 ** -53


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("logn", [4, 10, 16, 20])
def test_oracle_error_envelope(suf, logn):
    """rel-L2(oracle, fft_hp) <= 2 u sqrt(log2 N) and the worst bin <= 12 u
    sqrt(log2 N) rms: log2 N radix-2 levels, each a rounded sum and a rounded
    product by a rounded twiddle, errors adding in quadrature.  Measured: at
    most 0.7 (fp32) and 1.5 (fp64) u sqrt(log2 N), worst bin 2.8 and 7.6."""
    n = 1 << logn
    x, H = generated(suf, logn)
    O = oracle.fft(x, P=1)
    unit = U[suf] * math.sqrt(logn)
    e, m = rel_l2_ld(O, H), worst_bin_ld(O, H)
    print(f"oracle {suf} 2^{logn}: rel-L2 {e:.3e} = {e / unit:.2f} u sqrt(log2 N); worst bin {m:.3e} rms = {m / unit:.2f}")
    assert e <= 2 * unit
    assert m <= 12 * unit


def exact_cases(n, dtype):
    """(name, x, X): inputs whose DFT is exact in any precision -- every
    non-zero value meets only the twiddle w^0 = (1, -0), zeros stay zeros."""
    one = np.ones(n, dtype=dtype)
    delta = np.zeros(n, dtype=dtype)
    delta[0] = 1
    alt = np.zeros(n, dtype=dtype)
    alt[1::2] = 1
    X_alt = np.zeros(n, dtype=dtype)
    X_alt[0] += n // 2
    X_alt[n // 2] -= n // 2  # (n = 2: bins 0 and 1 are 1 and -1)
    return [("constant", one, n * delta), ("impulse", delta, one), ("alternating", alt, X_alt)]


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("logn,P", [(3, 1), (10, 4), (16, 8), (20, 32)])
def test_exact_inputs_through_the_oracle(suf, logn, P):
    for name, x, X in exact_cases(1 << logn, DT[suf]):
        got = oracle.fft(x, P=P, nthreads=16)
        assert np.array_equal(got, X), name
        assert np.array_equal(oracle.fft_hp(x), X.astype(np.clongdouble)), name
