#!/usr/bin/env python3
"""tools/accuracy_model.py -- the rounding-count model behind the worst-bin
bound of multi-pass plans in tests/test_gpu_accuracy.py.

No kernel runs here and no measured kernel error enters: the inputs are the
number format (one componentwise rounding of a unit complex value: rms rho u),
the count of rounded operations in the inter-pass twiddle chain as
csrc/pifft_kernels.h writes it (k_pass first stage of a later pass, BM == 2,
and apply_powers), and the oracle's own error constant c_o, rel-L2 = c_o u
sqrt(log2 N) (tests/test_hp_reference.py prints it: 0.66 fp32, 1.45 fp64; for
the C2R yardstick -- the real part of the oracle's transform of a Hermitian
spectrum -- `--hermitian` measures it here on the CPU: 0.65 fp32, 0.69 fp64).

Prints, per precision, pass count p and size: the model's rel-L2 ratio r =
sigma_k / sigma_o, the tail factor h (how much further the maximum over N bins
of the kernel's scale-mixture errors sits above its rms than that of N
equal-variance Gaussians), r h, and 1.3 r h (1.3: the same allowance for the
spread of a maximum that the factor 4 carries).  numpy only.

worst_bin_bound(c_o, passes, log2 N, bins) is that last figure as a function,
the tail taken over `bins` bins (default N): tests/test_gpu_instances.py puts
several hundred cases under one bound and takes bins = N times their number.
"""
import math
import os
import sys

import numpy as np

# rms error, in u, of rounding both components of a unit complex value: a
# component in [2^-j, 2^(1-j)) takes a uniform error of up to half an ulp =
# 2^-j u, variance (2^-j u)^2 / 3; |cos| of a uniform angle falls in [1/2, 1)
# with probability 2/3, [1/4, 1/2) 0.17, [1/8, 1/4) 0.08: 0.0596 u^2 per
# component, 0.119 u^2 per value.
RHO = 0.345
Q = 16  # radix of the first stage of a later pass (VPT 16)


def chain_variance():
    """(all of it, the part coherent along a last-pass line), in u^2 relative
    to the values, averaged over the power k < Q.
    step = fl(hi lo): two rounded table entries and a product of two rounded
    operations per component: var(delta) = 4 rho^2.  anc[i] = anc[i-1]^2 adds
    r_i (2 rho^2) and doubles what came before: w^k, k = sum of bits, carries
    k delta + (k >> 1) r_1 + (k >> 2) r_2 + (k >> 3) r_3 + one r per product of
    apply_powers.  (The product v[k] w^k itself is the oracle's too.)  The
    common factor base = fl(hi lo) in place of one correctly rounded entry
    adds 3 rho^2."""
    k = np.arange(Q)
    d2, r2 = 4 * RHO ** 2, 2 * RHO ** 2
    pops = np.array([bin(i).count("1") for i in k])
    var_k = k ** 2 * d2 + ((k >> 1) ** 2 + (k >> 2) ** 2 + (k >> 3) ** 2) * r2 + np.maximum(0, pops - 1) * r2
    return var_k.mean() + 3 * RHO ** 2, (k ** 2).mean() * d2


def tail(n, a2, b2):
    """t with n P(|eps| > t) = 1 for eps | z ~ CN(0, a2 + b2 z), z ~ Exp(1):
    |delta|^2 of a line taken as exponential (delta a sum of bounded
    roundings: a Gaussian tail overstates it).  Trapezoid rule and bisection."""
    z = np.linspace(0.0, 80.0, 400001)

    def log_np(t):
        f = np.exp(-z - t * t / (a2 + b2 * z))
        p = float(np.sum(f[1:] + f[:-1]) * 0.5 * (z[1] - z[0]))
        return math.log(n) + math.log(max(p, 1e-300))
    lo, hi = 0.1, 100 * math.sqrt(a2 + b2)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if log_np(mid) > 0 else (lo, mid)
    return 0.5 * (lo + hi)


def hermitian():
    """The C2R yardstick's constant: the oracle's transform of a Hermitian
    spectrum against fft_hp, real and imaginary parts of the error apart."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "oracle"))
    import pifft_oracle as oracle
    for name, dt, u in (("fp64", np.complex128, 2.0 ** -53), ("fp32", np.complex64, 2.0 ** -24)):
        for logn in (11, 16, 20):
            n, h = 1 << logn, 1 << (logn - 1)
            rng = np.random.default_rng(1000 * logn + 1)
            X = ((rng.uniform(-1, 1, h + 1) + 1j * rng.uniform(-1, 1, h + 1)) / math.sqrt(n)).astype(dt)
            X[0], X[h] = X[0].real, X[h].real
            full = np.concatenate([X, np.conj(X[h - 1:0:-1])])
            H = oracle.fft_hp(full)
            e = oracle.fft(full, P=1).astype(np.clongdouble) - H
            nh = float(np.sqrt(np.sum(H.real ** 2 + H.imag ** 2)))
            g = oracle.generate(n, dt, seed=5)
            G = oracle.fft_hp(g)
            eg = oracle.fft(g, P=1).astype(np.clongdouble) - G
            unit = u * math.sqrt(logn)
            re, im = (float(np.sqrt(np.sum(c ** 2))) / nh / unit for c in (e.real, e.imag))
            tot = float(np.sqrt(np.sum(eg.real ** 2 + eg.imag ** 2)) / np.sqrt(np.sum(G.real ** 2 + G.imag ** 2))) / unit
            print(f"{name} 2^{logn}: Hermitian input, error / (u sqrt(log2 N)): real part {re:.3f}  imaginary part {im:.3g}"
                  f"  | generic input, whole error {tot:.3f}")


SPREAD = 1.3  # the allowance for the spread of a maximum that the factor 4 carries


def model(co, passes, logn, bins=None):
    """(sigma_o, sigma_k, r, h) of a plan of `passes` passes at N = 2^logn,
    the oracle's constant co: the kernel's worst error taken over `bins` bins
    (default N: one transform), the oracle's over its own N.  More bins than
    N: a bound shared by several cases, the largest of whose ratios is held
    to it (tests/test_gpu_instances.py: bins = N times their number)."""
    c2, coh2 = chain_variance()
    n = 2.0 ** logn
    so2 = co ** 2 * logn
    sk2 = so2 + (passes - 1) * c2
    r = np.sqrt(sk2 / so2)
    # only the LAST pass's chain stays coherent over final bins: earlier
    # passes' lines are mixed by the passes behind them
    h = tail(n if bins is None else float(bins), sk2 - coh2, coh2) / np.sqrt(sk2 * np.log(n))
    return np.sqrt(so2), np.sqrt(sk2), r, h


def worst_bin_bound(co, passes, logn, bins=None):
    """The worst-bin bound, in units of the oracle's worst bin: 1.3 r h."""
    _, _, r, h = model(co, passes, logn, bins)
    return float(SPREAD * r * h)


def main():
    c2, coh2 = chain_variance()
    print(f"sigma_delta {2 * RHO:.2f} u; chain term per inter-pass twiddle {np.sqrt(c2):.2f} u "
          f"(of which one delta per line: {np.sqrt(coh2):.2f} u)")
    if "--hermitian" in sys.argv[1:]:
        return hermitian()
    for name, co in (("fp32", 0.66), ("fp64", 1.45), ("C2R fp32", 0.65), ("C2R fp64", 0.69)):
        for p in (2, 3):
            for logn in (14, 16, 18, 20, 21, 22):
                so, sk, r, h = model(co, p, logn)
                print(f"{name} p={p} 2^{logn}: sigma_o {so:.2f} u  sigma_k {sk:.2f} u  "
                      f"r {r:.2f}  h {h:.2f}  r h {r * h:.2f}  1.3 r h {SPREAD * r * h:.2f}")


if __name__ == "__main__":
    main()
