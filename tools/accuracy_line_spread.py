#!/usr/bin/env python3
"""tools/accuracy_line_spread.py -- how the error of multi-pass plans spreads
over the last pass's lines (needs an MI355X; profiles/accuracy_line_spread.txt
is its output, DESIGN.md section 13 reads it).

The final bins k = j + (N / R_last) r, r < R_last, come from line j of the last
pass and share its inter-pass step twiddle.  Per plan (P = 1, natural order,
the input of tests/test_gpu_accuracy.py) and for the oracle on the same
input: the error variance per line over the mean variance (1st percentile,
median, 99th, maximum), the same for a control grouping of R_last consecutive
bins, and the figure of the line that holds the worst bin.  Equal-variance
errors give both groupings the same narrow spread around 1."""
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(R, "cs87project-msolano2_amd"), os.path.join(R, "oracle")]
import numpy as np
import torch

import pifft
import pifft_oracle as oracle

for suf, logn in (("f32", 15), ("f32", 18), ("f32", 21), ("f64", 15), ("f64", 21)):
    n = 1 << logn
    dt = np.complex64 if suf == "f32" else np.complex128
    x = oracle.generate(n, dt, seed=0xACC0 + logn)
    H = np.fft.fft(x.astype(np.complex128)) if suf == "f32" else oracle.fft_hp(x)
    O = oracle.fft(x, P=1)
    plan = pifft.Plan(n, 1, 1, pifft.F32 if suf == "f32" else pifft.F64)
    d = plan.describe()
    d_in = torch.from_numpy(x).to("cuda")
    d_out = torch.empty_like(d_in)
    plan.execute_device(d_in.data_ptr(), d_out.data_ptr(), torch.cuda.current_stream())
    torch.cuda.synchronize()
    K = d_out.cpu().numpy()
    rl = d["radix"][-1]
    ns = n // rl
    for name, Y in (("kernel", K), ("oracle", O)):
        e = np.abs(np.asarray(Y - H, dtype=np.complex128)) ** 2
        tot = e.mean()
        line = e.reshape(rl, ns).mean(axis=0)          # bin k = j + ns r: line j = k mod ns
        other = e.reshape(ns, rl).mean(axis=1)         # control grouping: rl consecutive bins
        q = np.quantile(line / tot, [0.01, 0.5, 0.99])
        qo = np.quantile(other / tot, [0.01, 0.5, 0.99])
        worst = np.argmax(e)
        print(f"{suf} 2^{logn} radix {d['radix']} {name}: per-line variance / mean: 1% {q[0]:.2f} median {q[1]:.2f} 99% {q[2]:.2f} max {line.max() / tot:.2f}"
              f" | control (consecutive bins) 1% {qo[0]:.2f} 99% {qo[2]:.2f} max {other.max() / tot:.2f}"
              f" | worst bin's line variance / mean {line[worst % ns] / tot:.2f}")
