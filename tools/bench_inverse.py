#!/usr/bin/env python3
"""tools/bench_inverse.py [--out FILE] [--repeats R] -- does an inverse plan
(PIFFT_INVERSE) cost what the forward plan of the same shape costs?

An inverse plan is the forward plan with its first and last launches replaced
by kernels that swap re/im of what they load / store (register renames), so
it should run in the same time.  For each shape below a forward and an inverse
plan are built on the SAME input and output buffers, both go through
pifft_plan_tune_workspace (where a plan's workspace lands alone moves config 4
by 7-20 %, include/pifft.h), and after a warm-up the two are timed alternately,
R repeats each, every repeat a loop of executions between two device events.

Reported per shape: the medians (ms per execution), the forward plan's own
repeat-to-repeat spread (max - min over its median), the ratio inverse /
forward, and `ok` = ratio <= 1.03, the project's 3 % tolerance (checks.tol of
bench.py's roofline check).  Where the forward spread itself exceeds 3 % the
box cannot resolve the question: `resolved` is false and `ok` says nothing.
One JSON document on stdout (and in FILE)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cs87project-msolano2_amd"))

import torch  # noqa: E402  (before libpifft: one HIP runtime)
import pifft  # noqa: E402

TOL = 0.03
# name, log2 n, workers, first, count, batch, precision
SHAPES = [
    ("C1 fp64 2^20 P=1", 20, 1, 0, 1, 1, 64),
    ("C2 slice fp64 2^20 P=8, one worker", 20, 8, 0, 1, 1, 64),
    ("C3 fp32 4096 x 4096", 12, 1, 0, 1, 4096, 32),
    ("C4 fp64 2^28 P=1", 28, 1, 0, 1, 1, 64),
    ("C4 fp32 2^28 P=1", 28, 1, 0, 1, 1, 32),
    # the tree and interleave launches' twins: a tree twin (+ the plain interleave twin), a
    # worker-interleaved tree twin, two tree twins + the tiled interleave twin
    ("tree twin fp64 2^15 P=16", 15, 16, 0, 16, 1, 64),
    ("worker-interleaved tree twin fp64 2^23 P=16", 23, 16, 0, 16, 1, 64),
    ("tiled interleave twin fp64 2^16 P=32", 16, 32, 0, 32, 1, 64),
]


def time_loop(plan, x, y, reps):
    st = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        plan.execute_device(x.data_ptr(), y.data_ptr(), st)
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def measure(shape, repeats, tries):
    name, logn, P, first, count, batch, prec = shape
    n = 1 << logn
    cdt = torch.complex128 if prec == 64 else torch.complex64
    x = torch.empty(n * batch, dtype=cdt, device="cuda")
    pifft.generate_device(x.data_ptr(), n * batch, n, prec)
    flags = pifft.OUT_NATURAL if count == P else pifft.OUT_SLICES
    kw = dict(first=first, count=count, device=torch.cuda.current_device(), flags=flags)
    fwd = pifft.Plan(n, P, batch, prec, **kw)
    inv = pifft.Plan(n, P, batch, prec, inverse=True, **kw)
    y = torch.empty(fwd.info.out_elems, dtype=cdt, device="cuda")
    st = torch.cuda.current_stream()
    for p in (fwd, inv):
        p.tune_workspace(x.data_ptr(), y.data_ptr(), st, tries)
    # loops of >= ~20 ms (at least 10 executions), sized on a first timing
    est = min(time_loop(p, x, y, 5) for p in (fwd, inv) for _ in range(2))
    reps = max(10, int(20.0 / max(est, 1e-3)))
    for p in (fwd, inv):
        time_loop(p, x, y, reps)  # warm-up
    ms = {"forward": [], "inverse": []}
    for _ in range(repeats):
        ms["forward"].append(time_loop(fwd, x, y, reps))
        ms["inverse"].append(time_loop(inv, x, y, reps))
    f, i = statistics.median(ms["forward"]), statistics.median(ms["inverse"])
    spread = (max(ms["forward"]) - min(ms["forward"])) / f
    d = fwd.describe()
    out = {
        "shape": name, "n": n, "workers": P, "first": first, "count": count, "batch": batch, "prec": prec,
        "launch_kind": d["launch_kind"], "launch_mode": d["launch_mode"],
        "kernels_forward": [fwd.kernel_name(k) for k in range(fwd.info.num_launches)],
        "kernels_inverse": [inv.kernel_name(k) for k in range(inv.info.num_launches)],
        "executions_per_repeat": reps, "repeats": repeats,
        "forward_ms": [round(v, 6) for v in ms["forward"]], "inverse_ms": [round(v, 6) for v in ms["inverse"]],
        "forward_median_ms": round(f, 6), "inverse_median_ms": round(i, 6),
        "forward_spread": round(spread, 4), "ratio": round(i / f, 4), "tol": TOL,
        "resolved": spread <= TOL, "ok": i <= f * (1 + TOL),
    }
    fwd.close()
    inv.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the JSON document here")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--tries", type=int, default=4, help="workspace placements pifft_plan_tune_workspace tries")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_inverse.py needs a GPU")
    rows = [measure(s, a.repeats, a.tries) for s in SHAPES]
    doc = {"tool": "tools/bench_inverse.py", "device": torch.cuda.get_device_name(0), "tol": TOL, "shapes": rows,
           "all_ok": all(r["ok"] for r in rows), "all_resolved": all(r["resolved"] for r in rows)}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    for r in rows:
        print(f"# {r['shape']}: forward {r['forward_median_ms']:.4f} ms (spread {100 * r['forward_spread']:.1f} %), "
              f"inverse {r['inverse_median_ms']:.4f} ms, ratio {r['ratio']:.4f}"
              f"{'' if r['resolved'] else '  [forward spread > 3 %: unresolved]'}", file=sys.stderr)


if __name__ == "__main__":
    main()
