#!/usr/bin/env python3
"""tools/bench_real.py [--out FILE] [--repeats R] -- what does a real-input plan
(pifft_plan_create_real) cost beside the complex plan a caller had to use
before, and do its two fix-up kernels stream at the rate of a copy?

For each shape below, in one process and on the same samples:
  (a) the R2C plan of N reals,
  (b) the C2R plan on (a)'s output,
  (c) the complex plan of the same N on the samples widened to complex,
  (d) a device-to-device copy of exactly the fix-up step's byte count
      (batch (2H + 1) values, H = N/2: what the step reads plus what it writes,
      half of it copied from one buffer to another),
are timed alternately after a warm-up, R repeats each, every repeat a loop of
executions between two device events.  Beside each median: the byte model
(the sum of pifft_plan_info.launch_bytes), and the fix-up launches' own
durations from pifft_execute_device_timed (median of R), whose ratio to (d)
is the streaming question: `post_over_copy` / `pre_over_copy`, `ok` where
<= 1.15 -- meaningful only where the working set is beyond the caches (the
2^28 shapes).  One JSON document on stdout (and in FILE)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cs87project-msolano2_amd"))

import torch  # noqa: E402  (before libpifft: one HIP runtime)
import pifft  # noqa: E402

TOL = 1.15
# name, log2 n, batch, precision
SHAPES = [
    ("fp64 2^20", 20, 1, 64),
    ("fp64 2^28", 28, 1, 64),
    ("fp32 2^28", 28, 1, 32),
    ("fp32 2^12 x 4096", 12, 4096, 32),
]


def time_loop(fn, reps):
    st = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def measure(shape, repeats):
    name, logn, batch, prec = shape
    n, h = 1 << logn, 1 << (logn - 1)
    cdt = torch.complex128 if prec == 64 else torch.complex64
    esz = 16 if prec == 64 else 8
    st = torch.cuda.current_stream()
    x = torch.empty(batch * h, dtype=cdt, device="cuda")  # batch rows of n reals
    pifft.generate_device(x.data_ptr(), batch * h, n, prec)
    r2c = pifft.RealPlan(n, 1, batch, prec)
    c2r = pifft.RealPlan(n, 1, batch, prec, inverse=True)
    X = torch.empty(r2c.info.out_elems, dtype=cdt, device="cuda")
    y = torch.empty(c2r.info.out_elems, dtype=cdt, device="cuda")
    r2c.execute_device(x.data_ptr(), X.data_ptr(), st)
    # (c): the same samples widened to complex, the N-point complex plan
    wide = torch.view_as_real(x).reshape(-1).to(cdt)
    cplx = pifft.Plan(n, 1, batch, prec)
    Y = torch.empty(cplx.info.out_elems, dtype=cdt, device="cuda")
    # (d): the fix-up step's bytes, half read and half written
    step_bytes = batch * (2 * h + 1) * esz
    src = torch.empty(step_bytes // 2, dtype=torch.uint8, device="cuda").zero_()
    dst = torch.empty_like(src)
    runs = {
        "r2c": lambda: r2c.execute_device(x.data_ptr(), X.data_ptr(), st),
        "c2r": lambda: c2r.execute_device(X.data_ptr(), y.data_ptr(), st),
        "complex": lambda: cplx.execute_device(wide.data_ptr(), Y.data_ptr(), st),
        "copy": lambda: dst.copy_(src),
    }
    reps = {}
    for k, fn in runs.items():  # loops of >= ~20 ms (at least 10 executions), sized on a first timing
        est = min(time_loop(fn, 5) for _ in range(2))
        reps[k] = max(10, int(20.0 / max(est, 1e-3)))
        time_loop(fn, reps[k])  # warm-up
    ms = {k: [] for k in runs}
    post, pre = [], []
    for _ in range(repeats):
        for k, fn in runs.items():
            ms[k].append(time_loop(fn, reps[k]))
        post.append(r2c.execute_device_timed(x.data_ptr(), X.data_ptr(), st)[-1])
        pre.append(c2r.execute_device_timed(X.data_ptr(), y.data_ptr(), st)[0])
    med = {k: statistics.median(v) for k, v in ms.items()}
    dr, dc, di = r2c.describe(), c2r.describe(), cplx.describe()
    assert dr["launch_bytes"][-1] == step_bytes == dc["launch_bytes"][0]
    post_ms, pre_ms = statistics.median(post), statistics.median(pre)
    out = {
        "shape": name, "n": n, "batch": batch, "prec": prec,
        "launch_kind": {"r2c": dr["launch_kind"], "c2r": dc["launch_kind"], "complex": di["launch_kind"]},
        "model_bytes": {"r2c": sum(dr["launch_bytes"]), "c2r": sum(dc["launch_bytes"]),
                        "complex": sum(di["launch_bytes"]), "copy": step_bytes},
        "model_ratio_r2c_over_complex": round(sum(dr["launch_bytes"]) / sum(di["launch_bytes"]), 4),
        "executions_per_repeat": reps, "repeats": repeats,
        "ms": {k: [round(v, 6) for v in vs] for k, vs in ms.items()},
        "median_ms": {k: round(v, 6) for k, v in med.items()},
        "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in ms.items()},
        "r2c_over_complex": round(med["r2c"] / med["complex"], 4),
        "c2r_over_complex": round(med["c2r"] / med["complex"], 4),
        "post_step_ms": round(post_ms, 6), "pre_step_ms": round(pre_ms, 6),
        "post_step_tb_s": round(step_bytes / post_ms * 1e-9, 3), "pre_step_tb_s": round(step_bytes / pre_ms * 1e-9, 3),
        "copy_tb_s": round(step_bytes / med["copy"] * 1e-9, 3),
        "post_over_copy": round(post_ms / med["copy"], 4), "pre_over_copy": round(pre_ms / med["copy"], 4),
        "beyond_caches": step_bytes > (512 << 20), "tol": TOL,
        "ok": post_ms <= TOL * med["copy"] and pre_ms <= TOL * med["copy"],
    }
    for p in (r2c, c2r, cplx):
        p.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the JSON document here")
    ap.add_argument("--repeats", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_real.py needs a GPU")
    rows = [measure(s, a.repeats) for s in SHAPES]
    doc = {"tool": "tools/bench_real.py", "device": torch.cuda.get_device_name(0), "tol": TOL, "shapes": rows,
           "streaming_ok": all(r["ok"] for r in rows if r["beyond_caches"])}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    for r in rows:
        m = r["median_ms"]
        print(f"# {r['shape']}: r2c {m['r2c']:.4f} ms, c2r {m['c2r']:.4f}, complex {m['complex']:.4f} "
              f"(r2c/complex {r['r2c_over_complex']:.3f}, model {r['model_ratio_r2c_over_complex']:.3f}); "
              f"post {r['post_step_ms']:.4f} ms, pre {r['pre_step_ms']:.4f}, copy {m['copy']:.4f} "
              f"(post/copy {r['post_over_copy']:.3f}, pre/copy {r['pre_over_copy']:.3f})", file=sys.stderr)


if __name__ == "__main__":
    main()
