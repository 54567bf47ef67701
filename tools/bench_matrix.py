#!/usr/bin/env python3
"""tools/bench_matrix.py [--out FILE] [--repeats R] [--only SUBSTR] -- what does
a matrix plan (pifft_plan_create_matrix) cost, do its transposes stream at the
rate of a copy, and do its inner chains run as the same 1-D plans run alone?

For each shape below, in one process and on the same buffers:
  (a) the matrix plan, natural and transposed-out,
  (b) the 1-D plan of the rows, (n1, 1 worker, batch n0), alone,
  (c) the 1-D plan of the columns, (n0, 1 worker, batch n1), alone,
  (d) a device-to-device copy of the same batch n0 n1 values
      (torch.Tensor.copy_): as many bytes read and written as one transpose
      launch moves, its yardstick,
  (e) torch.fft.fft2 of the same tensor -- an outside figure, recorded only,
are timed alternately after a warm-up, R repeats each, every repeat a loop of
executions between two device events (medians and the spread (max - min) /
median).  Per-launch durations come from pifft_profile_start(...,
PROFILE_SAMPLED) -- in context, every timed dispatch after untimed ones -- for
the matrix plan and, the same way, for (b) and (c).  Targets (not assertions):
`transpose_over_copy` <= 1.10 at the HBM-sized shapes, `chain_over_alone`
<= 1.03.  One JSON document on stdout and in FILE, the run log beside it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cs87project-msolano2_amd"))

import torch  # noqa: E402  (before libpifft: one HIP runtime)
import pifft  # noqa: E402

TOL_COPY, TOL_CHAIN = 1.10, 1.03
# name, n0, n1, batch, precision, HBM-sized
SHAPES = [
    ("fp32 4096 x 4096", 4096, 4096, 1, 32, False),
    ("fp64 1024 x 1024", 1024, 1024, 1, 64, False),
    ("fp64 8192 x 8192", 8192, 8192, 1, 64, True),
    ("fp32 16384 x 16384", 16384, 16384, 1, 32, True),
    ("fp64 2048 x 8192", 2048, 8192, 1, 64, False),
    ("fp64 8192 x 2048", 8192, 2048, 1, 64, False),
    ("fp32 2048 x 8192", 2048, 8192, 1, 32, False),
    ("fp32 8192 x 2048", 8192, 2048, 1, 32, False),
]
LOG = []


def log(msg):
    LOG.append(msg)
    print("# " + msg, file=sys.stderr, flush=True)


def time_loop(fn, reps):
    st = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def sampled(plan, d_in, d_out, samples):
    """Mean in-context duration (ms) of every launch: PROFILE_SAMPLED, `samples` each."""
    nl = plan.info.num_launches
    st = torch.cuda.current_stream()
    plan.profile_start(2 * nl * samples, pifft.PROFILE_SAMPLED)
    for _ in range(2 * nl * samples):
        plan.execute_device(d_in, d_out, st)
    _, sums, counts = plan.profile_read()
    return [s / c for s, c in zip(sums, counts)]


def measure(shape, repeats):
    name, n0, n1, batch, prec, hbm = shape
    cdt = torch.complex128 if prec == 64 else torch.complex64
    esz = 16 if prec == 64 else 8
    total = batch * n0 * n1
    st = torch.cuda.current_stream()
    x = torch.empty(total, dtype=cdt, device="cuda")
    pifft.generate_device(x.data_ptr(), total, n0 * n1, prec)
    y = torch.empty_like(x)
    plans = {
        "matrix": pifft.MatrixPlan(n0, n1, batch, prec),
        "matrix_transposed_out": pifft.MatrixPlan(n0, n1, batch, prec, transposed_out=True),
        "rows": pifft.Plan(n1, 1, batch * n0, prec),
        "cols": pifft.Plan(n0, 1, batch * n1, prec),
    }
    runs = {k: (lambda p=p: p.execute_device(x.data_ptr(), y.data_ptr(), st)) for k, p in plans.items()}
    runs["copy"] = lambda: y.copy_(x)
    x2 = x.view(batch, n0, n1)
    try:
        torch.fft.fft2(x2)
        runs["torch_fft2"] = lambda: torch.fft.fft2(x2)
    except RuntimeError as e:  # (an outside figure: its absence is recorded, nothing else depends on it)
        log(f"{name}: torch.fft.fft2 failed: {str(e).splitlines()[0]}")
    reps = {}
    for k, fn in runs.items():  # loops of >= ~20 ms (at least 10 executions), sized on a first timing
        est = min(time_loop(fn, 5) for _ in range(2))
        reps[k] = max(10, int(20.0 / max(est, 1e-3)))
        time_loop(fn, reps[k])  # warm-up
    ms = {k: [] for k in runs}
    for _ in range(repeats):
        for k, fn in runs.items():
            ms[k].append(time_loop(fn, reps[k]))
    med = {k: statistics.median(v) for k, v in ms.items()}
    samples = max(8, min(64, int(40.0 / max(med["matrix"], 1e-3))))
    launch_ms = {k: sampled(p, x.data_ptr(), y.data_ptr(), samples) for k, p in plans.items()}
    d = plans["matrix"].describe()
    nr = plans["rows"].info.num_launches
    kinds = d["launch_kind"]
    assert kinds[nr] == "transpose" and kinds[-1] == "transpose" and d["launch_bytes"][nr] == 2 * total * esz
    lm = launch_ms["matrix"]
    rows_in, cols_in = sum(lm[:nr]), sum(lm[nr + 1:-1])
    rows_alone, cols_alone = sum(launch_ms["rows"]), sum(launch_ms["cols"])
    t_ms = [lm[nr], lm[-1]]
    out = {
        "shape": name, "n0": n0, "n1": n1, "batch": batch, "prec": prec, "hbm_sized": hbm,
        "launch_kind": kinds, "kernels": [plans["matrix"].kernel_name(i) for i in range(len(kinds))],
        "transpose_grid": [plans["matrix"].launch_grid(nr), plans["matrix"].launch_grid(len(kinds) - 1)],
        "transpose_bytes": 2 * total * esz, "workspace_bytes": d["workspace_bytes"],
        "executions_per_repeat": reps, "repeats": repeats, "samples_per_launch": samples,
        "ms": {k: [round(v, 6) for v in vs] for k, vs in ms.items()},
        "median_ms": {k: round(v, 6) for k, v in med.items()},
        "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in ms.items()},
        "launch_ms": {k: [round(v, 6) for v in vs] for k, vs in launch_ms.items()},
        "transpose_ms": [round(v, 6) for v in t_ms],
        "transpose_tb_s": [round(2 * total * esz / v * 1e-9, 3) for v in t_ms],
        "copy_tb_s": round(2 * total * esz / med["copy"] * 1e-9, 3),
        "transpose_over_copy": [round(v / med["copy"], 4) for v in t_ms],
        "transpose_share": round(sum(t_ms) / sum(lm), 4),
        "chain_ms": {"rows_in_matrix": round(rows_in, 6), "rows_alone": round(rows_alone, 6),
                     "cols_in_matrix": round(cols_in, 6), "cols_alone": round(cols_alone, 6)},
        "chain_over_alone": [round(rows_in / rows_alone, 4), round(cols_in / cols_alone, 4)],
        "matrix_over_parts": round(med["matrix"] / (med["rows"] + med["cols"] + 2 * med["copy"]), 4),
        "tol_copy": TOL_COPY, "tol_chain": TOL_CHAIN,
        "transpose_ok": all(v <= TOL_COPY * med["copy"] for v in t_ms),
        "chains_ok": rows_in <= TOL_CHAIN * rows_alone and cols_in <= TOL_CHAIN * cols_alone,
    }
    for p in plans.values():
        p.close()
    m = out["median_ms"]
    log(f"{name}: matrix {m['matrix']:.4f} ms (transposed-out {m['matrix_transposed_out']:.4f}), rows {m['rows']:.4f}, "
        f"cols {m['cols']:.4f}, copy {m['copy']:.4f}, torch fft2 {m.get('torch_fft2', float('nan')):.4f}; "
        f"launches {[round(v, 4) for v in lm]}; transpose/copy {out['transpose_over_copy']}, "
        f"chain/alone {out['chain_over_alone']}, spread {out['spread']}")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the JSON document here (the run log beside it, .log)")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--only", help="shapes whose name contains this")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_matrix.py needs a GPU")
    log(f"device {torch.cuda.get_device_name(0)}, repeats {a.repeats}")
    rows = []
    for s in SHAPES:
        if a.only and a.only not in s[0]:
            continue
        rows.append(measure(s, a.repeats))
        torch.cuda.empty_cache()
    doc = {"tool": "tools/bench_matrix.py", "device": torch.cuda.get_device_name(0), "tol_copy": TOL_COPY,
           "tol_chain": TOL_CHAIN, "shapes": rows,
           "transposes_stream": all(r["transpose_ok"] for r in rows if r["hbm_sized"]),
           "chains_as_alone": all(r["chains_ok"] for r in rows)}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
        with open(os.path.splitext(a.out)[0] + ".log", "w") as f:
            f.write("\n".join(LOG) + "\n")


if __name__ == "__main__":
    main()
