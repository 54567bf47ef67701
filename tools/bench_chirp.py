#!/usr/bin/env python3
"""tools/bench_chirp.py [--out FILE] [--repeats R] [--only SUBSTR] -- what does
a chirp plan (pifft_plan_create_chirp) cost, do its three streaming kernels move
their bytes at the rate of a copy, and do its inner chains run as the same 1-D
plans run alone?

For each shape below, in one process and on the same buffers:
  (a) the chirp plan of N values,
  (b) the 1-D plan of (M, 1 worker, batch 1), M = chirp_length(N), forward, alone,
  (c) the same plan with PIFFT_INVERSE, alone,
  (d) per new launch, a device-to-device copy (torch.Tensor.copy_) that reads
      and writes as many bytes in all as the launch's launch_bytes: its yardstick,
  (e) torch.fft.fft of the same N values -- an outside figure, recorded only,
are timed alternately after a warm-up, R repeats each, every repeat a loop of
executions between two device events (medians and the spread (max - min) /
median).  Per-launch durations come from pifft_profile_start(...,
PROFILE_SAMPLED) -- in context, every timed dispatch after untimed ones -- for
the chirp plan and, the same way, for (b) and (c).  The time of
pifft_plan_create_chirp (synchronous: it computes Bt on the device) is a host
clock around the constructor.  Targets (not assertions): `kernel_over_copy`
<= 1.10 at the HBM-sized shape, `chain_over_alone` <= 1.03.  One JSON document
on stdout and in FILE, the run log beside it."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cs87project-msolano2_amd"))

import torch  # noqa: E402  (before libpifft: one HIP runtime)
import pifft  # noqa: E402

TOL_COPY, TOL_CHAIN = 1.10, 1.03
# name, N, precision, HBM-sized
SHAPES = [(f"fp{prec} N={n}", n, prec, n == 10 ** 8) for n in (10 ** 8, 1000003, 10007) for prec in (64, 32)]
NEW = ("chirp_pre", "spectrum_mul", "chirp_post")
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
    name, n, prec, hbm = shape
    cdt = torch.complex128 if prec == 64 else torch.complex64
    m = pifft.chirp_length(n)
    st = torch.cuda.current_stream()
    x = torch.empty(n, dtype=cdt, device="cuda")
    pifft.generate_device(x.data_ptr(), n, n, prec)
    y = torch.empty_like(x)
    xm = torch.empty(m, dtype=cdt, device="cuda")  # the chains alone: M values in, M out
    pifft.generate_device(xm.data_ptr(), m, m, prec)
    ym = torch.empty_like(xm)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    chirp = pifft.ChirpPlan(n, 1, prec)
    create_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    pifft.ChirpPlan(n, 1, prec).close()
    create_again_ms = (time.perf_counter() - t0) * 1e3
    plans = {"chirp": chirp, "fwd": pifft.Plan(m, 1, 1, prec, device=0),
             "inv": pifft.Plan(m, 1, 1, prec, device=0, inverse=True)}
    bufs = {"chirp": (x, y), "fwd": (xm, ym), "inv": (xm, ym)}
    runs = {k: (lambda p=p, a=bufs[k][0], b=bufs[k][1]: p.execute_device(a.data_ptr(), b.data_ptr(), st))
            for k, p in plans.items()}
    d = chirp.describe()
    kinds = d["launch_kind"]
    at = {k: kinds.index(k) for k in NEW}
    copies = {}
    for k in NEW:  # a copy reading and writing launch_bytes in all
        half = d["launch_bytes"][at[k]] // 2
        copies[k] = (torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda"))
        copies[k][0].zero_()
        runs["copy_" + k] = lambda s=copies[k][0], t=copies[k][1]: t.copy_(s)
    try:
        torch.fft.fft(x)
        runs["torch_fft"] = lambda: torch.fft.fft(x)
    except RuntimeError as e:  # (an outside figure: its absence is recorded, nothing else depends on it)
        log(f"{name}: torch.fft.fft failed: {str(e).splitlines()[0]}")
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
    samples = max(8, min(64, int(40.0 / max(med["chirp"], 1e-3))))
    launch_ms = {k: sampled(p, bufs[k][0].data_ptr(), bufs[k][1].data_ptr(), samples) for k, p in plans.items()}
    lm = launch_ms["chirp"]
    nf = plans["fwd"].info.num_launches
    assert at["chirp_pre"] == 0 and at["spectrum_mul"] == 1 + nf and at["chirp_post"] == len(kinds) - 1
    fwd_in, inv_in = sum(lm[1:1 + nf]), sum(lm[2 + nf:-1])
    fwd_alone, inv_alone = sum(launch_ms["fwd"]), sum(launch_ms["inv"])
    new = {k: {"launch": at[k], "bytes": d["launch_bytes"][at[k]], "grid": chirp.launch_grid(at[k]),
               "ms": round(lm[at[k]], 6), "tb_s": round(d["launch_bytes"][at[k]] / lm[at[k]] * 1e-9, 3),
               "copy_ms": round(med["copy_" + k], 6),
               "copy_tb_s": round(d["launch_bytes"][at[k]] / med["copy_" + k] * 1e-9, 3),
               "kernel_over_copy": round(lm[at[k]] / med["copy_" + k], 4)} for k in NEW}
    out = {
        "shape": name, "n": n, "m": m, "prec": prec, "hbm_sized": hbm,
        "launch_kind": kinds, "kernels": [chirp.kernel_name(i) for i in range(len(kinds))],
        "workspace_bytes": d["workspace_bytes"], "create_ms": round(create_ms, 3),
        "create_again_ms": round(create_again_ms, 3),
        "executions_per_repeat": reps, "repeats": repeats, "samples_per_launch": samples,
        "ms": {k: [round(v, 6) for v in vs] for k, vs in ms.items()},
        "median_ms": {k: round(v, 6) for k, v in med.items()},
        "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in ms.items()},
        "launch_ms": {k: [round(v, 6) for v in vs] for k, vs in launch_ms.items()},
        "new_launches": new,
        "new_share": round(sum(lm[at[k]] for k in NEW) / sum(lm), 4),
        "chain_ms": {"fwd_in_chirp": round(fwd_in, 6), "fwd_alone": round(fwd_alone, 6),
                     "inv_in_chirp": round(inv_in, 6), "inv_alone": round(inv_alone, 6)},
        "chain_over_alone": [round(fwd_in / fwd_alone, 4), round(inv_in / inv_alone, 4)],
        "chirp_over_torch_fft": round(med["chirp"] / med["torch_fft"], 4) if "torch_fft" in med else None,
        "tol_copy": TOL_COPY, "tol_chain": TOL_CHAIN,
        "kernels_ok": all(v["kernel_over_copy"] <= TOL_COPY for v in new.values()),
        "chains_ok": fwd_in <= TOL_CHAIN * fwd_alone and inv_in <= TOL_CHAIN * inv_alone,
    }
    for p in plans.values():
        p.close()
    mm = out["median_ms"]
    log(f"{name}: chirp {mm['chirp']:.4f} ms, fwd {mm['fwd']:.4f}, inv {mm['inv']:.4f}, "
        f"torch fft {mm.get('torch_fft', float('nan')):.4f}, create {create_ms:.1f} ms (again {create_again_ms:.1f}); "
        f"launches {[round(v, 4) for v in lm]}; kernel/copy "
        f"{ {k: v['kernel_over_copy'] for k, v in new.items()} }, chain/alone {out['chain_over_alone']}, "
        f"spread {out['spread']}")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the JSON document here (the run log beside it, .log)")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--only", help="shapes whose name contains this")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_chirp.py needs a GPU")
    log(f"device {torch.cuda.get_device_name(0)}, repeats {a.repeats}")
    rows = []
    for s in SHAPES:
        if a.only and a.only not in s[0]:
            continue
        rows.append(measure(s, a.repeats))
        torch.cuda.empty_cache()
        if a.out:  # (kept after every shape: a long run leaves what it has)
            write(a.out, rows)
    print(json.dumps(document(rows), indent=1))


def document(rows):
    return {"tool": "tools/bench_chirp.py", "device": torch.cuda.get_device_name(0), "tol_copy": TOL_COPY,
            "tol_chain": TOL_CHAIN, "shapes": rows,
            "kernels_stream": all(r["kernels_ok"] for r in rows if r["hbm_sized"]),
            "chains_as_alone": all(r["chains_ok"] for r in rows)}


def write(path, rows):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(document(rows), indent=1) + "\n")
    with open(os.path.splitext(path)[0] + ".log", "w") as f:
        f.write("\n".join(LOG) + "\n")


if __name__ == "__main__":
    main()
