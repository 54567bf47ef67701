#!/usr/bin/env python3
"""tools/bench_conv.py [--out FILE] [--repeats R] [--only SUBSTR] -- what does a
convolution plan (pifft_plan_create_conv) cost against the same filtering put
together by hand, and do its three new kernels move their bytes at the rate of
a copy?

For each shape below, in one process and on the same input:
  (a) the convolution plan (linear, L = M: n = M - taps + 1),
  (b) the composition through the rest of the public interface: a torch pad to
      M reals, RealPlan R2C, a torch complex product with the filter's spectrum
      (RealPlan R2C of the padded filter / M, computed once), RealPlan C2R, a
      torch crop to L,
  (c) torch.fft.irfft(torch.fft.rfft(x, M) * torch.fft.rfft(h, M), M)[:, :L], and
      the same with rfft(h, M) computed once, outside the loop,
  (d) per new launch, a device-to-device copy (torch.Tensor.copy_) that reads
      and writes as many bytes in all as the launch's launch_bytes: its yardstick,
are timed alternately after a warm-up, R repeats each, every repeat a loop of
executions between two device events (medians and the spread (max - min) /
median).  Per-launch durations come from pifft_profile_start(...,
PROFILE_SAMPLED) -- in context, every timed dispatch after untimed ones.  The
three results are compared on the way (max difference over the result's rms).
Target (not an assertion): `kernel_over_copy` <= 1.10 at the HBM-sized shape.
One JSON document on stdout and in FILE, the run log beside it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cs87project-msolano2_amd"))

import torch  # noqa: E402  (before libpifft: one HIP runtime)
import pifft  # noqa: E402

TOL_COPY = 1.10
# name, M, taps, batch, precision, HBM-sized
SHAPES = [(f"fp{prec} M=2^{logm} batch={batch}", 1 << logm, taps, batch, prec, logm == 26)
          for logm, taps, batch in ((12, 65, 4096), (26, 1025, 1)) for prec in (32, 64)]
NEW = ("conv_pad", "conv_pair", "conv_crop")
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
    name, m, taps, batch, prec, hbm = shape
    rdt = torch.float64 if prec == 64 else torch.float32
    cdt = torch.complex128 if prec == 64 else torch.complex64
    n, L, h2 = m - taps + 1, m, m // 2
    st = torch.cuda.current_stream()
    g = torch.Generator(device="cuda").manual_seed(0xC0F0 + m)
    x = (torch.rand(batch, n, dtype=rdt, device="cuda", generator=g) * 2 - 1) / n ** 0.5
    h = (torch.rand(taps, dtype=rdt, device="cuda", generator=g) * 2 - 1) / taps ** 0.5
    y = torch.empty(batch, L, dtype=rdt, device="cuda")
    conv = pifft.ConvPlan(n, taps, batch, prec)
    conv.set_filter(h.data_ptr(), st)
    # (b): the pieces a caller has without the plan
    r2c, c2r = pifft.RealPlan(m, 1, batch, prec), pifft.RealPlan(m, 1, batch, prec, inverse=True)
    r2c1 = pifft.RealPlan(m, 1, 1, prec)
    hp = torch.nn.functional.pad(h, (0, m - taps)) * (1.0 / m)
    G = torch.empty(h2 + 1, dtype=cdt, device="cuda")
    r2c1.execute_device(hp.data_ptr(), G.data_ptr(), st)
    X = torch.empty(batch, h2 + 1, dtype=cdt, device="cuda")
    yb = torch.empty(batch, m, dtype=rdt, device="cuda")
    keep = {}

    def composed():
        xp = torch.nn.functional.pad(x, (0, m - n))
        r2c.execute_device(xp.data_ptr(), X.data_ptr(), st)
        P = X * G
        c2r.execute_device(P.data_ptr(), yb.data_ptr(), st)
        keep["composed"] = yb[:, :L].contiguous()

    Hf = torch.fft.rfft(h, m)

    def torch_fft():
        keep["torch_fft"] = torch.fft.irfft(torch.fft.rfft(x, m) * torch.fft.rfft(h, m), m)[:, :L]

    def torch_fft_filter_once():
        keep["torch_fft_once"] = torch.fft.irfft(torch.fft.rfft(x, m) * Hf, m)[:, :L]

    runs = {"conv": lambda: conv.execute_device(x.data_ptr(), y.data_ptr(), st), "composed": composed}
    for k, fn in (("torch_fft", torch_fft), ("torch_fft_filter_once", torch_fft_filter_once)):
        try:
            fn()
            runs[k] = fn
        except RuntimeError as e:  # (an outside figure: its absence is recorded, nothing else depends on it)
            log(f"{name}: {k} failed: {str(e).splitlines()[0]}")
    d = conv.describe()
    kinds = d["launch_kind"]
    at = {k: kinds.index(k) for k in NEW}
    copies = {}
    for k in NEW:  # a copy reading and writing launch_bytes in all
        half = d["launch_bytes"][at[k]] // 2
        copies[k] = (torch.zeros(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda"))
        runs["copy_" + k] = lambda s=copies[k][0], t=copies[k][1]: t.copy_(s)
    # the three results on the same input
    runs["conv"](), composed()
    torch.cuda.synchronize()
    rms = float(y.double().pow(2).mean().sqrt())
    agree = {k: float((v.double() - y.double()).abs().max()) / rms for k, v in keep.items()}
    keep.clear()
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
    samples = max(8, min(64, int(40.0 / max(med["conv"], 1e-3))))
    lm = sampled(conv, x.data_ptr(), y.data_ptr(), samples)
    xp = torch.nn.functional.pad(x, (0, m - n))
    fix = {"r2c": sampled(r2c, xp.data_ptr(), X.data_ptr(), samples)[-1],
           "c2r": sampled(c2r, X.data_ptr(), yb.data_ptr(), samples)[0]}
    new = {k: {"launch": at[k], "bytes": d["launch_bytes"][at[k]], "grid": conv.launch_grid(at[k]),
               "ms": round(lm[at[k]], 6), "tb_s": round(d["launch_bytes"][at[k]] / lm[at[k]] * 1e-9, 3),
               "copy_ms": round(med["copy_" + k], 6),
               "copy_tb_s": round(d["launch_bytes"][at[k]] / med["copy_" + k] * 1e-9, 3),
               "kernel_over_copy": round(lm[at[k]] / med["copy_" + k], 4)} for k in NEW}
    out = {
        "shape": name, "m": m, "n": n, "taps": taps, "batch": batch, "prec": prec, "hbm_sized": hbm,
        "launch_kind": kinds, "kernels": [conv.kernel_name(i) for i in range(len(kinds))],
        "workspace_bytes": d["workspace_bytes"],
        "executions_per_repeat": reps, "repeats": repeats, "samples_per_launch": samples,
        "ms": {k: [round(v, 6) for v in vs] for k, vs in ms.items()},
        "median_ms": {k: round(v, 6) for k, v in med.items()},
        "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in ms.items()},
        "launch_ms": [round(v, 6) for v in lm],
        "new_launches": new,
        "new_share": round(sum(lm[at[k]] for k in NEW) / sum(lm), 4),
        # the fused pair launch against the two fix-up launches it replaces (in context of their real plans;
        # the composition's pointwise product comes on top of them)
        "fixup_ms": {k: round(v, 6) for k, v in fix.items()},
        "pair_over_fixups": round(lm[at["conv_pair"]] / (fix["r2c"] + fix["c2r"]), 4),
        "max_difference_over_rms": {k: float(f"{v:.3e}") for k, v in agree.items()},
        "conv_over_composed": round(med["conv"] / med["composed"], 4),
        "conv_over_torch_fft": round(med["conv"] / med["torch_fft"], 4) if "torch_fft" in med else None,
        "conv_over_torch_fft_filter_once":
            round(med["conv"] / med["torch_fft_filter_once"], 4) if "torch_fft_filter_once" in med else None,
        "tol_copy": TOL_COPY,
        "kernels_ok": all(v["kernel_over_copy"] <= TOL_COPY for v in new.values()),
    }
    for p in (conv, r2c, c2r, r2c1):
        p.close()
    mm = out["median_ms"]
    log(f"{name}: conv {mm['conv']:.4f} ms, composed {mm['composed']:.4f}, torch fft "
        f"{mm.get('torch_fft', float('nan')):.4f} (filter once {mm.get('torch_fft_filter_once', float('nan')):.4f}); "
        f"launches {[round(v, 4) for v in lm]}; kernel/copy { {k: v['kernel_over_copy'] for k, v in new.items()} }, "
        f"pair / (r2c + c2r fix-ups) {out['pair_over_fixups']}, differences {out['max_difference_over_rms']}, "
        f"spread {out['spread']}")
    return out


def document(rows):
    return {"tool": "tools/bench_conv.py", "device": torch.cuda.get_device_name(0), "tol_copy": TOL_COPY,
            "shapes": rows, "kernels_stream": all(r["kernels_ok"] for r in rows if r["hbm_sized"])}


def write(path, rows):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(document(rows), indent=1) + "\n")
    with open(os.path.splitext(path)[0] + ".log", "w") as f:
        f.write("\n".join(LOG) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the JSON document here (the run log beside it, .log)")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--only", help="shapes whose name contains this")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_conv.py needs a GPU")
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


if __name__ == "__main__":
    main()
