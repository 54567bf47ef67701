"""Generates cs87project-msolano2_amd/csrc/pifft_instances_{0..NPART-1}.inc:
the k_pass<T, R, C, MODE, NTS, LP, VPT> instantiations the planner may pick,
spread over NPART translation units (compiled in parallel).  PK(...) is VPT 16;
PKV(..., VPT) names the values per thread (8 or 32) explicitly.

Rules: NT = C*R/VPT threads (VPT = 16 values per thread) <= 1024; LDS = C*(R + R/16 + 1)*sizeof(T)
<= 160 KiB.  MODE 0 single pass (any C); MODE 1/2 strided passes (C >= 4);
MODE 10 = MODE 2 on the worker-interleaved layout (all-worker plans);
MODE 11 = its first pass with every worker's tree fused in.
MODE 3 = MODE 1 with the tree fused in, LP = log2 P in 1..4, at the planner's
tile (8192 elements, both precisions) and C = 4.  MODE 4 / 6 = MODE 0 / 2
storing in bit-reversed order (the last pass of a PIFFT_OUT_BITREV plan), for
the C the planner can pick (C <= its tile / R).  NTS: 0 plain, 1 non-temporal
loads and stores.

Round 4 removed the measured losers' instances (their logs stay in profiles/,
git keeps the code): the chunked pass pairs (NTS 2/3), MODE 11 (the tree fused
into a worker-interleaved pass), two sub-tiles per workgroup (H = 2), the
all-worker fused tree pass (PIFFT_FUSE_ALL_MAX_MIB) and fp64 strided passes
at C = 2."""
import os

NPART = 8
items = []
for T, prec, esz, tile, vpt in (("double", 64, 8, 8192, 16), ("float", 32, 4, 16384, 16)):
    for lr in range(1, 15):
        R = 1 << lr
        for C in (1, 2, 4, 8, 16, 32, 64):
            if R <= 8 and C != 64:
                continue
            Q = vpt if R >= vpt else min(R, 16)
            nt = C * R // Q
            lds = C * (R + R // 16 + 1) * esz if R > 16 else 0
            if nt > 1024 or lds > 160 * 1024:
                continue
            for nts in (0, 1):
                items.append(f"PK({T}, {prec}, {R}, {C}, 0, {nts}, 0),")
                if C <= max(1, 4096 // R) or R <= 8:
                    items.append(f"PK({T}, {prec}, {R}, {C}, 4, {nts}, 0),")
                if 16 <= R <= 4096 and C >= 4:
                    items.append(f"PK({T}, {prec}, {R}, {C}, 1, {nts}, 0),")
                    items.append(f"PK({T}, {prec}, {R}, {C}, 2, {nts}, 0),")
                    if C <= max(4, tile // R):
                        items.append(f"PK({T}, {prec}, {R}, {C}, 6, {nts}, 0),")
                        # MODE 10 = 2 | 8: the worker-interleaved layout of
                        # all-worker plans (multi-pass local FFTs: R <= 1024;
                        # 2048 at C = 4 for the pass after a fused tree pass,
                        # MODE 11, e.g. config 2's 64 x 2048)
                        if R <= 1024 or (R == 2048 and C == 4):
                            items.append(f"PK({T}, {prec}, {R}, {C}, 10, {nts}, 0),")
                    if R == 2048 and C == 8:  # (its 8-line twin: a row of all 8 workers)
                        items.append(f"PK({T}, {prec}, {R}, {C}, 10, {nts}, 0),")
                # the planner's first-pass tile (tile_elems(): 8192 values for both precisions)
                # (and at half that C for R <= 256: the planner halves C to keep >= 512
                # workgroups on small local sizes, e.g. 2^21 = 128 x 128 x 128)
                cf = max(4, min(64, 8192 // R))
                if 16 <= R <= 2048 and (C == 4 or C == cf or (R <= 256 and C == cf // 2)):
                    for lp in (1, 2, 3, 4):
                        items.append(f"PK({T}, {prec}, {R}, {C}, 3, {nts}, {lp}),")
# the fused tree + first pass at C = 8 / 16 for R = 128-1024 (lines the
# planner's >= 512-workgroup rule picks for batched one-worker plans, e.g. 4 x
# fp64 2^21-2^23 split 4-16 ways)
for T, prec in (("double", 64), ("float", 32)):
    for R in (128, 256, 512, 1024):
        for C in (8, 16):
            if C == max(4, min(64, 8192 // R)) or (R <= 256 and C == max(4, min(64, 8192 // R)) // 2):
                continue  # already instantiated above
            for nts in (0, 1):
                for lp in (1, 2, 3, 4):
                    items.append(f"PK({T}, {prec}, {R}, {C}, 3, {nts}, {lp}),")
# fp32 strided passes at 32 values per thread: a 16384-value tile (the bytes
# and row-segment widths of the fp64 8192-value tile) on 512 threads, two
# workgroups per CU (PIFFT_VPT32; three passes 1024-512-512 at 2^28)
# (R = 512 and 1024: the radices of 2^27-2^30 three-pass plans; 256 and 2048
# spill 44-100 B per lane in this form)
# VPT 32 is float only: the kernels have no other form of it (pass_stages_packed)
for R in (512, 1024):
    C = 16384 // R
    for nts in (0, 1):
        for mode in (1, 2):
            items.append(f"PKV(float, 32, {R}, {C}, {mode}, {nts}, 0, 32),")
# The fused tree pass at 8 values per thread (radix-8 stages, twice the waves
# per workgroup) for small one-worker slices, whose fused launch has <= 128
# workgroups (local 2^15-2^18: R = 256 / 512 at C = 4), both precisions; and
# the worker-interleaved passes of config-2-sized all-worker plans (C = 8).
# Measured on MI355X (profiles/r04d_fused_vpt8.log, r04d_wil_vpt8_c2.log):
# fp64 slices +4.5-31 % (config 2's slice 14.05 -> 12.66 us), fp32 +0.6-4 %,
# config 2 +4 %; R = 1024 fused passes -2-3 % and config 1's strided passes
# -4 % at 8 (r04c_vpt8_c1.log): not instantiated.
for T, prec in (("double", 64), ("float", 32)):
    for R in (256, 512):
        for lp in (1, 2, 3, 4):
            for nts in (0, 1):
                items.append(f"PKV({T}, {prec}, {R}, 4, 3, {nts}, {lp}, 8),")
for R in (256, 512):
    for nts in (0, 1):
        items.append(f"PKV(double, 64, {R}, 8, 10, {nts}, 0, 8),")
# The last strided pass of small fp64 plans (R <= 512, <= 256 workgroups) at
# 8 values per thread (round 4, profiles/r04k_slice.log, r04k_shapes.log:
# config 2's slice +3.8 %, slices of local 2^16-2^19 +1.6-5 %, P = 1
# 2^16-2^18 +5-6 %), and at C = 8 for PIFFT_LAST_C (tuning).
# (4 values per thread: the slice's last pass +2.6 %, below 8; its fused
# tree pass -4 %, local 2^17-2^18 fused passes -6-9 %, +5-7 % only at local
# 2^15-2^16: not instantiated)
for R in (256, 512):
    for C in (4, 8):
        for nts in (0, 1):
            items.append(f"PKV(double, 64, {R}, {C}, 2, {nts}, 0, 8),")
# MODE 11 = 3 | 8: the tree of all P workers fused into the first
# worker-interleaved pass (round 5).  A tile is J adjacent line indices x the P
# workers (C = J P lines) at the 8192-value tile (R = 8192 / C), P = 2..16.
# The planner's J (wil_fuse_tile, pifft_planner.h): fp64 J = 8 (P <= 8, and P = 16 from
# 256 MiB); fp32 J = 8 up to 32 MiB and 16 up to 1 GiB; J = 4 (4096-value tile
# below 256 workgroups, or where J = 8 would split the remainder) and J = 2
# (fp64 P = 16, 32-64 MiB) as refinements below; other J only under
# PIFFT_WIL_FUSE_J (tuning).  Candidates: fp64 J = 16/8/4, fp32 J = 32/16/8.
for T, prec, js in (("double", 64, (16, 8, 4)), ("float", 32, (32, 16, 8))):
    for J in js:
        for lp in (1, 2, 3, 4):
            C = J << lp
            R = 8192 // C
            if R < 16:
                continue
            for nts in (0, 1):
                items.append(f"PK({T}, {prec}, {R}, {C}, 11, {nts}, {lp}),")
# ... and the planner's two refinements for P <= 8 (profiles/r05s-u_*): the
# 4096-value tile at J = 4 for grids of fewer than 256 workgroups (both
# precisions), and fp32 J = 4 at P = 8 (a 2048-point remainder or longer)
for T, prec in (("double", 64), ("float", 32)):
    for lp in (1, 2, 3):
        for nts in (0, 1):
            items.append(f"PK({T}, {prec}, {4096 // (4 << lp)}, {4 << lp}, 11, {nts}, {lp}),")
for nts in (0, 1):
    items.append(f"PK(float, 32, 256, 32, 11, {nts}, 3),")
    items.append(f"PK(float, 32, 128, 64, 11, {nts}, 4),")    # fp32 P = 16, J = 4
    items.append(f"PK(double, 64, 256, 32, 11, {nts}, 4),")   # fp64 P = 16, J = 2
# (fp64 P = 8 at J = 2 / 4096-value tile -- radices 256.512, both passes on
# 256 CUs instead of 128.1024, whose second pass has 128 workgroups: config 2
# 22.2 -> 22.9 us, 2^21 P = 8 33 -> 39 us, 2^19 +1 %; round 6,
# profiles/r06e_c2_j2.txt; not instantiated)
# ... and the one-launch form: a transform of P M <= 8192 values (from 1024)
# as ONE fused pass at J = 1 -- C = P lines of R = M points, every worker's
# tree then its whole M-point FFT, natural-order store (round 5; the
# reference's GPU sweep sizes, n = 1024-8192, p <= 16)
for T, prec in (("double", 64), ("float", 32)):
    for lp in (1, 2, 3, 4):
        for logm in range(10 - lp, min(14 - lp, 12)):  # (M < 4096: fp64 P = 2 at 4096 spills)
            items.append(f"PK({T}, {prec}, {1 << logm}, {1 << lp}, 11, 0, {lp}),")
# (fp32 spills nowhere at M = 4096, P = 2: that one too.  16384-value
# one-launch tiles -- 1024 threads, fp64 2^14 P = 8, fp32 2^14 P = 4 / 8 --
# measured 14-16 vs 9-11 us, profiles/r05za_small_plan_edges.log: not
# instantiated)
items.append("PK(float, 32, 4096, 2, 11, 0, 1),")
items.append("PKV(double, 64, 4096, 2, 11, 0, 1, 8),")  # fp64 P = 2 at 8192 values: 8 per thread, spill-free
# P = 32 (two threads per position, one launch only): n = 1024-4096 fp64 (8192
# spills), 1024-8192 fp32
for T, prec, ms in (("double", 64, (32, 64, 128)), ("float", 32, (32, 64, 128, 256))):
    for m in ms:
        items.append(f"PK({T}, {prec}, {m}, 32, 11, 0, 5),")
# (config 2's slice with its fused tree pass at C = 2 -- 128 workgroups
# gathering leaves, 32-B leaf segments: +0.7 % on the slice, 0 to +2.4 % on
# neighbouring slices, within run-to-run noise; round 4,
# profiles/r04n_fused_c2.log; not instantiated)
# (blocked intermediates between the 2^28 passes -- the reading pass's tile a
# contiguous region -- were built and lost 4-14 %: the writer's scattered
# stores cost more than the reader gained; round 4,
# profiles/r04d_blocked_intermediates.log; not instantiated)
# (a 32768-value tile -- C = 32 at R = 1024, one 1024-thread workgroup per CU,
# 256-B segments -- made the fp32 2^28 last pass 0.88 -> 1.07 ms: round 4,
# profiles/r04_fp32_last_pass_c32.log; not instantiated)
# (8 values per thread -- PKV(..., 8), radix-8 stages -- measured slower than
# 16 for every single pass and batch tried, fp32 4096 x 128..4096 and fp64
# 2^12 / 2^13 x 1..1024 (profiles/r02_vpt_sweep.log): not instantiated)
# Round 6: only the instances some plan launches are compiled.  The rules
# above are the candidates; the kept ones are those the default planner
# launches over its whole domain (tools/instance_sweep.py ->
# tests/golden/instances_default.txt) and those the GPU tests' plans launch
# under their tuning variables (conftest.py's PIFFTTEST_RECORD_INSTANCES ->
# tests/golden/instances_tests.txt from the GPU suite on MI355X,
# instances_tests_cpu.txt from the CPU suite's tuned dry runs).  A tuning variable that asks for a
# dropped instance gets the planner's "no pass kernel" error.
# tests/test_instances.py checks both lists against the built library.
# `--all`: every candidate (to re-derive the lists after a planner change).
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def desc(item: str) -> str:
    m = re.match(r"PK(V?)\((\w+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+)(?:, (\d+))?\),", item)
    prec, R, C, mode, nts, lp = (int(m.group(k)) for k in range(3, 9))
    vpt = int(m.group(9)) if m.group(1) else 16
    return "prec=%d R=%d C=%d mode=%d nts=%d lp=%d vpt=%d" % (prec, R, C, mode, nts, lp, vpt)


keep = set()
for name in ("instances_default.txt", "instances_tests.txt", "instances_tests_cpu.txt"):
    path = os.path.join(ROOT, "tests", "golden", name)
    if os.path.exists(path):
        keep |= {ln.strip() for ln in open(path) if ln.strip()}
candidates = len(items)
if keep and "--all" not in sys.argv:
    items = [it for it in items if desc(it) in keep]
    missing = keep - {desc(it) for it in items}
    assert not missing, f"kept instances no rule generates: {sorted(missing)[:5]}"
print(f"{candidates} candidate instances, {len(items)} kept")
d = os.path.join(ROOT, "cs87project-msolano2_amd", "csrc")
for k in range(NPART):
    with open(os.path.join(d, f"pifft_instances_{k}.inc"), "w") as f:
        f.write(f"// generated by tools/gen_instances.py -- part {k} of {NPART}\n")
        f.write("\n".join(items[k::NPART]) + "\n")
old = os.path.join(d, "pifft_instances.inc")
if os.path.exists(old):
    os.remove(old)
print(len(items), "instances in", NPART, "parts")
