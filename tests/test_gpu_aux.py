"""Every auxiliary kernel and swapping twin on an MI355X, and the second and
later trips of their grid-stride loops.

The auxiliary kernels are what libpifft compiles beside k_pass: k_tree and
k_tree_wil (L = 1..4), k_interleave and k_interleave_tile, their swapping twins
(inverse plans), the real plans' fix-ups k_r2c_post / k_c2r_pre and k_generate
-- 62 kernels, 60 of which a plan can launch (pifft.aux_kernels(), the
library's own registry; tests/test_aux_cases.py).  They move data or do a
handful of flops, so they are held to exact answers wherever one exists.

test_row: every row of tests/golden/aux_cases.tsv (tools/aux_cases.py: per
  kernel the smallest plan that launches it; 58 of the 60, the other two in
  aux_cases_exceptions.txt), built under the row's tuning variables.
  plan.kernel_name of each covered launch is the name built from the registry
  descriptor.  The execution goes through test_gpu_accuracy.run (the sentinel
  tail behind d_out survives, d_in keeps its bits) and
    - against fft_hp under test_gpu_accuracy.check with its bounds (rel-L2 4,
      worst bin 4, or 6 for fp32 and C2R plans of two or more passes);
    - a plan of tree launches only (M = 1; slices or bit-reversed order), bit
      for bit against oracle.tree_segment (every worker of every row; of the
      2^16-worker plans of test_second_trips 258 workers, tree_segment being
      O(N) per worker) and under check against tree_hp;
    - an inverse plan, bit for bit swap(forward(swap(x))), and check against
      the index-reversed references;
    - a forward complex plan, the three exact inputs (assert_exact);
    - a plan with an interleave launch: its output is, bit for bit, the
      permutation out[b N + bitrev_P(q) + P k] = in[b N + q M + k] of the
      slice-major plan's of the same shape, flags and variables, and
      pifft_interleave_device at that (N, P, batch) moves index-encoding
      values exactly so.
test_tree_device: pifft_tree_device per L and range form against tree_segment.
test_interleave_rule_ends: pifft_interleave_device at both ends of
  interleave_tiled's rule (fp64 from log2 P = 5, fp32 from 1, up to 11, from
  N = 2048), and which kernel the matching plan launches.
test_generate: pifft_generate_device against oracle.generate, bit for bit.
test_second_trips*: one smallest case per family, precision and SW under
  PIFFT_STRIDE_GRID_MAX = 1, 3 and one less than the uncapped grid.  Before
  each run the launch description (pifft.dry_run_aux) must show the capped
  grid below the workgroups the work needs -- at least two trips of the loop
  -- and, at 3, a workgroup count that is no multiple of 3; the capped output
  equals the uncapped one bit for bit, which is held to its reference first.
  k_tree_sw<T, L, 3> has no such run: the one launch that both reads d_in and
  writes d_out is the whole plan of N = P <= 16, at most 24 work items at
  batch 3 -- one workgroup, whatever the cap.

Every case has at most 2^16 values and batch <= 3.
"""
import functools
import os
import sys

import numpy as np
import pytest

import pifft
import pifft_oracle as oracle
import test_gpu_accuracy as acc
import test_gpu_real as real_tests
from test_gpu_instances import reversed_index, swap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import aux_cases as ac  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SUF = {32: "f32", 64: "f64"}
NAT, SL, BR, SEP = acc.NAT, acc.SL, acc.BR, acc.SEP
TREE, TREE_WIL, IL, IL_TILE = pifft.AUX_TREE, pifft.AUX_TREE_WIL, pifft.AUX_INTERLEAVE, pifft.AUX_INTERLEAVE_TILE
R2C, C2R = pifft.AUX_R2C, pifft.AUX_C2R
ROWS = ac.read_cases()


@functools.lru_cache(maxsize=None)
def table():
    return [tuple(d) for d in pifft.aux_kernels()]


def log2(x):
    return x.bit_length() - 1


def bitrev(q, bits):
    return int(format(q, "0%db" % bits)[::-1], 2) if bits else 0


# -------------------------------------------------------------- interleave ---
def natural_of_slices(sl, n, P, batch):
    """out[b N + bitrev_P(q) + P k] = in[b N + q M + k], as an index operation."""
    m, lp = n // P, log2(P)
    out = np.empty_like(sl)
    o, s = out.reshape(batch, m, P), sl.reshape(batch, P, m)
    for q in range(P):
        o[:, :, bitrev(q, lp)] = s[:, q, :]
    return out


def run_interleave(n, P, batch, suf):
    """pifft_interleave_device on values that encode their own index (exact in
    fp32 up to 2^23), with the sentinel tail; the output's bytes after the
    element-by-element check."""
    j = np.arange(batch * n, dtype=np.float64)
    src = (j - 1j * (j + 0.5)).astype(acc.DT[suf])
    d_in = acc.dev(src)
    out = torch.full((batch * n + acc.TAIL,), complex(acc.SENTINEL, acc.SENTINEL), dtype=d_in.dtype, device="cuda")
    torch.cuda.synchronize()
    pifft.interleave_device(d_in.data_ptr(), out.data_ptr(), n, P, batch, acc.PREC[suf], torch.cuda.current_stream())
    torch.cuda.synchronize()
    tail = torch.view_as_real(out[batch * n:]).cpu().numpy()
    assert (tail == tail.dtype.type(acc.SENTINEL)).all(), "the sentinel behind d_out was overwritten"
    assert d_in.cpu().numpy().tobytes() == src.tobytes(), "d_slices was written"
    got = out[:batch * n].cpu().numpy()
    want = natural_of_slices(src, n, P, batch)
    assert got.tobytes() == want.tobytes(), f"{np.count_nonzero(got != want)} of {got.size} values misplaced"
    return got.tobytes()


def tiled(prec, n, P):
    """interleave_tiled's rule (csrc/pifft.hip)."""
    return (5 if prec == 64 else 1) <= log2(P) <= 11 and n >= 2048


# ------------------------------------------------------------- one case ---
def make(c):
    if c.direction in ("r2c", "c2r"):
        return pifft.RealPlan(c.n, c.P, c.batch, c.prec, inverse=c.direction == "c2r")
    return pifft.Plan(c.n, c.P, c.batch, c.prec, first=c.first, count=c.count, device=0, flags=c.flags,
                      inverse=c.direction == "inv")


def real_input(c):
    suf, logn = SUF[c.prec], log2(c.n)
    if c.direction == "r2c":
        return oracle.generate(c.n, acc.DT[suf], count=c.batch * c.n // 2)  # = real_tests.device_input, bit for bit
    return np.array(real_tests.reference_c2r(suf, logn, c.batch)[0])


def plain_run(c):
    """The case's output bytes, nothing but test_gpu_accuracy.run's own checks."""
    if c.direction in ("r2c", "c2r"):
        return acc.run(make(c), acc.dev(real_input(c))).tobytes()
    x, _, _ = acc.references(SUF[c.prec], log2(c.n), c.batch)
    return acc.run(make(c), acc.dev(x)).tobytes()


def checked_real(c, plan, label):
    """test_gpu_accuracy's test_r2c / test_c2r on this plan."""
    suf, logn, batch = SUF[c.prec], log2(c.n), c.batch
    n, h = c.n, c.n // 2
    if c.direction == "r2c":
        z = real_input(c)
        x = z.view(acc.RDT[suf]).reshape(batch, n)
        H = np.stack([acc.hp(r.astype(acc.DT[suf]))[:h + 1] for r in x])
        O = np.array(real_tests.reference_r2c(suf, logn, batch)).reshape(batch, h + 1)
        got = acc.run(plan, acc.dev(z))
        acc.check(label, suf, got.reshape(batch, h + 1), H, O, plan.info.num_passes)
        return got.tobytes()
    X, y = real_tests.reference_c2r(suf, logn, batch)
    Xr = np.array(X).reshape(batch, h + 1)
    H = np.stack([acc.hp(np.conj(np.concatenate([r, np.conj(r[h - 1:0:-1])]))).real.astype(np.clongdouble) for r in Xr])
    got = acc.run(plan, acc.dev(X))
    acc.check(label, suf, got.view(acc.RDT[suf]).reshape(batch, n), H, np.array(y).reshape(batch, n),
              plan.info.num_passes, c2r=True)
    return got.tobytes()


def checked_run(c, cov=()):
    """Build, name, run and hold the case to its references (the module
    docstring's list); the output's bytes."""
    label = f"aux {ac.case_id(c)}"
    plan = make(c)
    for i, desc in cov:
        assert plan.kernel_name(i) == pifft.aux_kernel_name(desc), (i, desc)
    if c.direction in ("r2c", "c2r"):
        return checked_real(c, plan, label)
    suf, logn, inverse = SUF[c.prec], log2(c.n), c.direction == "inv"
    shape = (logn, c.P, c.first, c.count, c.flags, c.batch)
    d = plan.describe()
    assert d["inverse"] == inverse
    x, H, O = acc.references(suf, logn, c.batch)
    got = acc.run(plan, acc.dev(x))
    if inverse:
        fwd = acc.make_plan(suf, shape)
        want = swap(acc.run(fwd, acc.dev(swap(x))))
        assert got.tobytes() == want.tobytes(), "the inverse plan is not swap(forward(swap(x))) bit for bit"
        H, O = reversed_index(H), reversed_index(O)
    order = lambda A: np.stack([acc.plan_order(a, c.P, c.first, c.count, c.flags) for a in A])  # noqa: E731
    acc.check(label, suf, got.reshape(c.batch, -1), order(H), order(O), plan.info.num_passes)
    m = c.n // c.P
    rows = [x[b * c.n:(b + 1) * c.n] for b in range(c.batch)]
    if set(d["launch_kind"]) == {"tree"} and not inverse:  # M = 1: the output is the tree's segments, in either order
        assert m == 1 and (c.flags & 3) in (SL, BR)
        # (tree_segment walks one worker's path in O(N): every worker up to 1024 of them -- every row of
        # the table --, beyond that 258 spread over the range; check below still sees every value)
        qs = list(range(c.first, c.first + c.count))
        if c.count > 1024:
            qs = sorted(set(qs[::c.count // 256] + qs[:1] + qs[-1:]))
        g = got.reshape(c.batch, c.count)
        for b, r in enumerate(rows):
            seg = np.concatenate([oracle.tree_segment(r, c.P, q) for q in qs])
            assert g[b, [q - c.first for q in qs]].tobytes() == seg.tobytes(), "the tree is not oracle.tree_segment bit for bit"
        Th = np.stack([oracle.tree_hp(r, c.P)[c.first * m:(c.first + c.count) * m] for r in rows])
        acc.check(label + " tree_hp", suf, g, Th, order(O))
    if not inverse:
        acc.assert_exact(plan, suf, shape)
    if "interleave" in d["launch_kind"]:
        assert d["launch_kind"][-1] == "interleave" and d["launch_kind"].count("interleave") == 1
        sl = acc.make_plan(suf, (logn, c.P, 0, c.P, SL | (c.flags & SEP), c.batch), inverse=inverse)
        ds = sl.describe()
        assert (ds["launch_kind"], ds["radix"], ds["lines"], ds["vpt"]) == \
            (d["launch_kind"][:-1], d["radix"], d["lines"], d["vpt"]), "the slice-major plan is the same plan but for the interleave"
        want = natural_of_slices(acc.run(sl, acc.dev(x)), c.n, c.P, c.batch)
        assert got.tobytes() == want.tobytes(), "the interleave launch is not an exact permutation of the slices"
        name = plan.kernel_name(len(d["launch_kind"]) - 1)
        assert name.startswith("void pifft::k_interleave_tile" if tiled(c.prec, c.n, c.P) else "void pifft::k_interleave<"
                               if not inverse else "void pifft::k_interleave_sw<"), name
        run_interleave(c.n, c.P, c.batch, suf)
    return got.tobytes()


@pytest.mark.parametrize("row", ROWS, ids=lambda r: ac.case_id(r[0]))
def test_row(row, monkeypatch):
    c, cov = row
    for k, v in c.env:
        monkeypatch.setenv(k, v)
    checked_run(c, cov)


# ------------------------------------------------------ pifft_tree_device ---
@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_tree_device(suf, L):
    """k_tree<T, L> alone (N = 2^10, P = 2^L, batch 3): all workers, one
    worker, an aligned sub-range -- each bit for bit oracle.tree_segment."""
    logn, P, batch = 10, 1 << L, 3
    n = 1 << logn
    x, _, _ = acc.references(suf, logn, batch)
    rows = [x[b * n:(b + 1) * n] for b in range(batch)]
    for first, count in sorted({(0, P), (P - 1, 1), (P // 2, max(P // 2, 1))}):
        plan = acc.make_plan(suf, (logn, P, first, count, SL, batch))
        ids = pifft.dry_run_aux(n, P, batch, acc.PREC[suf], first=first, count=count, flags=SL)
        assert table()[ids[0][0]] == (TREE, acc.PREC[suf], L, 0) or count == 1  # (one worker: the fused first pass)
        got = acc.run(plan, acc.dev(x), tree=True)
        want = np.concatenate([oracle.tree_segment(r, P, q) for r in rows for q in range(first, first + count)])
        assert got.tobytes() == want.tobytes(), (first, count)


# ------------------------------------------------ interleave_tiled's ends ---
RULE_ENDS = [(10, 1), (11, 1), (11, 4), (11, 5), (11, 11), (12, 11), (12, 12), (13, 12), (14, 7)]


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("logn,lp", RULE_ENDS, ids=[f"2^{a}-P2^{b}" for a, b in RULE_ENDS])
def test_interleave_rule_ends(suf, logn, lp, monkeypatch):
    """(N, P) on both sides of each edge of the rule: N = 2048, log2 P = 1 / 5
    and 11.  P = 2048 at N = 2048 is one element per slice and tile.  The plan
    of the shape names the kernel: the default plan where it has an interleave
    launch, and the plan forced to have one (slice-major passes, no
    natural-order store)."""
    n, P, prec = 1 << logn, 1 << lp, acc.PREC[suf]
    for batch in (1, 3):
        run_interleave(n, P, batch, suf)
    want = "void pifft::k_interleave_tile<" if tiled(prec, n, P) else "void pifft::k_interleave<"
    assert tiled(prec, n, P) == {(10, 1): False, (11, 1): suf == "f32", (11, 4): suf == "f32", (11, 5): True,
                                 (11, 11): True, (12, 11): True, (12, 12): False, (13, 12): False,
                                 (14, 7): True}[(logn, lp)]
    seen = 0
    for env in ({}, {"PIFFT_WORKER_IL": "0", "PIFFT_ILV": "0"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        plan = pifft.Plan(n, P, 1, prec)
        kinds = plan.describe()["launch_kind"]
        if "interleave" in kinds:
            assert plan.kernel_name(kinds.index("interleave")).startswith(want), (env, plan.kernel_name(len(kinds) - 1))
            seen += 1
    assert seen >= 1, "no plan of this shape has an interleave launch"


# ---------------------------------------------------------------- generator ---
@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_generate(suf):
    n = 1 << 20
    for count in (1, 255, 256, 257, 1000):
        for first in (0, 7, 2 ** 32 - 3, 2 ** 40 + 1):
            assert run_generate(suf, n, count, first) == oracle.generate(n, acc.DT[suf], 0x5EED, count, first).tobytes(), \
                (count, first)


def run_generate(suf, n, count, first):
    out = torch.full((count + acc.TAIL,), complex(acc.SENTINEL, acc.SENTINEL),
                     dtype=torch.complex128 if suf == "f64" else torch.complex64, device="cuda")
    torch.cuda.synchronize()
    pifft.generate_device(out.data_ptr(), count, n, acc.PREC[suf], seed=0x5EED, first=first,
                          stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    tail = torch.view_as_real(out[count:]).cpu().numpy()
    assert (tail == tail.dtype.type(acc.SENTINEL)).all(), "the sentinel behind d_x was overwritten"
    return out[:count].cpu().numpy().tobytes()


# ------------------------------------------------- second and later trips ---
def C(logn, P, flags, direction, prec, batch=1):
    return ac.Case(1 << logn, P, 0, P, batch, prec, flags, direction, ())


# (case, the family in focus, the SW values of that family the plan must launch)
TRIPS = [t for prec in (64, 32) for t in [
    (C(16, 1 << 16, SL, "fwd", prec), TREE, {0}),          # four k_tree<T, 4> launches in place, 16 workgroups each
    (C(16, 1 << 16, SL, "inv", prec), TREE, {1, 0, 2}),    # SW 1 first, SW 2 last
    (C(16, 16, NAT | SEP, "fwd", prec), TREE_WIL, {0}),    # 16 workgroups through the LDS stage
    (C(16, 16, NAT | SEP, "inv", prec), TREE_WIL, {1}),
    (C(16, 1 << 16, NAT, "fwd", prec), IL, {0}),           # log2 P = 16: k_interleave, 256 workgroups
    (C(16, 1 << 16, NAT, "inv", prec), IL, {2}),
    # four tiles behind a tree and a pass: fp64 tiles from P = 32, fp32 from P = 2
    (C(13, 32 if prec == 64 else 2, NAT | SEP, "fwd", prec), IL_TILE, {0}),
    (C(13, 32 if prec == 64 else 2, NAT | SEP, "inv", prec), IL_TILE, {2}),
]]


def launches_in_focus(ids, family):
    return [(i, k, g) for i, (k, g) in enumerate(ids) if k >= 0 and table()[k][0] == family]


def capped_runs(c, family, monkeypatch, caps=None, want=None):
    """Uncapped (held to its references), then under each cap: the launch
    description first, then the output, bit for bit the uncapped one."""
    free = ac.launches(c)
    focus = launches_in_focus(free, family)
    assert focus, (c, free)
    want = checked_run(c) if want is None else want
    blocks = min(g for _, _, g in focus)
    for cap in caps or (1, 3, blocks - 1):
        monkeypatch.setenv("PIFFT_STRIDE_GRID_MAX", str(cap))
        ids = ac.launches(c)
        assert ids == [(k, min(g, cap) if k >= 0 else g) for k, g in free], (cap, ids, free)
        for i, _, g in focus:
            assert ids[i][1] == cap < g, f"cap {cap}: launch {i} needs {g} workgroups -- no second trip"
            assert cap != 3 or g % 3, f"{g} workgroups: every thread would make the same number of trips"
        assert plain_run(c) == want, f"PIFFT_STRIDE_GRID_MAX={cap}: the output differs from the uncapped run's"
        monkeypatch.delenv("PIFFT_STRIDE_GRID_MAX")
    return free


@pytest.mark.parametrize("c,family,sws", TRIPS, ids=[f"{ac.case_id(t[0])}-family{t[1]}" for t in TRIPS])
def test_second_trips(c, family, sws, monkeypatch):
    free = capped_runs(c, family, monkeypatch)
    assert sws <= {table()[k][3] for _, k, _ in launches_in_focus(free, family)}, free


def real_units(prec, n):
    """real_units<T>(H) of csrc/pifft_real.h."""
    return (n // 4) // (2 if prec == 32 else 1) + 1


# (log2 N at fp64 -- one more at fp32, the same units --, caps, step_rows per cap): batch 3, P = 1
REAL_TRIPS = [(9, (1,), (1,)),               # 129 units, 2 workgroups: 256 threads >= units, step_rows 1, step_units 127
              (11, (1, 3, 6), (0, 1, 2)),    # 513 units, 7 workgroups: threads < units at 1; rows 1 and 2 beyond
              (12, (1, 3, 12), (0, 0, 2))]   # 1025 units, 13 workgroups: 768 threads < units at 3


@pytest.mark.parametrize("direction", ["r2c", "c2r"])
@pytest.mark.parametrize("prec", [64, 32])
@pytest.mark.parametrize("logn,caps,rows", REAL_TRIPS, ids=[f"2^{t[0]}" for t in REAL_TRIPS])
def test_second_trips_real(logn, caps, rows, prec, direction, monkeypatch):
    """real_thread's walk (row += step_rows, u += step_units with a carry) in
    both regimes, step_rows / step_units taken by add_real_step from the grid
    it launches: threads >= units (step_rows >= 1, step_units != 0) and
    threads < units (step_rows = 0)."""
    n = 1 << (logn + (prec == 32))
    c = ac.Case(n, 1, 0, 1, 3, prec, NAT, direction, ())
    units = real_units(prec, n)
    blocks = (3 * units + 255) // 256
    for cap, r in zip(caps, rows):
        assert cap < blocks and (256 * cap) // units == r and (256 * cap) % units != 0, (cap, units)
    assert caps[-1] == blocks - 1 and max(rows) >= 1
    free = capped_runs(c, R2C if direction == "r2c" else C2R, monkeypatch, caps=caps)
    assert launches_in_focus(free, R2C if direction == "r2c" else C2R)[0][2] == blocks


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_second_trips_direct_calls(suf, monkeypatch):
    """pifft_interleave_device and pifft_generate_device have no plan to
    describe their grid (test_second_trips shows stride_grid reads the
    variable): capped against uncapped, bit for bit."""
    prec = acc.PREC[suf]
    for logn, lp in ((16, 16), (13, 5 if prec == 64 else 1)):   # k_interleave: 256 workgroups; the tiles: 4
        n, P = 1 << logn, 1 << lp
        blocks = n >> 11 if tiled(prec, n, P) else n // 256
        assert blocks > 3 and blocks % 3
        want = run_interleave(n, P, 1, suf)
        for cap in (1, 3, blocks - 1):
            monkeypatch.setenv("PIFFT_STRIDE_GRID_MAX", str(cap))
            assert run_interleave(n, P, 1, suf) == want, (logn, lp, cap)
            monkeypatch.delenv("PIFFT_STRIDE_GRID_MAX")
    want = run_generate(suf, 1 << 20, 1000, 7)   # 4 workgroups, the last of 232 values
    assert want == oracle.generate(1 << 20, acc.DT[suf], 0x5EED, 1000, 7).tobytes()
    for cap in (1, 3):
        monkeypatch.setenv("PIFFT_STRIDE_GRID_MAX", str(cap))
        assert run_generate(suf, 1 << 20, 1000, 7) == want, cap
        monkeypatch.delenv("PIFFT_STRIDE_GRID_MAX")
