"""Every single-pass k_pass instance and twin on a partial last tile, on an MI355X.

k_pass has one tail path (csrc/pifft_kernels.h): where a launch's nlines is no
multiple of the tile's C lines, the last workgroup runs with idle lines -- fp32
idle lanes load the last line again (clamp_loads), fp64 ones load nothing, all
of them go through the butterflies, the LDS hand-offs and the cross-lane
swaps, and every store form (slice-major, natural order through ilv_log,
bit-reversed) is guarded by line < nlines.  Only the single pass (MODE 0 and
4) meets it, with nlines = batch x workers of the plan, and
tests/test_gpu_instances.py runs whole tiles only.  So
tests/golden/partial_tile_cases.tsv (tools/partial_tile_cases.py; held to the
planner on the CPU by tests/test_partial_tile_cases.py) names, for each of the
214 such instances of C > 1 and for their 428 twins, plans with a partial last
tile -- one whole tile and one live line (batch C + 1), one idle line (2C - 1)
-- and a grid for the natural-order store.  For every row, built under the
row's tuning variables:

  * name and lines: plan.kernel_name of the pass launch names the instance
    (k_pass_sw and the stated SW for a twin), plan.info.lines[0] is C;
  * guards (run_guarded): d_out lies inside a larger buffer with C R sentinel
    values in front of it and C R behind -- every row the idle lines of the
    last tile could address -- which all survive; d_in lies between C R NaNs
    on either side and the whole buffer keeps its bits.  (test_gpu_accuracy.run
    guards 8 values: one idle line's stray stores cover R.)  Offsets of C R
    elements keep the allocation's alignment for the 16-byte accesses;
  * bit for bit against the whole tile: the same shape under the same
    variables at batch 2C (3C where the row's batch exceeds 2C) launches the
    same kernel on whole tiles; its first `batch` input transforms are the
    row's (pifft_oracle.generate is prefix-stable), and its first `batch`
    output transforms must equal the row's byte for byte -- a line's
    arithmetic does not depend on its neighbours, idle or live;
  * against the long-double FFT: test_gpu_accuracy.check on every transform of
    the batch, its references and bounds unchanged (FACTOR = 4 for rel-L2 and
    worst bin: these plans have one pass);
  * a forward row: the three exact inputs, bit for bit (assert_exact);
  * an inverse row: the output equals swap(forward(swap(x))) bit for bit, the
    forward plan built under the same shape and variables, and is checked
    against the index-reversed references, as tests/test_gpu_instances.py does.

The cases without tuning variables -- plans any caller with such a batch gets
-- and the forced ones are two test functions, so that they can run apart.
"""
import os
import sys

import numpy as np
import pytest

import test_gpu_accuracy as acc
from test_gpu_instances import SUF, kernel_name, reversed_index, swap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import instance_cases as ic  # noqa: E402
import partial_tile_cases as pt  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROWS = pt.read_cases()  # sorted by (precision, log2 N, batch): the cached references of a size serve its cases back to back
UNTUNED = [r for r in ROWS if not r[0].env]
FORCED = [r for r in ROWS if r[0].env]


def case_id(row):
    return ic.case_id(row[0])


def run_guarded(plan, x, guard):
    """Execute on x with `guard` sentinel values on either side of d_out and
    `guard` NaNs on either side of d_in: the sentinels survive and the input
    buffer, NaNs included, keeps its bits.  Returns the output."""
    ni, ne = plan.info.in_elems, plan.info.out_elems
    assert x.size == ni and guard > 0
    d_x = acc.dev(x)
    buf_in = torch.full((ni + 2 * guard,), complex(float("nan"), float("nan")), dtype=d_x.dtype, device="cuda")
    buf_in[guard:guard + ni] = d_x
    keep = buf_in.clone()
    buf_out = torch.full((ne + 2 * guard,), complex(acc.SENTINEL, acc.SENTINEL), dtype=d_x.dtype, device="cuda")
    d_in, d_out = buf_in[guard:], buf_out[guard:]
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    plan.execute_device(d_in.data_ptr(), d_out.data_ptr(), torch.cuda.current_stream())
    torch.cuda.synchronize()
    out = buf_out.cpu().numpy()
    flat = out.view(out.real.dtype)
    sentinel = flat.dtype.type(acc.SENTINEL)
    front, back = flat[:2 * guard] != sentinel, flat[2 * (guard + ne):] != sentinel
    assert not front.any(), f"{np.count_nonzero(front)} sentinel values in front of d_out were overwritten"
    assert not back.any(), (f"{np.count_nonzero(back)} sentinel values behind d_out were overwritten, the first "
                            f"{np.flatnonzero(back)[0] // 2} values behind it")
    assert torch.equal(acc.bits(buf_in), acc.bits(keep)), "d_in or its NaN guards were written"
    return out[guard:guard + ne]


def run_case(row, monkeypatch):
    c, cov = row
    (launch, desc, sw), = cov
    for k, v in c.env:
        monkeypatch.setenv(k, v)
    R, C = desc[1], desc[2]
    suf, logn = SUF[c.prec], ic.log2(c.n)
    whole_batch = 2 * C if c.batch <= 2 * C else 3 * C
    assert c.batch < whole_batch
    shape = (logn, c.P, c.first, c.count, c.flags, c.batch)
    whole_shape = shape[:5] + (whole_batch,)
    plan = acc.make_plan(suf, shape, inverse=c.inverse)
    whole = acc.make_plan(suf, whole_shape, inverse=c.inverse)
    assert plan.describe()["inverse"] == c.inverse
    assert plan.kernel_name(launch) == kernel_name(desc, sw) == whole.kernel_name(launch)
    assert plan.info.num_passes == whole.info.num_passes == 1
    assert plan.info.lines[0] == whole.info.lines[0] == C
    lines = c.count * (c.n // c.P) // R  # of one batch entry
    assert c.batch * lines % C != 0 and whole_batch * lines % C == 0

    guard = C * R
    x, H, O = acc.references(suf, logn, whole_batch)
    xp, H, O = x[:c.batch * c.n], H[:c.batch], O[:c.batch]
    got = run_guarded(plan, xp, guard)
    full = run_guarded(whole, x, guard)
    assert got.tobytes() == full[:got.size].tobytes(), "the partial tile's transforms differ from the whole tiles'"
    if c.inverse:
        fwd = acc.make_plan(suf, shape)
        want = swap(run_guarded(fwd, swap(xp), guard))
        assert got.tobytes() == want.tobytes(), "the inverse plan is not swap(forward(swap(x))) bit for bit"
        H, O = reversed_index(H), reversed_index(O)
    order = lambda A: np.stack([acc.plan_order(a, c.P, c.first, c.count, c.flags) for a in A])  # noqa: E731
    acc.check(f"ptl {case_id(row)}", suf, got.reshape(c.batch, -1), order(H), order(O), 1)
    if not c.inverse:
        acc.assert_exact(plan, suf, shape)


@pytest.mark.parametrize("row", UNTUNED, ids=case_id)
def test_untuned_case(row, monkeypatch):
    run_case(row, monkeypatch)


@pytest.mark.parametrize("row", FORCED, ids=case_id)
def test_forced_case(row, monkeypatch):
    run_case(row, monkeypatch)
