"""Every compiled k_pass instance and every swapping twin, run on an MI355X at a
small size against the long-double FFT.

libpifft.so holds 848 k_pass instances and 1163 twins (k_pass_sw), each a
compilation of its own with its own LDS layout, stage decomposition, exchange
and store path; a bad layout, a missing barrier or a wrong twiddle index in
one of them shows only when that one runs.  tests/golden/instance_cases.tsv
(tools/instance_cases.py; held to the planner on the CPU by
tests/test_instance_cases.py) names one plan of at most 2^20 values per
instance and twin -- all but the few of instance_cases_exceptions.txt.  For
every row, built under the row's tuning variables:

  * plan.kernel_name of each covered launch names that instance's template
    arguments (k_pass_sw and the stated SW for a twin);
  * the execution goes through test_gpu_accuracy.run: the sentinel tail behind
    d_out survives and d_in keeps its bits;
  * a forward case: the output, in the plan's order, against oracle.fft_hp and
    the oracle's own error (test_gpu_accuracy.references and check), and the
    three inputs whose transform is exact, bit for bit (assert_exact);
  * an inverse case: the output equals swap(forward(swap(x))) bit for bit,
    the forward plan built under the same shape and variables, and passes
    check against the index-reversed references H[(-k) mod N], O[(-k) mod N]:
    the unnormalised inverse of x is X[-k], an exact reordering of the arrays
    already cached.

Bounds (nothing taken from the kernels' measured error):
rel-L2 FACTOR = 4 times the oracle's; worst bin 4, and for fp32 plans of two
or more passes test_gpu_accuracy's 6 -- or, where larger, the same model
(tools/accuracy_model.py worst_bin_bound) with its tail taken over N times the
number of fp32 multi-pass cases of this file instead of N: several hundred
cases share that bound, which test_gpu_accuracy's largest case approaches
within 5 %, and a maximum over that many would exceed it by chance.  The
derivation holds from N = 2^14 up, the smallest multi-pass case of the table.

The cases without tuning variables -- plans any caller gets -- and the forced
ones are two test functions, so that they can run apart.
"""
import functools
import os
import sys

import numpy as np
import pytest

import test_gpu_accuracy as acc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import accuracy_model  # noqa: E402
import instance_cases as ic  # noqa: E402

pytestmark = pytest.mark.gpu

SUF = {32: "f32", 64: "f64"}
CTYPE = {32: "float", 64: "double"}
ORACLE_C32 = 0.66  # the fp32 oracle's rel-L2 / (u sqrt(log2 N)): tests/test_hp_reference.py, tools/accuracy_model.py

ROWS = ic.read_cases()  # sorted by (precision, log2 N, batch): the cached references of a size serve its cases back to back
UNTUNED = [r for r in ROWS if not r[0].env]
FORCED = [r for r in ROWS if r[0].env]


def case_id(row):
    return ic.case_id(row[0])


def kernel_name(desc, sw):
    prec, R, C, mode, nts, lp, vpt = desc
    args = f"{CTYPE[prec]}, {R}, {C}, {mode}, {nts}, {lp}, {vpt}"
    return (f"void pifft::k_pass_sw<{args}, {sw}>(pifft::PassArgs)" if sw else
            f"void pifft::k_pass<{args}>(pifft::PassArgs)")


@functools.lru_cache(maxsize=None)
def sharing():
    """How many cases of the table share the fp32 multi-pass worst-bin bound."""
    import pifft
    k = 0
    for c, _ in ROWS:
        if c.prec != 32:
            continue
        with ic.tuning(c.env or None):
            k += pifft.dry_run(c.n, c.P, c.batch, c.prec, first=c.first, count=c.count, flags=c.flags,
                               inverse=c.inverse)["num_passes"] >= 2
    return k


@functools.lru_cache(maxsize=None)
def shared_worst_bin(passes, logn):
    return accuracy_model.worst_bin_bound(ORACLE_C32, passes, logn, bins=float(sharing()) * 2.0 ** logn)


def swap(a):
    """b + ai of a + bi, bit for bit."""
    return np.ascontiguousarray(a.view(a.real.dtype).reshape(-1, 2)[:, ::-1]).view(a.dtype).reshape(a.shape)


def reversed_index(A):
    """A[(-k) mod N] along the last axis."""
    return np.concatenate([A[..., :1], A[..., :0:-1]], axis=-1)


def run_case(row, monkeypatch):
    c, cov = row
    for k, v in c.env:
        monkeypatch.setenv(k, v)
    suf, logn = SUF[c.prec], ic.log2(c.n)
    shape = (logn, c.P, c.first, c.count, c.flags, c.batch)
    plan = acc.make_plan(suf, shape, inverse=c.inverse)
    assert plan.describe()["inverse"] == c.inverse
    for i, desc, sw in cov:
        assert plan.kernel_name(i) == kernel_name(desc, sw), (i, desc, sw)
    passes = plan.info.num_passes
    assert passes < 2 or c.n >= ic.MULTI_MIN_N
    bound = shared_worst_bin(passes, logn) if suf == "f32" and passes >= 2 else None
    x, H, O = acc.references(suf, logn, c.batch)
    got = acc.run(plan, acc.dev(x))
    if c.inverse:
        fwd = acc.make_plan(suf, shape)
        want = swap(acc.run(fwd, acc.dev(swap(x))))
        assert got.tobytes() == want.tobytes(), "the inverse plan is not swap(forward(swap(x))) bit for bit"
        H, O = reversed_index(H), reversed_index(O)
    order = lambda A: np.stack([acc.plan_order(a, c.P, c.first, c.count, c.flags) for a in A])  # noqa: E731
    acc.check(f"ins {case_id(row)}", suf, got.reshape(c.batch, -1), order(H), order(O), passes, shared_worst_bin=bound)
    if not c.inverse:
        acc.assert_exact(plan, suf, shape)


@pytest.mark.parametrize("row", UNTUNED, ids=case_id)
def test_untuned_case(row, monkeypatch):
    run_case(row, monkeypatch)


@pytest.mark.parametrize("row", FORCED, ids=case_id)
def test_forced_case(row, monkeypatch):
    run_case(row, monkeypatch)
