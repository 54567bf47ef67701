"""2-D complex transforms (pifft_plan_create_matrix) on an MI355X, through the C-ABI.

A matrix plan of batch arrays of n0 x n1 values is the 1-D plan of the rows,
(n1, 1 worker, batch n0), a tiled transpose (k_transpose), the 1-D plan of the
columns, (n0, 1 worker, batch n1), and a transpose back unless the output
stays transposed.  Checked here: the output against that composition of
already-tested plans around torch's exact transposes, bit for bit (1); the
mathematics against numpy's fft2 in complex128, independently of the
composition, at the parity tests' bounds -- loose on purpose: a wrong axis,
sign or layout is an error of order 1 (2); inputs whose transform is exact (3);
round trips (4); kernel names and grids (5); the transpose's grid-stride
second trips under a lowered grid cap (6); the entry points' surface (7).

Every execution goes through tests/test_gpu_accuracy.py's run: 8 sentinel
values behind d_out must survive and d_in keeps its bits.

Shapes: 2 x 2 is the smallest; 2 x 4096 and 4096 x 2 have one dimension far
below the tile; 64 x 64 is one fp32 tile and 2 x 2 fp64 tiles; 32 x 128 and
128 x 32 with batch 3 are non-square with several tiles per matrix; 256 x 256
x 3 has 192 (fp64) / 48 (fp32) tiles; a 2^15 axis makes that axis's inner plan
multi-pass; 1024 x 1024 is the largest (2^20 values).  (t, t), (2t, t/2) and
(t/2, 2t) for both precisions' tiles t = 32, 64 are added where missing.
"""
import functools
import math

import numpy as np
import pytest

import pifft
import pifft_oracle as oracle
import test_gpu_accuracy as acc
from golden_io import rel_l2

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DT = {"f32": np.complex64, "f64": np.complex128}
PREC = {"f32": pifft.F32, "f64": pifft.F64}
CTYPE = {"f32": "float", "f64": "double"}

BASE = [(2, 2, 1), (2, 4096, 1), (4096, 2, 3), (64, 64, 1), (32, 128, 3), (128, 32, 3), (256, 256, 3),
        (4, 1 << 15, 1), (1 << 15, 4, 1), (1024, 1024, 1)]
TILES = [s for t in (32, 64) for s in ((t, t, 1), (2 * t, t // 2, 3), (t // 2, 2 * t, 3))]
S = BASE + [s for s in dict.fromkeys(TILES) if s not in BASE]
MULTI_PASS = {(4, 1 << 15, 1): (2, 1), (1 << 15, 4, 1): (1, 2)}  # (rows' passes, columns' passes)
NONSQUARE = [(32, 128, 3), (128, 32, 3), (4, 1 << 15, 1), (2, 4096, 1)]


def sid(s):
    return "%dx%d-b%d" % s


def tol(suf, n):
    """tests/test_gpu_real.py's tol(): the parity tests' bounds."""
    return 1e-12 if suf == "f64" else 1e-5 * math.log2(n)


def ibits(a):
    """A complex numpy array's bit patterns."""
    a = np.ascontiguousarray(a)
    return a.view(np.float64 if a.dtype == np.complex128 else np.float32).view(
        np.int64 if a.dtype == np.complex128 else np.int32)


@functools.lru_cache(maxsize=None)
def host_input(suf, shape):
    n0, n1, batch = shape
    x = oracle.generate(n0 * n1, DT[suf], count=batch * n0 * n1)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def composition(suf, shape, inverse):
    """The transposed-out result (batch arrays of n1 x n0) of the two 1-D plans
    around torch's transpose, computed once; read-only."""
    n0, n1, batch = shape
    rows = pifft.Plan(n1, 1, batch * n0, PREC[suf], inverse=inverse)
    cols = pifft.Plan(n0, 1, batch * n1, PREC[suf], inverse=inverse)
    y = acc.run(rows, acc.dev(host_input(suf, shape)))
    yt = torch.from_numpy(y).reshape(batch, n0, n1).transpose(-1, -2).contiguous().reshape(-1).to("cuda")
    z = acc.run(cols, yt)
    z.setflags(write=False)
    return z, (rows.info.num_passes, cols.info.num_passes), \
        ([rows.kernel_name(i) for i in range(rows.info.num_launches)],
         [cols.kernel_name(i) for i in range(cols.info.num_launches)])


def natural(zt, shape):
    n0, n1, batch = shape
    return torch.from_numpy(np.array(zt)).reshape(batch, n1, n0).transpose(-1, -2).contiguous().reshape(-1).numpy()


def make(suf, shape, **kw):
    n0, n1, batch = shape
    return pifft.MatrixPlan(n0, n1, batch, PREC[suf], **kw)


# ---- 1. the composition, bit for bit ----------------------------------------
@pytest.mark.parametrize("tout", [False, True], ids=["natural", "transposed"])
@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("shape", S, ids=sid)
def test_equals_the_composition_of_the_inner_plans(shape, suf, inverse, tout):
    zt, passes, _ = composition(suf, shape, inverse)
    if shape in MULTI_PASS:
        assert passes == MULTI_PASS[shape]
    plan = make(suf, shape, inverse=inverse, transposed_out=tout)
    assert plan.info.num_passes == sum(passes)
    got = acc.run(plan, acc.dev(host_input(suf, shape)))
    want = zt if tout else natural(zt, shape)
    diff = np.count_nonzero(ibits(got) != ibits(want))
    assert diff == 0, f"{diff} of {2 * got.size} words differ"


# ---- 2. the mathematics -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def fft2_reference(suf, shape, inverse):
    n0, n1, batch = shape
    x = host_input(suf, shape).astype(np.complex128).reshape(batch, n0, n1)
    X = np.fft.ifft2(x) * (n0 * n1) if inverse else np.fft.fft2(x)
    X.setflags(write=False)
    return X


@pytest.mark.parametrize("tout", [False, True], ids=["natural", "transposed"])
@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("shape", S, ids=sid)
def test_against_numpy_fft2(shape, suf, inverse, tout):
    n0, n1, batch = shape
    X = fft2_reference(suf, shape, inverse)
    plan = make(suf, shape, inverse=inverse, transposed_out=tout)
    got = acc.run(plan, acc.dev(host_input(suf, shape)))
    got = got.reshape(batch, n1, n0).transpose(0, 2, 1) if tout else got.reshape(batch, n0, n1)
    err = rel_l2(got.astype(np.complex128).reshape(-1), X.reshape(-1))
    print(f"fft2 {suf} {sid(shape)} inv={inverse} tout={tout}: rel-L2 {err:.3e} (bound {tol(suf, n0 * n1):.3e})")
    assert err <= tol(suf, n0 * n1)


# ---- 3. exact inputs, bit for bit -------------------------------------------
def exact_cases(n0, n1, dtype):
    """(name, x, X): every non-zero value meets only the twiddle w^0."""
    j0, j1 = np.arange(n0)[:, None], np.arange(n1)[None, :]
    def at(k0, k1):
        X = np.zeros((n0, n1), dtype=dtype)
        X[k0, k1] = n0 * n1
        return X
    delta = np.zeros((n0, n1), dtype=dtype)
    delta[0, 0] = 1
    return [("impulse", delta, np.ones((n0, n1), dtype=dtype)),
            ("constant", np.ones((n0, n1), dtype=dtype), at(0, 0)),
            ("(-1)^j0", ((-1.0) ** j0 * np.ones((1, n1))).astype(dtype), at(n0 // 2, 0)),
            ("(-1)^j1", (np.ones((n0, 1)) * (-1.0) ** j1).astype(dtype), at(0, n1 // 2))]


@pytest.mark.parametrize("tout", [False, True], ids=["natural", "transposed"])
@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("shape", NONSQUARE, ids=sid)
def test_exact_inputs(shape, suf, inverse, tout):
    """Every bit of the exact answer, the zeros' sign bits included (+0)."""
    n0, n1, batch = shape
    plan = make(suf, shape, inverse=inverse, transposed_out=tout)
    for name, x, X in exact_cases(n0, n1, DT[suf]):
        got = acc.run(plan, acc.dev(np.tile(x.reshape(-1), batch)))
        want = np.tile((X.T if tout else X).reshape(-1), batch)
        diff = np.count_nonzero(ibits(got) != ibits(want))
        print(f"exact {suf} {sid(shape)} inv={inverse} tout={tout} {name}: {diff} words differ in bits")
        assert diff == 0, f"{name}: {diff} words differ ({np.count_nonzero(got != want)} values)"


# ---- 4. round trips ---------------------------------------------------------
@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("shape", S, ids=sid)
def test_round_trip(shape, suf):
    n0, n1, batch = shape
    x = host_input(suf, shape)
    X = acc.run(make(suf, shape), acc.dev(x))
    back = acc.run(make(suf, shape, inverse=True), acc.dev(X)) / DT[suf](n0 * n1)
    err = rel_l2(back.astype(np.complex128), x.astype(np.complex128))
    # transposed-out forward, then the inverse plan of the n1 x n0 shape with transposed-out: the original layout
    Xt = acc.run(make(suf, shape, transposed_out=True), acc.dev(x))
    back_t = acc.run(make(suf, (n1, n0, batch), inverse=True, transposed_out=True), acc.dev(Xt)) / DT[suf](n0 * n1)
    err_t = rel_l2(back_t.astype(np.complex128), x.astype(np.complex128))
    print(f"round trip {suf} {sid(shape)}: rel-L2 {err:.3e}, through transposed-out {err_t:.3e} "
          f"(bound {tol(suf, n0 * n1):.3e})")
    assert err <= tol(suf, n0 * n1) and err_t <= tol(suf, n0 * n1)


# ---- 5. kernel names and grids ----------------------------------------------
@pytest.mark.parametrize("tout", [False, True], ids=["natural", "transposed"])
@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("shape", S, ids=sid)
def test_kernel_names_and_grids(shape, suf, inverse, tout):
    n0, n1, batch = shape
    _, _, (row_names, col_names) = composition(suf, shape, inverse)
    plan = make(suf, shape, inverse=inverse, transposed_out=tout)
    kinds = list(plan.info.launch_kind[:plan.info.num_launches])
    names = [plan.kernel_name(i) for i in range(plan.info.num_launches)]
    t_name = f"void pifft::k_transpose<{CTYPE[suf]}>(pifft::TransposeArgs)"
    assert names == row_names + [t_name] + col_names + ([] if tout else [t_name])
    assert [k == 7 for k in kinds] == [n == t_name for n in names]
    # launch_fn: equal ids exactly for equal kernels, over the whole plan
    fn = list(plan.info.launch_fn[:plan.info.num_launches])
    seen = {}
    assert fn == [seen.setdefault(n, len(seen)) for n in names]
    t_at = [i for i, k in enumerate(kinds) if k == 7]
    assert plan.launch_grid(t_at[0]) == pifft.transpose_tiles(n0, n1, batch, PREC[suf])
    if not tout:
        assert plan.launch_grid(t_at[1]) == pifft.transpose_tiles(n1, n0, batch, PREC[suf])
    with pytest.raises(pifft.PifftError, match="out of range"):
        plan.launch_grid(plan.info.num_launches)


def test_launch_grid_of_a_one_dimensional_plan():
    plan = pifft.Plan(1 << 10, 4, 2, pifft.F64)
    want = [g for _, g in pifft.dry_run_aux(1 << 10, 4, 2, pifft.F64)]
    assert [plan.launch_grid(i) for i in range(plan.info.num_launches)] == want


# ---- 6. grid-stride second trips --------------------------------------------
@pytest.mark.parametrize("tout", [False, True], ids=["natural", "transposed"])
@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("shape", [(256, 256, 3), (32, 128, 3)], ids=sid)
def test_second_trips(shape, suf, tout, monkeypatch):
    n0, n1, batch = shape
    x = acc.dev(host_input(suf, shape))
    free = acc.run(make(suf, shape, transposed_out=tout), x)
    tiles = pifft.transpose_tiles(n0, n1, batch, PREC[suf])
    assert tiles == pifft.transpose_tiles(n1, n0, batch, PREC[suf]) and tiles > 2
    for cap in (1, 3, tiles - 1):
        monkeypatch.setenv("PIFFT_STRIDE_GRID_MAX", str(cap))
        plan = make(suf, shape, transposed_out=tout)
        monkeypatch.delenv("PIFFT_STRIDE_GRID_MAX")
        t_at = [i for i in range(plan.info.num_launches) if plan.info.launch_kind[i] == 7]
        assert len(t_at) == (1 if tout else 2)
        for i in t_at:
            assert plan.launch_grid(i) == min(cap, tiles) < tiles
        got = acc.run(plan, x)
        assert np.array_equal(ibits(got), ibits(free)), f"cap {cap}"


# ---- 7. the surface ---------------------------------------------------------
@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_surface(suf):
    shape = (32, 128, 3)
    n0, n1, batch = shape
    plan = make(suf, shape)
    assert plan.is_real() == 0 and plan.dims() == (n0, n1)
    assert make(suf, shape, transposed_out=True).dims() == (n0, n1)
    one = pifft.Plan(1 << 10, 2, 3, PREC[suf])
    assert one.dims() == (1, 1 << 10) and one.is_real() == 0
    assert pifft.RealPlan(1 << 10, 1, 2, PREC[suf]).dims() == (1, 1 << 10)
    d = plan.describe()
    assert d["launch_kind"] == ["pass", "transpose", "pass", "transpose"] and d["n"] == n0 * n1
    x = acc.dev(host_input(suf, shape))
    a, b = acc.run(plan, x), acc.run(plan, x)
    assert np.array_equal(ibits(a), ibits(b))
    # the timed and profiled paths run the same launches
    out = torch.empty(plan.info.out_elems, dtype=x.dtype, device="cuda")
    ms = plan.execute_device_timed(x.data_ptr(), out.data_ptr(), torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert len(ms) == 4 and all(m > 0 for m in ms) and np.array_equal(ibits(out.cpu().numpy()), ibits(a))
    plan.profile_start(8, pifft.PROFILE_SAMPLED)
    for _ in range(8):
        plan.execute_device(x.data_ptr(), out.data_ptr(), torch.cuda.current_stream())
    used, sums, counts = plan.profile_read()
    assert used == 8 and counts == [1, 1, 1, 1] and all(s > 0 for s in sums)
    assert plan.launch_loop([1], 3, x.data_ptr(), out.data_ptr(), torch.cuda.current_stream()) > 0
    assert np.array_equal(ibits(out.cpu().numpy()), ibits(a))
    # refused: the host boundary, multi-plan calls, the tree, workspace tuning, misaligned and in-place buffers
    host = np.array(host_input(suf, shape))
    for call in (lambda: plan.execute(host),
                 lambda: pifft.execute_group([plan], host),
                 lambda: pifft.execute_group_kernel_times([plan]),
                 lambda: pifft.allgather([plan], [x.data_ptr()], [out.data_ptr()]),
                 lambda: plan.tree_device(x.data_ptr(), out.data_ptr()),
                 lambda: plan.tune_workspace(x.data_ptr(), out.data_ptr())):
        with pytest.raises(pifft.PifftError, match="matrix plans"):
            call()
    with pytest.raises(pifft.PifftError, match="16-byte aligned"):
        plan.execute_device(x.data_ptr() + 8, out.data_ptr())
    with pytest.raises(pifft.PifftError, match="in-place"):
        plan.execute_device(x.data_ptr(), x.data_ptr())
