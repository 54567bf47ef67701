"""Real-input transforms (pifft_plan_create_real) on an MI355X, through the C-ABI.

R2C: N reals -> N/2 + 1 bins; C2R: N/2 + 1 bins -> N reals, unnormalised
(C2R(R2C(x)) = N x).  A real plan is the complex plan of H = N/2 points on
the same bytes plus one fix-up launch pairing bins k and H - k.  Checked here:
parity with the reference transform of the same data at the forward parity
tests' own bounds, the exact edge bins (which tie the plan to the inner plan
it contains, bit for bit), bin placement, round trips at twice the bounds (two
transforms' errors add), buffer discipline and the entry points' surface.
Every output buffer carries 8 trailing sentinel values, checked after every
execution.  Shapes are the smallest at which something new happens (see
SHAPES)."""
import functools
import math

import numpy as np
import pytest

import pifft
import pifft_oracle as oracle
from golden_io import rel_l2

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DT = {"f32": np.complex64, "f64": np.complex128}
RDT = {"f32": np.float32, "f64": np.float64}
TDT = {"f32": torch.complex64, "f64": torch.complex128}
PREC = {"f32": pifft.F32, "f64": pifft.F64}
SENTINEL = -7.5e33
TAIL = 8


def tol(suf, n):
    """The forward parity tests' bounds (tests/test_gpu_parity.py)."""
    return 1e-12 if suf == "f64" else 1e-5 * math.log2(n)


def bits(t):
    r = torch.view_as_real(t) if t.is_complex() else t
    return r.view(torch.int64 if r.dtype == torch.float64 else torch.int32)


def device_input(suf, batch, n, seed=0x5EED):
    """batch rows of n reals, as batch * n/2 generated complex values."""
    count = batch * n // 2
    x = torch.empty(count, dtype=TDT[suf], device="cuda")
    pifft.generate_device(x.data_ptr(), count, n, PREC[suf], seed)
    return x


def run(plan, d_in, stream=None, out=None):
    """Execute into a buffer with TAIL sentinel values behind it; the tail must survive."""
    ne = plan.info.out_elems
    if out is None:
        out = torch.full((ne + TAIL,), complex(SENTINEL, SENTINEL), dtype=d_in.dtype, device="cuda")
    assert d_in.numel() == plan.info.in_elems
    torch.cuda.synchronize()
    plan.execute_device(d_in.data_ptr(), out.data_ptr(), stream or torch.cuda.current_stream())
    torch.cuda.synchronize()
    tail = torch.view_as_real(out[ne:]).cpu().numpy()
    assert (tail == tail.dtype.type(SENTINEL)).all(), "the sentinel behind d_out was overwritten"
    return out[:ne]


# (log2 N, P, batch): 2, 3 have bin 0 and the self-paired bin only, 4 the first
# true pair; 6 with P = H an inner plan of tree and interleave launches only; 11
# with P = 32 and batch 3 the fp32 rows at 8 mod 16; 14 one inner pass, 15 the
# largest single inner pass, 16 two inner passes, 17 the fp64 last pass at 8
# values per thread, 22 three inner passes.  (One twiddle form, the two-level
# table, at every size: no table switch to straddle.)
SHAPES = [(logn, P, 1) for logn in (2, 3, 4) for P in sorted({1, 2, 1 << (logn - 1)})] + \
         [(6, 1, 3), (6, 2, 1), (6, 32, 1), (11, 32, 3), (14, 1, 1), (15, 1, 1), (16, 1, 1), (17, 1, 1), (22, 1, 1)]
INNER_PASSES = {14: 1, 15: 1, 16: 2, 17: 2, 22: 3}


def shape_id(s):
    return "2^%d-P%d-b%d" % s


@functools.lru_cache(maxsize=None)
def reference_r2c(suf, logn, batch):
    """(x, X) per row: X = oracle.fft(x + 0j, P=1)[:H+1] in the plan's precision, computed once."""
    n = 1 << logn
    z = oracle.generate(n, DT[suf], count=batch * n // 2)
    x = z.view(RDT[suf])
    X = np.concatenate([oracle.fft(x[b * n:(b + 1) * n].astype(DT[suf]), P=1)[:n // 2 + 1] for b in range(batch)])
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def reference_c2r(suf, logn, batch):
    """A random half spectrum per row with real X[0], X[H], and the real part of
    conj(oracle.fft(conj(X_full))) of its Hermitian extension."""
    n, h = 1 << logn, 1 << (logn - 1)
    rng = np.random.default_rng(1000 * logn + batch)
    X = ((rng.uniform(-1, 1, batch * (h + 1)) + 1j * rng.uniform(-1, 1, batch * (h + 1))) / math.sqrt(n)).astype(DT[suf])
    X = X.reshape(batch, h + 1)
    X[:, 0] = X[:, 0].real
    X[:, h] = X[:, h].real
    y = []
    for b in range(batch):
        full = np.concatenate([X[b], np.conj(X[b, h - 1:0:-1])])
        y.append(np.conj(oracle.fft(np.conj(full), P=1)).real.astype(RDT[suf]))
    X, y = X.reshape(-1), np.concatenate(y)
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_r2c_against_the_reference(suf, shape):
    logn, P, batch = shape
    n = 1 << logn
    plan = pifft.RealPlan(n, P, batch, PREC[suf])
    d = plan.describe()
    assert d["real"] == 1 and d["launch_kind"][-1] == "r2c" and "r2c" not in d["launch_kind"][:-1]
    if logn in INNER_PASSES:
        assert d["num_passes"] == INNER_PASSES[logn] and d["launch_kind"] == ["pass"] * INNER_PASSES[logn] + ["r2c"]
    if (logn, suf) == (17, "f64"):
        assert d["vpt"][-1] == 8
    if logn == 11:
        assert d["launch_kind"] == ["tree+pass", "r2c"]  # the one-launch inner plan of 32 workers
    if (logn, P) == (6, 32):
        assert d["launch_kind"] == ["tree", "tree", "interleave", "r2c"] and d["num_passes"] == 0
    x = device_input(suf, batch, n)
    got = run(plan, x).cpu().numpy()
    want = reference_r2c(suf, logn, batch)
    err = rel_l2(got, want)
    print(f"R2C {suf} 2^{logn} P={P} batch={batch}: rel-L2 {err:.3e} (bound {tol(suf, n):.1e})")
    assert got.shape == want.shape and err <= tol(suf, n)


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_c2r_against_the_reference(suf, shape):
    logn, P, batch = shape
    n = 1 << logn
    plan = pifft.RealPlan(n, P, batch, PREC[suf], inverse=True)
    d = plan.describe()
    assert d["real"] == 2 and d["inverse"] and d["launch_kind"][0] == "c2r" and "c2r" not in d["launch_kind"][1:]
    if logn in INNER_PASSES:
        assert d["launch_kind"] == ["c2r"] + ["pass"] * INNER_PASSES[logn]
    X, want = reference_c2r(suf, logn, batch)
    got = torch.view_as_real(run(plan, torch.from_numpy(np.array(X)).to("cuda"))).reshape(-1).cpu().numpy()
    err = rel_l2(got, want)
    print(f"C2R {suf} 2^{logn} P={P} batch={batch}: rel-L2 {err:.3e} (bound {tol(suf, n):.1e})")
    assert got.shape == want.shape and err <= tol(suf, n)


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("logn,P,batch", [(11, 1, 3), (11, 32, 3), (16, 1, 1), (16, 2, 3)])
def test_exact_edges_tie_the_real_plan_to_its_inner_plan(suf, logn, P, batch):
    """X[0] = Zr + Zi and X[H] = Zr - Zi of Z[0], bit for bit, imaginary parts
    exactly 0, with Z from the complex plan of H points on the same buffer:
    2^11 a single-pass inner plan, 2^16 a multi-pass one."""
    n, h = 1 << logn, 1 << (logn - 1)
    x = device_input(suf, batch, n)
    inner = pifft.Plan(h, P, batch, PREC[suf])
    assert inner.describe()["num_passes"] == (1 if logn == 11 else 2)
    Z = run(inner, x).reshape(batch, h)
    X = run(pifft.RealPlan(n, P, batch, PREC[suf]), x).reshape(batch, h + 1)
    zr, zi = Z[:, 0].real.contiguous(), Z[:, 0].imag.contiguous()
    assert torch.equal(bits(X[:, 0].real.contiguous()), bits(zr + zi))
    assert torch.equal(bits(X[:, h].real.contiguous()), bits(zr - zi))
    zero = torch.zeros_like(zr)
    assert torch.equal(bits(X[:, 0].imag.contiguous()), bits(zero))
    assert torch.equal(bits(X[:, h].imag.contiguous()), bits(zero))
    assert float(X[:, 0].real.abs().max()) > 0


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("logn,P,batch", [(3, 1, 3), (11, 32, 3), (16, 1, 1)])
def test_c2r_ignores_the_imaginary_parts_of_the_edge_bins(suf, logn, P, batch):
    n, h = 1 << logn, 1 << (logn - 1)
    X, _ = reference_c2r(suf, logn, batch)
    plan = pifft.RealPlan(n, P, batch, PREC[suf], inverse=True)
    a = torch.from_numpy(np.array(X)).to("cuda")
    b = a.clone().reshape(batch, h + 1)
    b[:, 0] += 1e3j
    b[:, h] += 1e3j
    b = b.reshape(-1)
    assert not torch.equal(bits(a), bits(b))
    ya, yb = run(plan, a), run(plan, b)
    assert torch.equal(bits(ya), bits(yb)) and float(ya.abs().max()) > 0


def test_bin_placement():
    logn, suf = 10, "f64"
    n, h = 1 << logn, 1 << (logn - 1)
    plan = pifft.RealPlan(n, 1, 1, PREC[suf])
    for f in (0, 1, h // 2, h - 1, h):
        x = np.cos(2 * np.pi * f * np.arange(n) / n)
        d_in = torch.view_as_complex(torch.from_numpy(x).to("cuda").reshape(h, 2))
        X = run(plan, d_in).cpu().numpy()
        peak = n if f in (0, h) else n / 2
        assert abs(X[f] - peak) <= 1e-9 * n, (f, X[f])
        rest = np.delete(X, f)
        assert np.abs(rest).max() < 1e-9 * n, (f, np.abs(rest).max())


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("logn", [3, 15, 16])
@pytest.mark.parametrize("batch", [1, 3])
def test_round_trip(suf, logn, batch):
    n = 1 << logn
    x = device_input(suf, batch, n)
    X = run(pifft.RealPlan(n, 1, batch, PREC[suf]), x)
    back = run(pifft.RealPlan(n, 1, batch, PREC[suf], inverse=True), X.contiguous())
    want = (x * n).to(torch.complex128)
    err = float(torch.linalg.vector_norm(back.to(torch.complex128) - want) / torch.linalg.vector_norm(want))
    print(f"{suf} 2^{logn} batch={batch}: round trip rel-L2 {err:.3e} (bound {2 * tol(suf, n):.1e})")
    assert err <= 2 * tol(suf, n)


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("logn,P,batch", [(11, 32, 3), (16, 2, 3), (22, 1, 1)])
@pytest.mark.parametrize("inverse", [False, True], ids=["r2c", "c2r"])
def test_buffer_discipline(suf, logn, P, batch, inverse):
    """d_in untouched (multi-pass inner plans use their output as a ping-pong
    stage: here it is the plan's staging buffer), two executions bit-identical,
    a non-default stream gives the default stream's bits."""
    n = 1 << logn
    plan = pifft.RealPlan(n, P, batch, PREC[suf], inverse=inverse)
    d_in = device_input(suf, batch, n)
    if inverse:  # a half spectrum: the forward plan's output
        d_in = run(pifft.RealPlan(n, P, batch, PREC[suf]), d_in).clone()
    keep = d_in.clone()
    first = run(plan, d_in)
    assert torch.equal(bits(d_in), bits(keep))
    assert float(first.abs().max()) > 0
    again = run(plan, d_in)
    assert torch.equal(bits(first), bits(again))
    side = torch.cuda.Stream()
    other = run(plan, d_in, stream=side)
    assert torch.equal(bits(first), bits(other)) and torch.equal(bits(d_in), bits(keep))


@pytest.mark.parametrize("inverse", [False, True], ids=["r2c", "c2r"])
def test_surface(inverse):
    suf, logn, P, batch = "f32", 16, 2, 3
    n, h = 1 << logn, 1 << (logn - 1)
    plan = pifft.RealPlan(n, P, batch, PREC[suf], inverse=inverse)
    inner = pifft.Plan(h, P, batch, PREC[suf], inverse=inverse)
    assert plan.is_real() == (2 if inverse else 1) and inner.is_real() == 0
    nl = plan.info.num_launches
    assert nl == inner.info.num_launches + 1
    new = 0 if inverse else nl - 1
    names = [plan.kernel_name(i) for i in range(nl)]
    assert names[new] == "void pifft::%s<float>(pifft::RealArgs)" % ("k_c2r_pre" if inverse else "k_r2c_post")
    rest = names[1:] if inverse else names[:-1]
    assert rest == [inner.kernel_name(i) for i in range(nl - 1)]  # the inner plan's own kernels
    d_in = torch.zeros(plan.info.in_elems, dtype=TDT[suf], device="cuda")
    d_in[1::7] = 0.25 + 0.5j
    want = run(plan, d_in)
    out = torch.full((plan.info.out_elems + TAIL,), complex(SENTINEL, SENTINEL), dtype=TDT[suf], device="cuda")
    ms = plan.execute_device_timed(d_in.data_ptr(), out.data_ptr(), torch.cuda.current_stream())
    assert len(ms) == nl and all(t > 0 for t in ms)
    assert torch.equal(bits(out[:plan.info.out_elems]), bits(want))
    plan.profile_start(4, pifft.PROFILE_ALL)
    for _ in range(4):
        plan.execute_device(d_in.data_ptr(), out.data_ptr(), torch.cuda.current_stream())
    used, sums, cnt = plan.profile_read()
    assert used == 4 and cnt == [4] * nl and all(s > 0 for s in sums)
    mean = plan.launch_loop([new], 3, d_in.data_ptr(), out.data_ptr(), torch.cuda.current_stream())
    assert mean > 0 and torch.equal(bits(out[:plan.info.out_elems]), bits(want))
    assert (torch.view_as_real(out[plan.info.out_elems:]).cpu().numpy() == np.float32(SENTINEL)).all()
    # the host-boundary, multi-plan, tree and workspace-tuning entry points refuse real plans
    host = np.zeros(batch * n, dtype=DT[suf])
    with pytest.raises(pifft.PifftError, match="real plans"):
        plan.execute(host, np.zeros_like(host))
    with pytest.raises(pifft.PifftError, match="real plans"):
        pifft.execute_group([plan], host, np.zeros_like(host))
    with pytest.raises(pifft.PifftError, match="real plans"):
        pifft.execute_group_kernel_times([plan])
    with pytest.raises(pifft.PifftError, match="real plans"):
        pifft.allgather([plan], [d_in.data_ptr()], [out.data_ptr()])
    with pytest.raises(pifft.PifftError, match="real plans"):
        plan.tree_device(d_in.data_ptr(), out.data_ptr(), torch.cuda.current_stream())
    with pytest.raises(pifft.PifftError, match="real plans"):
        plan.tune_workspace(d_in.data_ptr(), out.data_ptr(), torch.cuda.current_stream(), 2)
    # ... and the plan still runs afterwards
    assert torch.equal(bits(run(plan, d_in)), bits(want))
