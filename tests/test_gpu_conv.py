"""Real FFT convolution plans (pifft_plan_create_conv) on an MI355X, through the C-ABI.

A convolution plan of batch rows of n reals and one filter of taps reals:
k_conv_pad, the 1-D plan of (H, 1 worker, batch) forward, k_conv_pair -- the R2C
fix-up, the product with the filter's spectrum G and the C2R fix-up of a pair of
bins in one launch -- the same plan inverse, k_conv_crop; M the smallest power of
two >= max(n + taps - 1, 4), H = M/2.  A cyclic plan (M = n) has no pad and crop.

Truth (truth()): the convolution summed directly in long double where n * taps
<= 2^21, else the product of oracle.fft_hp transforms of the padded rows,
transformed back as hi + lo doubles (test_gpu_chirp.fft_hp2).

Yardstick (yardstick()): the same composition in the plan's precision on the
oracle, as tests/test_gpu_real.py takes its references: oracle.fft of the
padded real row, its first H + 1 bins, times those of the padded filter scaled
by 1/M, rounded; the Hermitian extension through conj . oracle.fft . conj, its
real part.

Bounds: tests/test_gpu_accuracy.py's rule on the real output, not a new number.
With e_o, m_o the yardstick's rel-L2 and worst-element errors against the truth,
    rel-L2 <= 4 max(e_o, u),   worst element <= 4 max(m_o, u) rms,
the worst element 6 where an inner chain has two or more passes: the output is
a C2R result.  Each case prints e_k/e_o and m_k/m_o
(profiles/conv_gpu_tests_figures.txt holds a run's lines).

Every execution goes through run(): d_in and d_out are carved out of larger
allocations, n NaNs on either side of d_in, n sentinel values on either side of
d_out, which must survive, and d_in keeps its bits.  The carving puts the rows
of an odd n at every 4-byte (fp64: 8-byte) residue.
"""
import functools

import numpy as np
import pytest

import pifft
import pifft_oracle as oracle
import test_gpu_accuracy as acc
from test_gpu_chirp import fft_hp2
from test_hp_reference import U

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LD, CLD = np.longdouble, np.clongdouble
DT = {"f32": np.complex64, "f64": np.complex128}
RDT = {"f32": np.float32, "f64": np.float64}
TRDT = {"f32": torch.float32, "f64": torch.float64}
TCDT = {"f32": torch.complex64, "f64": torch.complex128}
PREC = {"f32": pifft.F32, "f64": pifft.F64}
CTYPE = {"f32": "float", "f64": "double"}
VEC = {"f32": 4, "f64": 2}  # reals per work item of pad and crop
SENTINEL = -7.5e33
GRID_MAX = 262144
DIRECT_MAX = 1 << 21  # n * taps up to which the truth is summed directly

LINEAR = [(2, 2, 1), (5, 3, 3), (3, 5, 1), (1000, 25, 3), (1000, 26, 1), (1021, 17, 3), (40000, 30000, 1)]
CYCLIC = [(n, taps) for n in (4, 8, 16, 1024, 65536) for taps in (1, n)]
BIT_H = [2, 4, 8, 16, 1024, 32768]


def ibits(a):
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "c":
        a = a.view(np.float64 if a.dtype == np.complex128 else np.float32)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


# ------------------------------------------------------------ references ---
@functools.lru_cache(maxsize=None)
def host_reals(suf, count, seed):
    """count reals of the generator's values (re/im interleaved), read-only."""
    z = oracle.generate(max(count, 2), DT[suf], seed=seed, count=(count + 1) // 2)
    x = np.array(z.view(RDT[suf])[:count])
    x.setflags(write=False)
    return x


def host_input(suf, n, batch, seed=0):
    return host_reals(suf, batch * n, 0xC0F0 + n + seed)


def host_filter(suf, taps, seed=0):
    return host_reals(suf, taps, 0xF117 + taps + seed)


def m_of(n, taps, cyclic):
    return n if cyclic else pifft.conv_length(n, taps)


def padded(v, m, dtype):
    p = np.zeros(m, dtype=dtype)
    p[:len(v)] = v
    return p


def truth_row(x, h, m, out_len, cyclic):
    """One row's convolution (h already in the order it is applied) in long double."""
    n, taps = len(x), len(h)
    if n * taps <= DIRECT_MAX:
        full = np.convolve(x.astype(LD), h.astype(LD))
        if not cyclic:
            return full
        y = full[:n].copy()
        y[:len(full) - n] += full[n:]
        return y
    cdt = np.complex128 if x.dtype == np.float64 else np.complex64
    C = oracle.fft_hp(padded(x, m, cdt)) * oracle.fft_hp(padded(h, m, cdt))
    return (np.conj(fft_hp2(np.conj(C))) / LD(m)).real[:out_len]


def half_spectrum(v, suf):
    """The first H + 1 bins of oracle.fft of the real row v, in the plan's precision."""
    return oracle.fft(v.astype(DT[suf]), P=1)[:len(v) // 2 + 1]


def yardstick_row(x, G, m, out_len, suf):
    h2 = m // 2
    P = (half_spectrum(padded(x, m, RDT[suf]), suf) * G).astype(DT[suf])
    P[0], P[h2] = P[0].real, P[h2].real  # (the C2R path ignores their imaginary parts)
    full = np.concatenate([P, np.conj(P[h2 - 1:0:-1])])
    return np.conj(oracle.fft(np.conj(full), P=1)).real.astype(RDT[suf])[:out_len]


@functools.lru_cache(maxsize=4)
def references(suf, n, taps, batch, correlate, cyclic):
    """(x, h, H, O): the input rows, the filter as given, the truth and the yardstick per row; read-only."""
    m = m_of(n, taps, cyclic)
    out_len = n if cyclic else n + taps - 1
    x, h = host_input(suf, n, batch), host_filter(suf, taps)
    ha = np.array(h[::-1] if correlate else h)
    G = half_spectrum(padded(ha, m, RDT[suf]) * RDT[suf](1.0 / m), suf)
    rows = np.array(x).reshape(batch, n)
    H = np.stack([truth_row(r, ha, m, out_len, cyclic) for r in rows])
    O = np.stack([yardstick_row(r, G, m, out_len, suf) for r in rows])
    for a in (H, O):
        a.setflags(write=False)
    return x, h, H, O


# ------------------------------------------------------------- execution ---
def dev(a):
    return torch.from_numpy(np.array(a)).to("cuda")  # (a copy: the cached references are read-only)


def make(suf, n, taps, batch=1, correlate=False, cyclic=False, h=None):
    plan = pifft.ConvPlan(n, taps, batch, PREC[suf], correlate=correlate, cyclic=cyclic)
    assert plan.is_conv() == 1 and (plan.n, plan.taps, plan.m) == (n, taps, m_of(n, taps, cyclic))
    assert plan.out_len == (n if cyclic else n + taps - 1)
    if h is not None:
        set_filter(plan, h)
    return plan


def set_filter(plan, h):
    """The taps reals carved out of a larger allocation of NaNs, which they keep around them."""
    taps = plan.taps
    big = torch.full((taps + 2,), float("nan"), dtype=TRDT["f64" if h.dtype == np.float64 else "f32"], device="cuda")
    big[1:1 + taps] = dev(h)
    keep = big.clone()
    torch.cuda.synchronize()
    plan.set_filter(big[1:1 + taps].data_ptr(), torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert torch.equal(acc.bits(big), acc.bits(keep)), "the filter (or the NaNs around it) was written"


def run(plan, x):
    """Execute on the host array x (reals) with d_in and d_out carved from
    larger allocations: n NaNs around d_in, n sentinels around d_out (they
    survive), d_in bit-identical afterwards.  Returns the output as a numpy array."""
    n = plan.dims()[1]
    ni, no = plan.info.in_elems, plan.info.out_elems
    assert ni == x.size == plan.info.batch * n and no == plan.info.batch * plan.out_len
    dt = TRDT["f64" if x.dtype == np.float64 else "f32"]
    big_in = torch.full((ni + 2 * n,), float("nan"), dtype=dt, device="cuda")
    big_in[n:n + ni] = dev(x)
    big_out = torch.full((no + 2 * n,), SENTINEL, dtype=dt, device="cuda")
    d_in, d_out = big_in[n:n + ni], big_out[n:n + no]
    keep = big_in.clone()
    torch.cuda.synchronize()
    plan.execute_device(d_in.data_ptr(), d_out.data_ptr(), torch.cuda.current_stream())
    torch.cuda.synchronize()
    out = big_out.cpu().numpy()
    guard = np.concatenate([out[:n], out[n + no:]])
    assert (guard == guard.dtype.type(SENTINEL)).all(), "a sentinel beside d_out was overwritten"
    assert torch.equal(acc.bits(big_in), acc.bits(keep)), "d_in (or the NaNs around it) was written"
    return out[n:n + no]


def bounds(plan):
    """(rel-L2 factor, worst-element factor): 4 and 4; the worst element 6 where a chain has >= 2 passes."""
    chain_passes = plan.info.num_passes // 2
    return acc.FACTOR, (acc.WORST_BIN_CHAIN if chain_passes >= 2 else acc.FACTOR)


def check(label, suf, plan, got, H, O):
    """got, H, O: (batch, out_len).  Prints each row's ratios, then holds every row to the bounds."""
    fe, fm = bounds(plan)
    u = U[suf]
    rows = []
    for b, (g, h, o) in enumerate(zip(got, H, O)):
        (e_k, m_k), (e_o, m_o) = acc.errors(g, h), acc.errors(o, h)
        rows.append((e_k, e_o, m_k, m_o))
        print(f"CONV {label} row {b}: e_k {e_k:.3e} e_o {e_o:.3e} = {e_o / u:.2f} u (e_k/e_o {e_k / max(e_o, u):.2f})  "
              f"m_k {m_k:.3e} m_o {m_o:.3e} = {m_o / u:.2f} u (m_k/m_o {m_k / max(m_o, u):.2f})  bounds {fe}x {fm}x")
    for e_k, e_o, m_k, m_o in rows:
        assert e_k <= fe * max(e_o, u), f"rel-L2 {e_k:.3e} > {fe} x max({e_o:.3e}, u)"
        assert m_k <= fm * max(m_o, u), f"worst element {m_k:.3e} rms > {fm} x max({m_o:.3e}, u)"
    return rows


# ---- 1. accuracy ------------------------------------------------------------
@pytest.mark.parametrize("correlate", [False, True], ids=["convolve", "correlate"])
@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("n,taps,batch", LINEAR)
def test_linear_accuracy(n, taps, batch, suf, correlate):
    x, h, H, O = references(suf, n, taps, batch, correlate, False)
    plan = make(suf, n, taps, batch, correlate, h=h)
    assert plan.info.num_passes == (4 if (n, taps) == (40000, 30000) else 2)
    got = run(plan, x).reshape(batch, -1)
    check(f"{'cor' if correlate else 'conv'} {suf} n={n} taps={taps} batch={batch}", suf, plan, got, H, O)


@pytest.mark.parametrize("correlate", [False, True], ids=["convolve", "correlate"])
@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("n,taps", CYCLIC)
def test_cyclic_accuracy(n, taps, suf, correlate):
    batch = 3 if n <= 1024 else 1
    x, h, H, O = references(suf, n, taps, batch, correlate, True)
    plan = make(suf, n, taps, batch, correlate, cyclic=True, h=h)
    assert plan.info.num_passes == (4 if n == 65536 else 2) and plan.out_len == n
    got = run(plan, x).reshape(batch, -1)
    check(f"cyclic {'cor' if correlate else 'conv'} {suf} n={n} taps={taps} batch={batch}", suf, plan, got, H, O)


# ---- 2. three-pass chains ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def three_pass_m(suf):
    """The smallest M whose inner chains have three passes, from the dry run."""
    for logm in range(12, 27):
        if pifft.dry_run_conv(1 << logm, 1, 1, PREC[suf], cyclic=True)["num_passes"] == 6:
            return 1 << logm
    raise AssertionError("no three-pass chain up to 2^26")


SPARSE_TAPS = 4  # one nonzero tap, the last: y[j] = c x[j - 3]


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_three_pass_chains(suf):
    """A sparse signal and a filter of one nonzero tap: the truth is the signal
    shifted and scaled, exact in long double; no long transform on the host but
    the yardstick's."""
    m = three_pass_m(suf)
    taps, n = SPARSE_TAPS, m - SPARSE_TAPS + 1  # L = M, n odd
    at = (0, 1, 2, n // 2, n // 2 + 1, n - 3, n - 2, n - 1)
    v = oracle.generate(8, np.complex64, seed=0xC0F0).view(np.float32)  # (exact in both precisions)
    x = np.zeros(n, dtype=RDT[suf])
    x[list(at)] = v[:8]
    h = np.zeros(taps, dtype=RDT[suf])
    h[taps - 1] = v[8]
    plan = make(suf, n, taps, 1, h=h)
    assert plan.info.num_passes == 6 and plan.m == m and plan.out_len == m
    assert pifft.dry_run_conv(m // 2, 1, 1, PREC[suf], cyclic=True)["num_passes"] < 6
    got = run(plan, x)
    H = np.zeros(m, dtype=LD)
    H[taps - 1:] = x.astype(LD) * LD(h[taps - 1])
    G = half_spectrum(padded(h, m, RDT[suf]) * RDT[suf](1.0 / m), suf)
    O = yardstick_row(x, G, m, m, suf)
    check(f"conv {suf} n={n} taps={taps} sparse", suf, plan, got[None], H[None], O[None])


# ---- 3. bit for bit ---------------------------------------------------------
def real_r2c(suf, m, batch, x):
    """RealPlan R2C of batch rows of m reals: (batch, m/2 + 1) bins."""
    plan = pifft.RealPlan(m, 1, batch, PREC[suf])
    d_in = dev(x)
    d_out = torch.empty(batch * (m // 2 + 1), dtype=TCDT[suf], device="cuda")
    plan.execute_device(d_in.data_ptr(), d_out.data_ptr(), torch.cuda.current_stream())
    torch.cuda.synchronize()
    return d_out.cpu().numpy().reshape(batch, m // 2 + 1)


def real_c2r(suf, m, batch, X):
    plan = pifft.RealPlan(m, 1, batch, PREC[suf], inverse=True)
    d_in = dev(X.reshape(-1))
    d_out = torch.empty(batch * m, dtype=TRDT[suf], device="cuda")
    plan.execute_device(d_in.data_ptr(), d_out.data_ptr(), torch.cuda.current_stream())
    torch.cuda.synchronize()
    return d_out.cpu().numpy().reshape(batch, m)


def launches_differ(h2, batch, suf):
    """Whether the planner's launches for (H, 1 worker) differ between batch 1 and `batch`."""
    a, b = pifft.dry_run(h2, 1, 1, PREC[suf]), pifft.dry_run(h2, 1, batch, PREC[suf])
    return any(a[k] != b[k] for k in ("launch_kind", "launch_mode", "radix", "lines", "vpt"))


def batch_dependent_case():
    """(H, batch) where the filter's batch-1 chain differs from the executions', if the dry run shows one."""
    for h2 in (16, 64, 256, 1024, 4096, 16384, 32768):
        for batch in (3, 16, 64, 256):
            if any(launches_differ(h2, batch, suf) for suf in ("f64", "f32")):
                return [(h2, batch)]
    return []


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("h2,batch", [(h2, 3 if h2 <= 1024 else 1) for h2 in BIT_H] + batch_dependent_case())
def test_cyclic_plan_is_the_three_launch_composition_bit_for_bit(h2, batch, suf):
    """RealPlan R2C, a host product in the kernel's operation order on separate
    real arrays, RealPlan C2R.  G: RealPlan R2C (batch 1) of the padded filter
    scaled by 1/M."""
    m = 2 * h2
    taps = min(m, 5)
    x, h = host_input(suf, m, batch), host_filter(suf, taps)
    got = run(make(suf, m, taps, batch, cyclic=True, h=h), x).reshape(batch, m)
    G = real_r2c(suf, m, 1, padded(h, m, RDT[suf]) * RDT[suf](1.0 / m))[0]
    X = real_r2c(suf, m, batch, x)
    xr, xi, gr, gi = X.real.copy(), X.imag.copy(), G.real.copy(), G.imag.copy()
    assert xr.dtype == RDT[suf] and not gi[0] and not gi[h2] and not xi[:, 0].any() and not xi[:, h2].any()
    P = np.empty_like(X)
    P.real = xr * gr - xi * gi
    P.imag = xr * gi + xi * gr
    want = real_c2r(suf, m, batch, P)
    assert np.array_equal(ibits(got), ibits(want))


@pytest.mark.parametrize("correlate", [False, True], ids=["convolve", "correlate"])
@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("n,taps,batch", [(2, 2, 1), (5, 3, 3), (3, 5, 1), (1000, 26, 1), (1021, 17, 3), (40000, 30000, 1)])
def test_linear_plan_is_the_cyclic_plan_on_padded_rows(n, taps, batch, suf, correlate):
    m, L = pifft.conv_length(n, taps), n + taps - 1
    x, h = host_input(suf, n, batch), host_filter(suf, taps)
    got = run(make(suf, n, taps, batch, correlate, h=h), x).reshape(batch, L)
    xp = np.zeros((batch, m), dtype=RDT[suf])
    xp[:, :n] = np.array(x).reshape(batch, n)
    want = run(make(suf, m, taps, batch, correlate, cyclic=True, h=h), xp.reshape(-1)).reshape(batch, m)[:, :L]
    assert np.array_equal(ibits(got), ibits(want))
    # correlate: convolve with the filter reversed on the host
    if correlate:
        rev = run(make(suf, n, taps, batch, h=np.array(h[::-1])), x).reshape(batch, L)
        assert np.array_equal(ibits(got), ibits(rev))


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("n,taps,batch,cyclic", [(1021, 17, 3, False), (40000, 30000, 1, False), (1024, 1024, 3, True)])
def test_second_execution_and_second_filter(n, taps, batch, cyclic, suf):
    """The inverse chain leaves its result in Z: the pad [n, M) is rewritten on
    every execution.  A second pifft_conv_set_filter replaces G altogether."""
    x1, x2 = host_input(suf, n, batch, 1), host_input(suf, n, batch, 2)
    h1, h2 = host_filter(suf, taps, 1), host_filter(suf, taps, 2)
    plan = make(suf, n, taps, batch, cyclic=cyclic, h=h1)
    first = run(plan, x1)
    again = run(plan, x1)
    assert np.array_equal(ibits(first), ibits(again))
    second = run(plan, x2)
    fresh1 = make(suf, n, taps, batch, cyclic=cyclic, h=h1)
    assert not np.array_equal(ibits(first), ibits(second))
    assert np.array_equal(ibits(second), ibits(run(fresh1, x2)))
    set_filter(plan, h2)
    refiltered = run(plan, x2)
    assert not np.array_equal(ibits(refiltered), ibits(second))
    assert np.array_equal(ibits(refiltered), ibits(run(make(suf, n, taps, batch, cyclic=cyclic, h=h2), x2)))


# ---- 4. launches ------------------------------------------------------------
def new_grid(units):
    return min((units + 255) // 256, GRID_MAX)


def new_units(suf, n, taps, batch, cyclic):
    """Work items of (pad, pair, crop) launches."""
    m = m_of(n, taps, cyclic)
    L = n if cyclic else n + taps - 1
    v, pv = VEC[suf], (2 if suf == "f32" else 1)
    return batch * (m // v), batch * ((m // 4) // pv + 1), batch * ((L + v - 1) // v)


@pytest.mark.parametrize("cyclic", [False, True], ids=["linear", "cyclic"])
@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("n,taps,batch", [(4, 1, 1), (1024, 17, 3), (65536, 30000, 1)])
def test_kernel_names_and_grids(n, taps, batch, suf, cyclic):
    m = m_of(n, taps, cyclic)
    T = CTYPE[suf]
    plan = make(suf, n, taps, batch, cyclic=cyclic)
    chains = [pifft.Plan(m // 2, 1, batch, PREC[suf], device=0, inverse=inv) for inv in (False, True)]
    inner = [[c.kernel_name(i) for i in range(c.info.num_launches)] for c in chains]
    names = [plan.kernel_name(i) for i in range(plan.info.num_launches)]
    pad, crop = ([] if cyclic else [f"void pifft::k_conv_pad<{T}>(pifft::ConvArgs)"],
                 [] if cyclic else [f"void pifft::k_conv_crop<{T}>(pifft::ConvArgs)"])
    assert names == pad + inner[0] + [f"void pifft::k_conv_pair<{T}>(pifft::ConvArgs)"] + inner[1] + crop
    fn = list(plan.info.launch_fn[:plan.info.num_launches])
    seen = {}
    assert fn == [seen.setdefault(k, len(seen)) for k in names]
    # grids: the inner launches' from the inner plans' dry runs, the new ones' from their work items
    dry = [[g for _, g in pifft.dry_run_aux(m // 2, 1, batch, PREC[suf], inverse=inv)] for inv in (False, True)]
    grids = [plan.launch_grid(i) for i in range(plan.info.num_launches)]
    u_pad, u_pair, u_crop = new_units(suf, n, taps, batch, cyclic)
    assert grids == ([] if cyclic else [new_grid(u_pad)]) + dry[0] + [new_grid(u_pair)] + dry[1] + \
        ([] if cyclic else [new_grid(u_crop)])
    assert plan.describe() == pifft.dry_run_conv(n, taps, batch, PREC[suf], cyclic=cyclic)
    with pytest.raises(pifft.PifftError, match="out of range"):
        plan.launch_grid(plan.info.num_launches)


# ---- 5. grid-stride second trips --------------------------------------------
@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_second_trips(suf, monkeypatch):
    n, taps, batch = 1021, 17, 3
    x, h = host_input(suf, n, batch), host_filter(suf, taps)
    free_plan = make(suf, n, taps, batch, h=h)
    free = run(free_plan, x)
    nl = free_plan.info.num_launches
    new = [i for i in range(nl) if free_plan.info.launch_kind[i] in (11, 12, 13)]
    units = new_units(suf, n, taps, batch, False)
    full = [free_plan.launch_grid(i) for i in new]
    assert len(new) == 3 and full == [new_grid(u) for u in units] and min(full) > 3
    monkeypatch.setenv("PIFFT_TUNING", "1")
    for cap in (1, 3, min(full) - 1):
        monkeypatch.setenv("PIFFT_STRIDE_GRID_MAX", str(cap))
        plan = make(suf, n, taps, batch, h=h)  # (its G too comes from capped filter and fix-up launches)
        monkeypatch.delenv("PIFFT_STRIDE_GRID_MAX")
        grids = [plan.launch_grid(i) for i in new]
        assert grids == [cap] * 3
        # fewer threads than work items in every new launch: its threads make a second trip
        assert all(g * 256 < u for g, u in zip(grids, units))
        assert [plan.launch_grid(i) for i in range(nl) if i not in new] == \
            [free_plan.launch_grid(i) for i in range(nl) if i not in new]
        got = run(plan, x)
        assert np.array_equal(ibits(got), ibits(free)), f"cap {cap}"


# ---- 6. the surface ---------------------------------------------------------
@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_surface(suf):
    n, taps, batch = 1000, 26, 3
    plan = make(suf, n, taps, batch)
    assert plan.is_conv() == 1 and plan.is_real() == 0 and plan.is_chirp() == 0 and plan.dims() == (1, n)
    assert pifft.Plan(1 << 10, 1, 1, PREC[suf]).is_conv() == 0
    d = plan.describe()
    assert d["launch_kind"] == ["conv_pad", "pass", "conv_pair", "pass", "conv_crop"] and d["conv"] and d["n"] == n
    x, h = host_input(suf, n, batch), host_filter(suf, taps)
    dx = dev(x)
    out = torch.empty(plan.info.out_elems, dtype=dx.dtype, device="cuda")
    # no filter yet: every entry point that would run the launches refuses
    for call in (lambda: plan.execute_device(dx.data_ptr(), out.data_ptr()),
                 lambda: plan.execute_device_timed(dx.data_ptr(), out.data_ptr()),
                 lambda: plan.launch_loop([0], 1, dx.data_ptr(), out.data_ptr())):
        with pytest.raises(pifft.PifftError, match="no filter set"):
            call()
    set_filter(plan, h)
    a = run(plan, x)
    # the timed and profiled paths run the same launches
    ms = plan.execute_device_timed(dx.data_ptr(), out.data_ptr(), torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert len(ms) == 5 and all(t > 0 for t in ms) and np.array_equal(ibits(out.cpu().numpy()), ibits(a))
    plan.profile_start(10, pifft.PROFILE_SAMPLED)
    for _ in range(10):
        plan.execute_device(dx.data_ptr(), out.data_ptr(), torch.cuda.current_stream())
    used, sums, counts = plan.profile_read()
    assert used == 10 and counts == [1] * 5 and all(s > 0 for s in sums)
    assert plan.launch_loop([2], 3, dx.data_ptr(), out.data_ptr(), torch.cuda.current_stream()) > 0
    assert np.array_equal(ibits(out.cpu().numpy()), ibits(a))
    # refused: the host boundary, multi-plan calls, the tree, workspace tuning, in-place buffers
    host = np.zeros(batch * n, dtype=DT[suf])
    cdx = torch.zeros(batch * n, dtype=TCDT[suf], device="cuda")
    cout = torch.zeros(batch * n, dtype=TCDT[suf], device="cuda")
    for call in (lambda: plan.execute(host),
                 lambda: pifft.execute_group([plan], host),
                 lambda: pifft.execute_group_kernel_times([plan]),
                 lambda: pifft.allgather([plan], [cdx.data_ptr()], [cout.data_ptr()]),
                 lambda: plan.tree_device(cdx.data_ptr(), cout.data_ptr()),
                 lambda: plan.tune_workspace(cdx.data_ptr(), cout.data_ptr())):
        with pytest.raises(pifft.PifftError, match="convolution plans"):
            call()
    with pytest.raises(pifft.PifftError, match="in-place"):
        plan.execute_device(dx.data_ptr(), dx.data_ptr())
    with pytest.raises(pifft.PifftError, match="not a convolution plan"):
        pifft.ConvPlan.set_filter(pifft.Plan(1 << 10, 1, 1, PREC[suf]), dx.data_ptr())
