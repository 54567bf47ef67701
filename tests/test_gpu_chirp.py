"""Arbitrary-length 1-D transforms (pifft_plan_create_chirp) on an MI355X, through the C-ABI.

A chirp plan of batch rows of N values, N no power of two, is Bluestein's
chirp-z algorithm: k_chirp_pre, the 1-D plan of (M, 1 worker, batch) forward,
k_spectrum_mul, the same plan inverse, k_chirp_post; M the smallest power of
two >= 2N - 1, w[j] = e^{-i pi j^2/N}.

Truth (truth()): the same chirp-z composition in long double on oracle.fft_hp
-- a and b widened as hi + lo doubles and the two transforms added, pi taken as
4 arctan(1) in long double -- checked below against directly summed long-double
DFTs at N <= 1021 (test_truth_against_direct_sums).

Yardstick (yardstick()): the composition in the plan's precision on the oracle
-- w rounded once from long double, oracle.fft forward, swap . oracle.fft . swap
inverse, Bt from the fp64 oracle.fft of the rounded b, scaled by 1/M and rounded
once as the library does.

Bounds: tests/test_gpu_accuracy.py's rule, not a new number.  With e_o, m_o the
yardstick's rel-L2 and worst-bin errors against the truth on the same input,
    rel-L2 <= 4 max(e_o, u),   worst bin <= 4 max(m_o, u) rms,
the worst bin 6 at fp32 where a chain has two or more passes (DESIGN.md section
13).  The factor is not fitted to the kernels.  Each case prints e_k/e_o and
m_k/m_o (profiles/chirp_gpu_tests_figures.txt holds a run's lines).

Every execution goes through run(): d_in and d_out are carved out of larger
allocations, N NaNs on either side of d_in, N sentinel values on either side of
d_out, which must survive, and d_in keeps its bits.  The carving puts the
buffers of an odd N at 8 mod 16 at fp32.
"""
import functools

import numpy as np
import pytest

import pifft
import pifft_oracle as oracle
import test_gpu_accuracy as acc
from test_hp_reference import U, norm_ld

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LD, CLD = np.longdouble, np.clongdouble
DT = {"f32": np.complex64, "f64": np.complex128}
PREC = {"f32": pifft.F32, "f64": pifft.F64}
CTYPE = {"f32": "float", "f64": "double"}
PI = 4 * np.arctan(LD(1))
SENTINEL = -7.5e33
GRID_MAX = 262144

ACCURACY_N = [3, 5, 7, 12, 17, 100, 127, 129, 1000, 1021, 4097, 8191, 8193, 10007, 40000]
INVERSE_N = [7, 1021, 8193]
BATCHED = [(17, 5), (1021, 3), (1000, 3)]
THREE_PASS_N = 786433
THREE_PASS_AT = (0, 1, 2, 393216, 524287, 786430, 786431, 786432)


def swap(z):
    return (z.imag + 1j * z.real).astype(z.dtype)


def ibits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.float64 if a.dtype == np.complex128 else np.float32).view(
        np.int64 if a.dtype == np.complex128 else np.int32)


# ------------------------------------------------------------ references ---
@functools.lru_cache(maxsize=None)
def chirp_ld(n):
    """w[j] = e^{-i pi (j^2 mod 2n)/n} in long double; the exponent in integers."""
    j = np.arange(n, dtype=np.uint64)
    r = (j * j) % np.uint64(2 * n)  # (j^2 < 2^54)
    ang = PI * (r.astype(LD) / LD(n))
    w = (np.cos(ang) - 1j * np.sin(ang)).astype(CLD)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def b_ld(n):
    m = pifft.chirp_length(n)
    w = chirp_ld(n)
    b = np.zeros(m, dtype=CLD)
    b[:n] = np.conj(w)
    b[m - n + 1:] = np.conj(w[:0:-1])  # b[m - j] = conj w[j], 1 <= j < n
    b.setflags(write=False)
    return b


def fft_hp2(v):
    """fft_hp of a long-double vector: widened as hi + lo doubles, the two transforms added."""
    hi = v.astype(np.complex128)
    lo = (v - hi.astype(CLD)).astype(np.complex128)
    return oracle.fft_hp(hi) + oracle.fft_hp(lo)


@functools.lru_cache(maxsize=4)
def B_ld(n):
    return fft_hp2(b_ld(n))


def truth(x):
    """The DFT of one row x (any n >= 3) by chirp-z in long double."""
    n = len(x)
    m = pifft.chirp_length(n)
    w = chirp_ld(n)
    a = np.zeros(m, dtype=CLD)
    a[:n] = x.astype(CLD) * w
    C = fft_hp2(a) * B_ld(n)
    c = np.conj(fft_hp2(np.conj(C))) / LD(m)
    return w * c[:n]


@functools.lru_cache(maxsize=None)
def bt_of(suf, n):
    """Bt as the library fixes it: the fp64 transform of b rounded to fp64,
    scaled by the exact 1/M, rounded once to the plan's precision."""
    m = pifft.chirp_length(n)
    return (oracle.fft(b_ld(n).astype(np.complex128), P=1) * (1.0 / m)).astype(DT[suf])


def yardstick(x, suf):
    """The same composition in the plan's precision on the oracle."""
    n = len(x)
    m = pifft.chirp_length(n)
    w = chirp_ld(n).astype(DT[suf])
    a = np.zeros(m, dtype=DT[suf])
    a[:n] = x * w
    C = (oracle.fft(a, P=1) * bt_of(suf, n)).astype(DT[suf])
    c = swap(oracle.fft(swap(C), P=1))
    return (w * c[:n]).astype(DT[suf])


def direct_ld(x, inverse=False):
    """Every bin summed directly in long double, the exponent j k mod n in integers."""
    n = len(x)
    j = np.arange(n, dtype=np.uint64)
    e = (j[:, None] * j[None, :]) % np.uint64(n)
    ang = 2 * PI * (e.astype(LD) / LD(n))
    W = np.cos(ang) + (1j if inverse else -1j) * np.sin(ang)
    return W @ x.astype(CLD)


@functools.lru_cache(maxsize=None)
def host_input(suf, n, batch, seed=0):
    x = oracle.generate(n, DT[suf], seed=0xC412 + n + seed, count=batch * n)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=8)
def references(suf, n, batch, inverse=False, seed=0):
    """(x, H, O): the input rows, the truth and the yardstick per row; read-only.
    inverse: swap(.(swap(x))) of both."""
    x = host_input(suf, n, batch, seed)
    rows = [swap(r) if inverse else r for r in np.array(x).reshape(batch, n)]
    H = np.stack([truth(r) for r in rows])
    O = np.stack([yardstick(r, suf) for r in rows])
    if inverse:
        H, O = np.stack([swap(h) for h in H]), np.stack([swap(o) for o in O])
    for a in (H, O):
        a.setflags(write=False)
    return x, H, O


# ------------------------------------------------------------- execution ---
def run(plan, x):
    """Execute on the host array x with d_in and d_out carved from larger
    allocations: N NaNs around d_in, N sentinels around d_out (they survive),
    d_in bit-identical afterwards.  Returns the output as a numpy array."""
    n = plan.dims()[1]
    ne = plan.info.in_elems
    assert plan.info.out_elems == ne == x.size
    dt = torch.complex128 if x.dtype == np.complex128 else torch.complex64
    big_in = torch.full((ne + 2 * n,), complex(float("nan"), float("nan")), dtype=dt, device="cuda")
    big_in[n:n + ne] = torch.from_numpy(np.array(x)).to("cuda")
    big_out = torch.full((ne + 2 * n,), complex(SENTINEL, SENTINEL), dtype=dt, device="cuda")
    d_in, d_out = big_in[n:n + ne], big_out[n:n + ne]
    keep = big_in.clone()
    torch.cuda.synchronize()
    plan.execute_device(d_in.data_ptr(), d_out.data_ptr(), torch.cuda.current_stream())
    torch.cuda.synchronize()
    out = big_out.cpu().numpy()
    guard = np.concatenate([out[:n], out[n + ne:]]).view(out.real.dtype)
    assert (guard == guard.dtype.type(SENTINEL)).all(), "a sentinel beside d_out was overwritten"
    assert torch.equal(acc.bits(big_in), acc.bits(keep)), "d_in (or the NaNs around it) was written"
    return out[n:n + ne]


def make(suf, n, batch=1, inverse=False):
    return pifft.ChirpPlan(n, batch, PREC[suf], inverse=inverse)


def bounds(suf, plan):
    """(rel-L2 factor, worst-bin factor): 4 and 4; the worst bin 6 at fp32 where a chain has >= 2 passes."""
    chain_passes = plan.info.num_passes // 2
    return acc.FACTOR, (acc.WORST_BIN_CHAIN if suf == "f32" and chain_passes >= 2 else acc.FACTOR)


def check(label, suf, plan, got, H, O):
    """got, H, O: (batch, n).  Prints each row's ratios, then holds every row to the bounds."""
    fe, fm = bounds(suf, plan)
    u = U[suf]
    rows = []
    for b, (g, h, o) in enumerate(zip(got, H, O)):
        (e_k, m_k), (e_o, m_o) = acc.errors(g, h), acc.errors(o, h)
        rows.append((e_k, e_o, m_k, m_o))
        print(f"CHIRP {label} row {b}: e_k {e_k:.3e} e_o {e_o:.3e} = {e_o / u:.2f} u (e_k/e_o {e_k / max(e_o, u):.2f})  "
              f"m_k {m_k:.3e} m_o {m_o:.3e} = {m_o / u:.2f} u (m_k/m_o {m_k / max(m_o, u):.2f})  bounds {fe}x {fm}x")
    for e_k, e_o, m_k, m_o in rows:
        assert e_k <= fe * max(e_o, u), f"rel-L2 {e_k:.3e} > {fe} x max({e_o:.3e}, u)"
        assert m_k <= fm * max(m_o, u), f"worst bin {m_k:.3e} rms > {fm} x max({m_o:.3e}, u)"
    return rows


# ---- 0. the truth itself ----------------------------------------------------
@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("n", [n for n in ACCURACY_N if n <= 1021])
def test_truth_against_direct_sums(n, suf):
    """Long double rounds at 2^-64 = 5.4e-20.  The truth goes through three
    transforms of log2 M <= 12 levels and three pointwise products: some 40
    roundings a value, adding in quadrature, about 6 x 2^-64 = 3.4e-19 in
    rel-L2; held to 32 x 2^-64 = 1.7e-18, and the worst of at most 1021 bins
    (four standard deviations) to 128 x 2^-64 = 6.9e-18 rms."""
    x = np.array(host_input(suf, n, 1))
    for inverse in (False, True):
        D = direct_ld(x, inverse)
        T = swap(truth(swap(x))) if inverse else truth(x)
        e, m = acc.errors(T, D)
        print(f"truth n = {n} {suf} inverse = {inverse}: rel-L2 {e:.2e}, worst bin {m:.2e} rms")
        assert e <= 32 * 2.0 ** -64 and m <= 128 * 2.0 ** -64


# ---- 1. accuracy ------------------------------------------------------------
@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("n", ACCURACY_N)
def test_forward_accuracy(n, suf):
    x, H, O = references(suf, n, 1)
    plan = make(suf, n)
    want_passes = 1 if n <= 8191 else 2
    assert plan.info.num_passes == 2 * want_passes and plan.info.local_n == pifft.chirp_length(n)
    got = run(plan, x)
    check(f"fwd {suf} n={n}", suf, plan, got[None], H, O)


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("n", INVERSE_N)
def test_inverse_accuracy(n, suf):
    x, H, O = references(suf, n, 1, True)
    plan = make(suf, n, inverse=True)
    assert plan.describe()["inverse"]
    got = run(plan, x)
    check(f"inv {suf} n={n}", suf, plan, got[None], H, O)


# ---- 2. three-pass chains ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def sparse_input(suf):
    n = THREE_PASS_N
    v = oracle.generate(8, np.complex64, seed=0xC412)  # (exact in both precisions: one truth serves both)
    x = np.zeros(n, dtype=DT[suf])
    x[list(THREE_PASS_AT)] = v
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def sparse_truth():
    """The direct long-double sum of the 8 terms of every bin; j k mod n in integers."""
    n = THREE_PASS_N
    x = sparse_input("f64")
    k = np.arange(n, dtype=np.uint64)
    X = np.zeros(n, dtype=CLD)
    for j in THREE_PASS_AT:
        ang = 2 * PI * (((np.uint64(j) * k) % np.uint64(n)).astype(LD) / LD(n))  # (j k < 2^40)
        X += CLD(x[j]) * (np.cos(ang) - 1j * np.sin(ang))
    X.setflags(write=False)
    return X


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_three_pass_chains(suf):
    n = THREE_PASS_N
    x = sparse_input(suf)
    plan = make(suf, n)
    assert plan.info.num_passes == 6 and plan.info.local_n == 1 << 21
    got = run(plan, x)
    check(f"fwd {suf} n={n} sparse", suf, plan, got[None], sparse_truth()[None], yardstick(np.array(x), suf)[None])


# ---- 3. the inverse ---------------------------------------------------------
@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("n", INVERSE_N)
def test_inverse_is_the_swapped_forward_bit_for_bit(n, suf):
    x = host_input(suf, n, 1)
    inv = run(make(suf, n, inverse=True), x)
    fwd = run(make(suf, n), swap(np.array(x)))
    assert np.array_equal(ibits(inv), ibits(swap(fwd)))


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("n", INVERSE_N)
def test_round_trip(n, suf):
    """inverse(forward(x)) against n x in rel-L2, under the sum of the two
    plans' bounds: the forward result's error passes through the exact inverse
    (unitary up to the factor n) unchanged in rel-L2, the inverse plan adds its
    own on the input it was given.  The worst bin is not held: the inverse
    spreads a bin error of the forward result over all samples."""
    x, _, O = references(suf, n, 1)
    fwd, inv = make(suf, n), make(suf, n, inverse=True)
    X = run(fwd, x)
    back = run(inv, X)
    u = U[suf]
    e_of = acc.errors(O[0], truth(np.array(x)))[0]
    e_oi = acc.errors(swap(yardstick(swap(X), suf)), swap(truth(swap(X))))[0]
    want = np.array(x).astype(CLD) * LD(n)
    e = float(norm_ld(back.astype(CLD) - want) / norm_ld(want))
    bound = acc.FACTOR * max(e_of, u) + acc.FACTOR * max(e_oi, u)
    print(f"CHIRP round trip {suf} n={n}: rel-L2 {e:.3e}, bound {bound:.3e} ({e / bound:.2f})")
    assert e <= bound


# ---- 4. batch and alignment -------------------------------------------------
@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("n,batch", BATCHED)
def test_batch_rows(n, batch, suf):
    plan = make(suf, n, batch)
    one = np.array(host_input(suf, n, 1))
    got = run(plan, np.tile(one, batch)).reshape(batch, n)
    for b in range(1, batch):
        assert np.array_equal(ibits(got[b]), ibits(got[0])), f"row {b} differs from row 0 on the same input"
    x, H, O = references(suf, n, batch)
    got = run(plan, x).reshape(batch, n)
    check(f"fwd {suf} n={n} batch={batch}", suf, plan, got, H, O)


# ---- 6. the dirty pad -------------------------------------------------------
@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("n,batch", [(100, 1), (1021, 3), (8193, 1)])
def test_second_execution_equals_a_fresh_plan(n, batch, suf):
    """The inverse chain leaves its result in Z: the pad [N, M) is rewritten on every execution."""
    x1, x2 = host_input(suf, n, batch, 1), host_input(suf, n, batch, 2)
    plan = make(suf, n, batch)
    first = run(plan, x1)
    second = run(plan, x2)
    fresh = run(make(suf, n, batch), x2)
    assert not np.array_equal(ibits(first), ibits(second))
    assert np.array_equal(ibits(second), ibits(fresh))


# ---- 7. launches ------------------------------------------------------------
def new_grid(units):
    return min((units + 255) // 256, GRID_MAX)


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("n,batch", [(7, 1), (1021, 3), (8193, 1), (1000, 3)])
def test_kernel_names_and_grids(n, batch, suf, inverse):
    m = pifft.chirp_length(n)
    T, vec = CTYPE[suf], (2 if suf == "f32" else 1)
    plan = make(suf, n, batch, inverse)
    chains = [pifft.Plan(m, 1, batch, PREC[suf], device=0, inverse=inv) for inv in (False, True)]
    inner = [[c.kernel_name(i) for i in range(c.info.num_launches)] for c in chains]
    names = [plan.kernel_name(i) for i in range(plan.info.num_launches)]
    assert names == ([f"void pifft::k_chirp_pre<{T}, {1 if inverse else 0}>(pifft::ChirpArgs)"] + inner[0] +
                     [f"void pifft::k_spectrum_mul<{T}>(pifft::ChirpArgs)"] + inner[1] +
                     [f"void pifft::k_chirp_post<{T}, {2 if inverse else 0}>(pifft::ChirpArgs)"])
    fn = list(plan.info.launch_fn[:plan.info.num_launches])
    seen = {}
    assert fn == [seen.setdefault(k, len(seen)) for k in names]
    # grids: the inner launches' from the inner plans' dry runs, the new ones' from their work items
    dry = [[g for _, g in pifft.dry_run_aux(m, 1, batch, PREC[suf], inverse=inv)] for inv in (False, True)]
    grids = [plan.launch_grid(i) for i in range(plan.info.num_launches)]
    assert grids == ([new_grid(batch * m // vec)] + dry[0] + [new_grid(batch * m // vec)] + dry[1] +
                     [new_grid(batch * ((n + vec - 1) // vec))])
    assert plan.describe() == pifft.dry_run_chirp(n, batch, PREC[suf], inverse=inverse)
    with pytest.raises(pifft.PifftError, match="out of range"):
        plan.launch_grid(plan.info.num_launches)


# ---- 8. grid-stride second trips --------------------------------------------
@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_second_trips(suf, monkeypatch):
    n, batch = 1021, 3
    x = host_input(suf, n, batch)
    free_plan = make(suf, n, batch)
    free = run(free_plan, x)
    nl = free_plan.info.num_launches
    new = [i for i in range(nl) if free_plan.info.launch_kind[i] in (8, 9, 10)]
    assert len(new) == 3 and all(free_plan.launch_grid(i) > 3 for i in new)
    for cap in (1, 3):
        monkeypatch.setenv("PIFFT_STRIDE_GRID_MAX", str(cap))
        plan = make(suf, n, batch)  # (its Bt too comes from capped fill and rounding launches)
        monkeypatch.delenv("PIFFT_STRIDE_GRID_MAX")
        assert [plan.launch_grid(i) for i in new] == [cap] * 3
        assert [plan.launch_grid(i) for i in range(nl) if i not in new] == \
            [free_plan.launch_grid(i) for i in range(nl) if i not in new]
        got = run(plan, x)
        assert np.array_equal(ibits(got), ibits(free)), f"cap {cap}"


# ---- 9. the surface ---------------------------------------------------------
@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_surface(suf):
    n, batch = 1000, 3
    plan = make(suf, n, batch)
    assert plan.is_chirp() == 1 and plan.is_real() == 0 and plan.dims() == (1, n)
    assert pifft.Plan(1 << 10, 1, 1, PREC[suf]).is_chirp() == 0
    d = plan.describe()
    assert d["launch_kind"] == ["chirp_pre", "pass", "spectrum_mul", "pass", "chirp_post"] and d["chirp"] and d["n"] == n
    # plan_1d: the dispatch on n
    p2, pc = pifft.plan_1d(1024, batch, PREC[suf]), pifft.plan_1d(n, batch, PREC[suf], inverse=True)
    assert type(p2) is pifft.Plan and p2.is_chirp() == 0 and p2.dims() == (1, 1024) and p2.info.workers == 1
    assert type(pc) is pifft.ChirpPlan and pc.is_chirp() == 1 and pc.describe()["inverse"]
    x = host_input(suf, n, batch)
    a = run(plan, x)
    # the timed and profiled paths run the same launches
    dx = torch.from_numpy(np.array(x)).to("cuda")
    out = torch.empty(plan.info.out_elems, dtype=dx.dtype, device="cuda")
    ms = plan.execute_device_timed(dx.data_ptr(), out.data_ptr(), torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert len(ms) == 5 and all(t > 0 for t in ms) and np.array_equal(ibits(out.cpu().numpy()), ibits(a))
    plan.profile_start(10, pifft.PROFILE_SAMPLED)
    for _ in range(10):
        plan.execute_device(dx.data_ptr(), out.data_ptr(), torch.cuda.current_stream())
    used, sums, counts = plan.profile_read()
    assert used == 10 and counts == [1] * 5 and all(s > 0 for s in sums)
    assert plan.launch_loop([0], 3, dx.data_ptr(), out.data_ptr(), torch.cuda.current_stream()) > 0
    assert np.array_equal(ibits(out.cpu().numpy()), ibits(a))
    # refused: the host boundary, multi-plan calls, the tree, workspace tuning, in-place buffers
    host = np.array(x)
    for call in (lambda: plan.execute(host),
                 lambda: pifft.execute_group([plan], host),
                 lambda: pifft.execute_group_kernel_times([plan]),
                 lambda: pifft.allgather([plan], [dx.data_ptr()], [out.data_ptr()]),
                 lambda: plan.tree_device(dx.data_ptr(), out.data_ptr()),
                 lambda: plan.tune_workspace(dx.data_ptr(), out.data_ptr())):
        with pytest.raises(pifft.PifftError, match="chirp plans"):
            call()
    with pytest.raises(pifft.PifftError, match="in-place"):
        plan.execute_device(dx.data_ptr(), dx.data_ptr())
