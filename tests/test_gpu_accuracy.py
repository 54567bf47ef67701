"""Kernel accuracy on an MI355X against a long-double FFT, bounded by the oracle's own error.

The other GPU tests hold the kernels to the north-star bars (rel-L2 1e-12 fp64,
1e-5 log2 N fp32): acceptance limits about a thousand times the error the
kernels deliver, under which a twiddle exponent off by one in a late stage
(a phase error of 2 pi / N) or one power too many in a twiddle chain passes.
Here every plan structure is measured against oracle.fft_hp (an 80-bit
radix-2 FFT, oracle/fft_hp.c; checked on the CPU in tests/test_hp_reference.py)
and held to a multiple of what the ORACLE -- a plain radix-2 transform in the
plan's own precision with correctly rounded twiddles -- loses on the same input:

    e_k = rel-L2(kernel, H)        e_o = rel-L2(oracle, H)
    m_k = max |kernel - H| / rms   m_o = max |oracle - H| / rms
    e_k <= 4 max(e_o, u)           m_k <= 4 max(m_o, u)      per transform
    (m_k: 6 in the one derived case below),

u = 2^-24 / 2^-53, all in long double.  Why 4: the
recorded figures put two- and three-pass fp32 plans at 2.3-2.7 times the
oracle (the inter-pass twiddle chain: w = hi lo squared up to three times,
then w^k by up to three more products), fp64 near 1.3; the factored tree's two
products per level at P = 32 bring the model to about 3.0; the rest is room
for the spread of a maximum over N bins.  tests/test_hp_reference.py keeps the
oracle's error under 2 u sqrt(log2 N), so 4 e_o never exceeds 8 u sqrt(log2 N).
The factor is not fitted to any kernel's measured error; a case above it is a
finding to explain from the kernel source, not a number to raise.

One finding, and its derived bound: the WORST BIN of
fp32 plans of two or more passes, and of C2R plans of two or more inner passes
in either precision, is held to 6, not 4, times the oracle's; every rel-L2,
and the worst bin of everything else (fp64 complex and R2C multi-pass plans
included: their model gives 2.7-3.1), stays at 4.  A later pass multiplies the
16 inputs of each first-stage butterfly by step^k, and step = fl(hi lo) is ONE
value per line: its relative error delta (three rounded operands) enters
every output of the line with weight k <= 15, so the R final bins of a
last-pass line share one |delta|.  The error variance then differs from line
to line (measured, tools/accuracy_line_spread.py: 0.17 to 10 times the mean,
the oracle's lines 0.7 to 1.7), and the maximum over N bins sits in the line
with the largest |delta|: the errors are a scale mixture, not the
equal-variance Gaussians the factor 4 assumed.  Counting roundings (delta: two
table entries and a product, then squarings and power products) puts the
chain at 6.5 u per inter-pass twiddle and the worst bin at 4.4-4.7 times an
oracle error of 0.66 u sqrt(log2 N); times the same 1.3 for the spread of a
maximum: 5.7-6.1.  That oracle error is the fp32 oracle's, and the C2R
yardstick's in both precisions: on Hermitian input the oracle's arithmetic
roundings are conjugate-symmetric and stay in the real part, while the fp64
oracle's larger twiddle-angle error lands in the imaginary part, which the
yardstick (the real part, as tests/test_gpu_real.py takes it) drops -- e_o of
fp64 C2R is half that of R2C, of fp32 C2R the same.  The model's r h alone
(4.4-4.7) is BELOW the largest measured ratios (4.9-5.7 on three-pass fp32
plans): the bound rests on the 1.3 allowance, the largest case sits 5 % under
it, and another seed could exceed it with no kernel change; the seeds are
fixed, so a given build gives the same figures on every run.

Every execution runs with 8 sentinel values behind d_out, which must survive,
and must leave d_in bit-identical -- the buffer discipline the real-plan tests
check, here for the complex plans too.

Cases: the forward plan of every structure of tests/test_gpu_inverse.py's
SHAPES and SHAPES_BY_PREC (fp32 all, fp64 up to 2^22); two inverse plans; the
tuning forms at the shapes tests/test_gpu_parity.py runs them; the factored
tree table (default only above 2^22) forced at small N by
PIFFT_TREE_DIRECT_MAX_LOG=0; R2C / C2R at tests/test_gpu_real.py's inputs; and
the three inputs whose transform is exact in any precision, bit for bit.  Every
shape is one an existing GPU test already plans: no k_pass instance is added.

Not covered, because the long-double reference alone costs ~8 s or more there:
the fp64 2^23, P = 2 shape (MODE 11 with three passes) and the fp32 2^27
packed shape (32 values per thread).  No 4-pass or packed-fp32 plan exists at
a small N either: the pruned library has no such instances.
"""
import functools
import math

import numpy as np
import pytest

import pifft
import pifft_dist
import pifft_oracle as oracle
import test_gpu_real as real_tests
from test_gpu_inverse import SHAPES, SHAPES_BY_PREC
from test_gpu_parity import _bitrev_perm
from test_hp_reference import U, exact_cases, norm_ld

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DT = {"f32": np.complex64, "f64": np.complex128}
RDT = {"f32": np.float32, "f64": np.float64}
PREC = {"f32": pifft.F32, "f64": pifft.F64}
NAT, SL, BR, SEP = pifft.OUT_NATURAL, pifft.OUT_SLICES, pifft.OUT_BITREV, pifft.SEPARATE_TREE
SENTINEL = -7.5e33
TAIL = 8
FACTOR = 4  # times the oracle's error; see the module docstring
WORST_BIN_CHAIN = 6  # worst bin, >= 2 passes, where the yardstick is 0.66 u sqrt(log2 N): fp32, and C2R


def bits(t):
    r = torch.view_as_real(t) if t.is_complex() else t
    return r.view(torch.int64 if r.dtype == torch.float64 else torch.int32)


def run(plan, d_in, tree=False):
    """Execute (or, tree: pifft_tree_device) into a buffer with TAIL sentinel
    values behind it: the tail survives and d_in keeps its bits."""
    ne = plan.info.out_elems
    assert d_in.numel() == plan.info.in_elems
    out = torch.full((ne + TAIL,), complex(SENTINEL, SENTINEL), dtype=d_in.dtype, device="cuda")
    keep = d_in.clone()
    torch.cuda.synchronize()
    (plan.tree_device if tree else plan.execute_device)(d_in.data_ptr(), out.data_ptr(), torch.cuda.current_stream())
    torch.cuda.synchronize()
    tail = torch.view_as_real(out[ne:]).cpu().numpy()
    assert (tail == tail.dtype.type(SENTINEL)).all(), "the sentinel behind d_out was overwritten"
    assert torch.equal(bits(d_in), bits(keep)), "d_in was written"
    return out[:ne].cpu().numpy()


def dev(x):
    return torch.from_numpy(np.array(x)).to("cuda")  # (a copy: the cached references are read-only)


def hp(x):
    """The high-precision DFT of one transform: fft_hp; for fp32 data above
    2^16, numpy's fp64 FFT (within 1e-15 of fft_hp up to 2^22, the largest size
    here: tests/test_hp_reference.py; 1e-8 of the fp32 errors measured) to save time."""
    if x.dtype == np.complex64 and len(x) > 1 << 16:
        return np.fft.fft(x.astype(np.complex128)).astype(np.clongdouble)
    return oracle.fft_hp(x)


@functools.lru_cache(maxsize=3)
def references(suf, logn, batch, inverse=False):
    """(x, H, O) of a size: the generator's input (one seed per size: every plan
    structure of a size shares these), H = fft_hp and O = oracle.fft(P=1) per
    transform, natural order, read-only.  inverse: conj(.(conj(x))) of both."""
    n = 1 << logn
    x = oracle.generate(n, DT[suf], seed=0xACC0 + logn, count=batch * n)
    rows = [np.conj(x[b * n:(b + 1) * n]) if inverse else x[b * n:(b + 1) * n] for b in range(batch)]
    H = np.stack([hp(r) for r in rows])
    O = np.stack([oracle.fft(r, P=1) for r in rows])
    if inverse:
        H, O = np.conj(H), np.conj(O)
    for a in (x, H, O):
        a.setflags(write=False)
    return x, H, O


def plan_order(X, P, first, count, flags):
    """A natural-order transform in a plan's output order: natural, the
    workers' slices X[bitrev(q) + P k] back to back, or the bit-reversed
    scratch order's segments of the workers."""
    n = len(X)
    m = n // P
    order = flags & 3
    if order == NAT:
        return X
    if order == SL:
        return np.concatenate([pifft_dist.slice_of_natural(X, P, first + j) for j in range(count)])
    return X[_bitrev_perm(n)][first * m:(first + count) * m]


def errors(got, H):
    """(rel-L2, worst bin / rms) of got against H, in long double."""
    d = got.astype(H.dtype) - H
    nh = norm_ld(H)
    return float(norm_ld(d) / nh), float(np.sqrt(np.max(d.real * d.real + d.imag * d.imag)) / (nh / math.sqrt(H.size)))


def check(label, suf, got, H, O, passes=0, c2r=False, shared_worst_bin=None):
    """got, H, O: (batch, per-transform) arrays in one order; passes: the plan's
    num_passes.  Prints the transform with the largest ratio, then holds every
    transform's rel-L2 to FACTOR and its worst bin to FACTOR -- or to
    WORST_BIN_CHAIN where an inter-pass twiddle chain exists (passes >= 2) and
    the derivation gives more than 4: fp32 plans and C2R plans.
    shared_worst_bin (tests/test_gpu_instances.py only; no test of this file
    passes it): that derivation evaluated for the many cases that share the
    bound there, in its place where it is the larger."""
    worst = WORST_BIN_CHAIN if passes >= 2 and (suf == "f32" or c2r) else FACTOR
    if shared_worst_bin is not None:
        worst = max(worst, shared_worst_bin)
    assert got.shape == H.shape == O.shape, (got.shape, H.shape, O.shape)
    u = U[suf]
    rows = []
    for g, h, o in zip(got, H, O):
        (e_k, m_k), (e_o, m_o) = errors(g, h), errors(o, h)
        rows.append((max(e_k / max(e_o, u), m_k / max(m_o, u)), e_k, e_o, m_k, m_o))
    _, e_k, e_o, m_k, m_o = max(rows)
    print(f"ACC {label}: e_k {e_k:.3e} e_o {e_o:.3e} ({e_k / max(e_o, u):.2f}x)  "
          f"m_k {m_k:.3e} m_o {m_o:.3e} ({m_k / max(m_o, u):.2f}x)  bounds {FACTOR}x {worst}x")
    for _, e_k, e_o, m_k, m_o in rows:
        assert e_k <= FACTOR * max(e_o, u), f"rel-L2 {e_k:.3e} > {FACTOR} x max({e_o:.3e}, u)"
        assert m_k <= worst * max(m_o, u), f"worst bin {m_k:.3e} rms > {worst} x max({m_o:.3e}, u)"


def check_plan(label, suf, plan, shape, inverse=False):
    """Run a complex plan of `shape` on the size's shared input; returns its output."""
    logn, P, first, count, flags, batch = shape
    x, H, O = references(suf, logn, batch, inverse)
    got = run(plan, dev(x))
    check(label, suf, got.reshape(batch, -1),
          np.stack([plan_order(h, P, first, count, flags) for h in H]),
          np.stack([plan_order(o, P, first, count, flags) for o in O]), plan.info.num_passes)
    return got


def make_plan(suf, shape, inverse=False):
    logn, P, first, count, flags, batch = shape
    return pifft.Plan(1 << logn, P, batch, PREC[suf], first=first, count=count, device=0, flags=flags, inverse=inverse)


def shape_id(shape):
    logn, P, first, count, flags, batch = shape
    return f"2^{logn}-P{P}-q{first}+{count}-fl{flags}-b{batch}"


# ---------------------------------------------------------- forward plans ---
# fp32: every structure; fp64: those up to 2^22.  Sorted by size, so the cached
# references of a size serve its cases back to back.
FORWARD = sorted([(suf, sh, k, m) for sh, k, m in SHAPES for suf in ("f64", "f32")] +
                 [(suf, sh, k, m) for sh, by in SHAPES_BY_PREC for suf, (k, m) in by.items()
                  if suf == "f32" or sh[0] <= 22],
                 key=lambda c: (c[0], c[1][0], c[1][5]))
KINDS = {(suf, sh): (k, m) for suf, sh, k, m in FORWARD}


@pytest.mark.parametrize("case", FORWARD, ids=lambda c: f"{c[0]}-{shape_id(c[1])}")
def test_forward_plan(case):
    suf, shape, kinds, modes = case
    plan = make_plan(suf, shape)
    d = plan.describe()
    assert d["launch_kind"] == kinds and d["launch_mode"] == modes, d
    check_plan(f"fwd {suf} {shape_id(shape)} {'/'.join(kinds)} {modes}", suf, plan, shape)


# ---------------------------------------------------------- inverse plans ---
@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("logn,P", [(16, 8), (21, 1)])
def test_inverse_plan(suf, logn, P):
    """Against conj(fft_hp(conj(x))); the yardstick conj(oracle.fft(conj(x)))."""
    shape = (logn, P, 0, P, NAT, 1)
    plan = make_plan(suf, shape, inverse=True)
    assert plan.describe()["inverse"]
    check_plan(f"inv {suf} {shape_id(shape)} {'/'.join(plan.describe()['launch_kind'])}", suf, plan, shape, inverse=True)


# ----------------------------------------------------------- tuning forms ---
# (environment, precision, shape, launch kinds, modes, values per thread): at
# the shapes tests/test_gpu_parity.py and tests/test_gpu_inverse.py run them
TP, PS, T, IL = "tree+pass", "pass", "tree", "interleave"
TUNING = [
    ({"PIFFT_LAST_VPT": "16"}, "f64", (18, 4, 3, 1, SL, 1), [TP, PS], [3, 2], [8, 16]),
    ({"PIFFT_LAST_VPT": "8", "PIFFT_LAST_C": "8"}, "f64", (18, 4, 3, 1, SL, 1), [TP, PS], [3, 2], [8, 8]),
    ({"PIFFT_NT": "1"}, "f64", (16, 1, 0, 1, NAT, 1), [PS, PS], [1, 2], [16, 16]),
    ({"PIFFT_NT": "1"}, "f32", (18, 1, 0, 1, NAT, 1), [PS, PS], [1, 2], [16, 16]),
    ({"PIFFT_WIL_VPT": "16", "PIFFT_WIL_FUSE": "0"}, "f64", (18, 8, 0, 8, NAT, 2), [T, PS, PS], [0, 10, 10], [16, 16]),
    ({"PIFFT_WORKER_IL": "0"}, "f64", (18, 8, 0, 8, NAT, 2), [T, PS, PS], [0, 1, 2], [16, 16]),
    ({"PIFFT_WIL_ONE_LAUNCH": "0"}, "f64", (12, 32, 0, 32, NAT, 1), [T, T, PS, IL], [0, 0, 0, 0], [16]),
    ({"PIFFT_WIL_ONE_LAUNCH": "0"}, "f32", (12, 32, 0, 32, NAT, 1), [T, T, PS, IL], [0, 0, 0, 0], [16]),
]


def env_id(env):
    return ",".join(f"{k[len('PIFFT_'):]}={v}" for k, v in env.items())


@pytest.mark.parametrize("env,suf,shape,kinds,modes,vpt", TUNING,
                         ids=[f"{env_id(c[0])}-{c[1]}-{shape_id(c[2])}" for c in TUNING])
def test_tuning_form(env, suf, shape, kinds, modes, vpt, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    plan = make_plan(suf, shape)
    d = plan.describe()
    assert d["launch_kind"] == kinds and d["launch_mode"] == modes and d["vpt"] == vpt, d
    if "PIFFT_NT" in env:
        assert ", 1, 1, 0, 16>" in plan.kernel_name(0) and ", 2, 1, 0, 16>" in plan.kernel_name(1)  # NTS = 1
    check_plan(f"tun {suf} {shape_id(shape)} {env_id(env)}", suf, plan, shape)


# ---------------------------------------------- the factored tree table ---
FACTORED = [(16, 2, 0, 2, SL, 1),    # tree, pass, pass
            (20, 32, 0, 32, NAT, 1),  # two tree launches
            (16, 2, 1, 1, SL, 1),    # MODE 3
            (14, 2, 0, 2, NAT, 1),   # MODE 11, then a pass
            (17, 2, 1, 1, SL, 3)]    # MODE 3 at the other width, batched


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("shape", FACTORED, ids=shape_id)
def test_factored_tree_table(suf, shape, monkeypatch):
    """TREE_TW_FACTORED (a two-level base hi lo times a compile-time root; the
    default only where N > 2^22) at small N: PIFFT_TREE_DIRECT_MAX_LOG=0
    changes the launches' arguments, not the kernels -- the same launch list,
    other bytes."""
    kinds, modes = KINDS[(suf, shape)]
    x, _, _ = references(suf, shape[0], shape[5])
    dflt = run(make_plan(suf, shape), dev(x))
    monkeypatch.setenv("PIFFT_TREE_DIRECT_MAX_LOG", "0")
    plan = make_plan(suf, shape)
    d = plan.describe()
    assert d["launch_kind"] == kinds and d["launch_mode"] == modes, d
    got = check_plan(f"fac {suf} {shape_id(shape)} {'/'.join(kinds)} {modes}", suf, plan, shape)
    assert got.tobytes() != dflt.tobytes(), "PIFFT_TREE_DIRECT_MAX_LOG=0 changed nothing"


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_factored_tree_stage(suf, monkeypatch):
    """pifft_tree_device with the factored table against the long-double tree
    (fft_hp's first log2 P levels); the yardstick the oracle's tree_segment."""
    shape = logn, P, _, _, _, _ = FACTORED[0]
    x, _, _ = references(suf, logn, 1)
    Th = oracle.tree_hp(x, P)
    To = np.concatenate([oracle.tree_segment(x, P, q) for q in range(P)])
    dflt = run(make_plan(suf, shape), dev(x), tree=True)
    assert dflt.tobytes() == To.tobytes()  # the reference table: the oracle's bits
    monkeypatch.setenv("PIFFT_TREE_DIRECT_MAX_LOG", "0")
    got = run(make_plan(suf, shape), dev(x), tree=True)
    assert got.tobytes() != dflt.tobytes(), "PIFFT_TREE_DIRECT_MAX_LOG=0 changed nothing"
    check(f"fac {suf} {shape_id(shape)} tree_device", suf, got[None], Th[None], To[None])


# -------------------------------------------------------------- real plans ---
REAL = [(4, 1, 1), (11, 32, 3), (15, 1, 1), (16, 1, 1), (22, 1, 1)]
assert set(REAL) <= set(real_tests.SHAPES)


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("shape", REAL, ids=real_tests.shape_id)
def test_r2c(suf, shape):
    """tests/test_gpu_real.py's input rows; H = fft_hp of the real row."""
    logn, P, batch = shape
    n, h = 1 << logn, 1 << (logn - 1)
    z = oracle.generate(n, DT[suf], count=batch * h)  # = real_tests.device_input, bit for bit
    x = z.view(RDT[suf]).reshape(batch, n)
    H = np.stack([hp(r.astype(DT[suf]))[:h + 1] for r in x])
    O = np.array(real_tests.reference_r2c(suf, logn, batch)).reshape(batch, h + 1)
    plan = pifft.RealPlan(n, P, batch, PREC[suf])
    got = run(plan, dev(z))
    check(f"r2c {suf} {real_tests.shape_id(shape)} {'/'.join(plan.describe()['launch_kind'])}", suf,
          got.reshape(batch, h + 1), H, O, plan.info.num_passes)


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("shape", REAL, ids=real_tests.shape_id)
def test_c2r(suf, shape):
    """tests/test_gpu_real.py's half spectra; H = conj(fft_hp(conj(.))) of the
    Hermitian extension (real up to fft_hp's own rounding: its real part)."""
    logn, P, batch = shape
    n, h = 1 << logn, 1 << (logn - 1)
    X, y = real_tests.reference_c2r(suf, logn, batch)
    Xr = np.array(X).reshape(batch, h + 1)
    H = np.stack([hp(np.conj(np.concatenate([r, np.conj(r[h - 1:0:-1])]))).real.astype(np.clongdouble) for r in Xr])
    plan = pifft.RealPlan(n, P, batch, PREC[suf], inverse=True)
    got = run(plan, dev(X)).view(RDT[suf])
    check(f"c2r {suf} {real_tests.shape_id(shape)} {'/'.join(plan.describe()['launch_kind'])}", suf,
          got.reshape(batch, n), H, np.array(y).reshape(batch, n), plan.info.num_passes, c2r=True)


# ------------------------------------------------------------ exact inputs ---
# constant 1 -> N delta_0; a unit impulse at 0 -> all ones; 0,1,0,1,... -> N/2
# at bin 0, -N/2 at bin N/2.  Every non-zero value of these transforms meets
# only the twiddle w^0, which is exactly (1, -0) in every table (cos 0 and
# sin 0 are exact), in every hi[0] lo[0] product, and in every power of it;
# zeros stay zeros.  So every plan structure must give the exact answer.
EXACT = [(suf, sh) for sh, _, _ in SHAPES if sh[0] <= 17 for suf in ("f64", "f32")]


def assert_exact(plan, suf, shape):
    logn, P, first, count, flags, batch = shape
    for name, x, X in exact_cases(1 << logn, DT[suf]):
        got = run(plan, dev(np.tile(x, batch))).reshape(batch, -1)
        want = plan_order(X, P, first, count, flags)
        for b in range(batch):
            assert np.array_equal(got[b], want), f"{name}, transform {b}: {np.count_nonzero(got[b] != want)} values differ"


@pytest.mark.parametrize("suf,shape", EXACT, ids=lambda v: v if isinstance(v, str) else shape_id(v))
def test_exact_inputs(suf, shape):
    plan = make_plan(suf, shape)
    kinds, modes = KINDS[(suf, shape)]
    assert plan.describe()["launch_kind"] == kinds and plan.describe()["launch_mode"] == modes
    assert_exact(plan, suf, shape)


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_exact_inputs_factored_tree(suf, monkeypatch):
    monkeypatch.setenv("PIFFT_TREE_DIRECT_MAX_LOG", "0")
    assert_exact(make_plan(suf, FACTORED[0]), suf, FACTORED[0])
