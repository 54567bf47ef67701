"""Inverse transforms (PIFFT_INVERSE) on an MI355X, through the C-ABI.

The sharp oracle: with swap(a + bi) = b + ai, IDFT(x) = swap(DFT(swap(x))),
and an inverse plan is the forward plan whose launch reading d_in swaps what
it loads and whose launch writing d_out swaps what it stores -- so
inverse(x) must equal swap(forward(swap(x))) BIT FOR BIT, on every plan
structure (where the two swaps land differs per structure; each shape below is
the smallest at which one appears, and asserts it).  Beside that: the
reference (conj(oracle.fft(conj(x)))) at the forward parity tests' own bounds,
round trips at twice those bounds (two transforms' errors add), the host and
multi-plan entry points, kernel names, and the CLI's -i.
"""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import pifft
import pifft_oracle as oracle
from golden_io import rel_l2

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DT = {"f32": np.complex64, "f64": np.complex128}
TDT = {"f32": torch.complex64, "f64": torch.complex128}
PREC = {"f32": pifft.F32, "f64": pifft.F64}
NAT, SL, BR, SEP = pifft.OUT_NATURAL, pifft.OUT_SLICES, pifft.OUT_BITREV, pifft.SEPARATE_TREE
T, PS, IL, TP = "tree", "pass", "interleave", "tree+pass"


def tol(suf, n):
    """The forward parity tests' bounds (tests/test_gpu_parity.py)."""
    return 1e-12 if suf == "f64" else 1e-5 * math.log2(n)


def swap(t):
    """re <-> im, on the device."""
    return torch.view_as_complex(torch.view_as_real(t).flip(-1).contiguous())


def bits(t):
    r = torch.view_as_real(t)
    return r.view(torch.int64 if r.dtype == torch.float64 else torch.int32)


def device_input(suf, count, n, seed=0x5EED):
    x = torch.empty(count, dtype=TDT[suf], device="cuda")
    pifft.generate_device(x.data_ptr(), count, n, PREC[suf], seed)
    return x


def run(plan, d_in):
    d_out = torch.empty(plan.info.out_elems, dtype=d_in.dtype, device="cuda")
    plan.execute_device(d_in.data_ptr(), d_out.data_ptr(), torch.cuda.current_stream())
    torch.cuda.synchronize()
    return d_out


def plans(suf, logn, P, first, count, flags, batch):
    kw = dict(first=first, count=count, device=0, flags=flags)
    return (pifft.Plan(1 << logn, P, batch, PREC[suf], **kw),
            pifft.Plan(1 << logn, P, batch, PREC[suf], inverse=True, **kw))


def assert_bitwise_identity(fwd, inv, x):
    """inverse(x) == swap(forward(swap(x))), same bytes; and the input untouched."""
    keep = x.clone()
    got = run(inv, x)
    want = swap(run(fwd, swap(x)))
    assert torch.equal(bits(x), bits(keep))
    assert got.shape == want.shape
    assert torch.equal(bits(got), bits(want))
    assert float(got.abs().max()) > 0  # (not two buffers of zeros)


# (log2 N, P, first, count, flags, batch) -> launch kinds, k_pass modes; by
# precision where the planner's choice differs.  Dry runs of the planner.
SHAPES = [
    # single pass, both swaps in one launch
    ((1, 1, 0, 1, NAT, 1), [PS], [0]),
    ((13, 1, 0, 1, NAT, 1), [PS], [0]),
    ((4, 1, 0, 1, BR, 1), [PS], [4]),
    # tree only (M = 1): both swaps in one tree launch; then tree + interleave
    ((1, 2, 0, 2, SL, 1), [T], [0]),
    ((1, 2, 0, 2, NAT, 1), [T, IL], [0, 0]),
    # two tree launches: in on the first, out on the second (or on the interleave)
    ((5, 32, 0, 32, SL, 1), [T, T], [0, 0]),
    ((5, 32, 0, 32, NAT, 1), [T, T, IL], [0, 0, 0]),
    # tree, then a single pass carrying the out swap only
    ((2, 2, 0, 2, NAT, 1), [T, PS, IL], [0, 0, 0]),
    ((2, 2, 0, 2, SL, 1), [T, PS], [0, 0]),
    ((2, 2, 0, 2, BR, 1), [T, PS], [0, 4]),
    # the natural-order store of a last pass
    ((11, 128, 0, 128, NAT, 3), [T, T, PS], [0, 0, 0]),
    # one-launch MODE 11
    ((10, 2, 0, 2, NAT, 1), [TP], [11]),
    ((10, 32, 0, 32, NAT, 1), [TP], [11]),
    ((14, 2, 0, 2, NAT, 1), [TP, PS], [11, 10]),
    ((15, 1, 0, 1, NAT, 1), [PS, PS], [1, 2]),
    ((15, 1, 0, 1, BR, 1), [PS, PS], [1, 6]),
    # fused one-worker tree (MODE 3) at 8 and 16 values per thread
    ((16, 2, 1, 1, SL, 1), [TP, PS], [3, 2]),
    ((17, 2, 1, 1, SL, 3), [TP, PS], [3, 2]),
    # tree, 1, 2: the first pass reads the tree's output -- the forward kernel
    ((16, 2, 0, 2, SL, 1), [T, PS, PS], [0, 1, 2]),
    ((16, 2, 0, 2, NAT | SEP, 1), [T, PS, PS], [0, 10, 10]),
    ((20, 32, 0, 32, NAT, 1), [T, T, PS, PS], [0, 0, 1, 2]),
    ((21, 1, 0, 1, NAT, 1), [PS, PS, PS], [1, 2, 2]),
    ((22, 2, 1, 1, SL, 1), [TP, PS, PS], [3, 2, 2]),
]
# shapes whose plan depends on the precision: (shape, {suf: (kinds, modes)})
SHAPES_BY_PREC = [
    ((16, 1, 0, 1, NAT, 1), {"f64": ([PS, PS], [1, 2])}),  # last pass at 8 values per thread
    ((18, 8, 0, 8, NAT, 1), {"f64": ([TP, PS], [11, 10])}),
    ((20, 32, 0, 32, NAT, 3), {"f64": ([T, T, PS, PS], [0, 0, 1, 2]),
                               "f32": ([T, T, PS, PS, IL], [0, 0, 1, 2, 0])}),  # fp32: ends in an interleave launch
    ((23, 2, 0, 2, NAT, 1), {"f64": ([TP, PS, PS], [11, 10, 10])}),
    ((21, 2, 0, 2, NAT, 3), {"f32": ([TP, PS, PS], [11, 10, 10])}),
    # the tiled interleave launch's twin (fp64 from P = 32) and, fp64 P = 16, the 4-level
    # worker-interleaved tree launch's
    ((16, 32, 0, 32, NAT, 1), {"f64": ([T, T, PS, IL], [0, 0, 0, 0]), "f32": ([T, T, PS, IL], [0, 0, 0, 0])}),
    ((18, 16, 0, 16, NAT, 1), {"f64": ([T, PS, PS], [0, 10, 10]), "f32": ([TP, PS], [11, 10])}),
]
CASES = [(suf, sh, k, m) for sh, k, m in SHAPES for suf in ("f64", "f32")] + \
        [(suf, sh, k, m) for sh, by in SHAPES_BY_PREC for suf, (k, m) in by.items()]


def case_id(c):
    suf, (logn, P, first, count, flags, batch), _, _ = c
    return f"{suf}-2^{logn}-P{P}-q{first}+{count}-fl{flags}-b{batch}"


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_inverse_is_swap_forward_swap_bitwise(case):
    suf, (logn, P, first, count, flags, batch), kinds, modes = case
    fwd, inv = plans(suf, logn, P, first, count, flags, batch)
    d = inv.describe()
    assert d["inverse"] and not fwd.describe()["inverse"]
    assert d["launch_kind"] == kinds and d["launch_mode"] == modes, d
    assert fwd.describe()["launch_kind"] == kinds and fwd.describe()["launch_mode"] == modes
    if (logn, P, count) == (16, 1, 1) or (logn, P) == (18, 8):
        assert d["vpt"][-1] == 8
    if (logn, first) in ((16, 1), (17, 1)):
        assert d["vpt"][0] == (8 if logn == 16 else 16)
    if (logn, P, batch) == (11, 128, 3):
        assert d["natural_store"]
    assert_bitwise_identity(fwd, inv, device_input(suf, batch << logn, 1 << logn))


@pytest.mark.parametrize("suf,logn", [("f64", 16), ("f32", 18)])
def test_non_temporal_form(suf, logn, monkeypatch):
    """The modes 1 then 2 plan with PIFFT_NT=1: the non-temporal instances.  At
    2^15 (the smallest 1-then-2 plan) the planner has no non-temporal instance
    in either direction -- 'no pass decomposition', forward and inverse alike;
    2^16 (fp64) and 2^18 (fp32) are the smallest sizes at which it has them
    (dry runs under PIFFT_NT=1)."""
    monkeypatch.setenv("PIFFT_NT", "1")
    for inverse in (False, True):
        with pytest.raises(pifft.PifftError, match="no pass decomposition"):
            pifft.dry_run(1 << 15, 1, 1, PREC[suf], inverse=inverse)
        if logn > 16:
            with pytest.raises(pifft.PifftError, match="no pass decomposition"):
                pifft.dry_run(1 << (logn - 1), 1, 1, PREC[suf], inverse=inverse)
    fwd, inv = plans(suf, logn, 1, 0, 1, NAT, 1)
    assert inv.describe()["launch_mode"] == [1, 2]
    assert ", 1, 1, 0, 16>" in fwd.kernel_name(0) and ", 2, 1, 0, 16>" in fwd.kernel_name(1)  # NTS = 1
    assert ", 1, 1, 0, 16, 1>" in inv.kernel_name(0) and ", 2, 1, 0, 16, 2>" in inv.kernel_name(1)
    assert_bitwise_identity(fwd, inv, device_input(suf, 1 << logn, 1 << logn))


def test_packed_fp32():
    """The packed fp32 passes at 32 values per thread: the default plan of fp32
    2^27, P = 1 -- the smallest size the planner gives them."""
    n = 1 << 27
    fwd, inv = plans("f32", 27, 1, 0, 1, NAT, 1)
    assert inv.describe()["vpt"] == [32, 32, 32] and inv.describe()["launch_mode"] == [1, 2, 2]
    assert_bitwise_identity(fwd, inv, device_input("f32", n, n))


@functools.lru_cache(maxsize=None)
def reference_inverse(suf, logn, P, batch):
    """(x, conj(oracle.fft(conj(x), P))) per transform of the batch, computed once."""
    n = 1 << logn
    x = oracle.generate(n, DT[suf], count=batch * n)
    y = np.concatenate([np.conj(oracle.fft(np.conj(x[b * n:(b + 1) * n]), P)) for b in range(batch)])
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("logn,P,batch", [(10, 4, 1), (16, 8, 1), (20, 8, 1), (21, 1, 1), (12, 1, 64)])
def test_inverse_against_the_reference(suf, logn, P, batch):
    n = 1 << logn
    x, want = reference_inverse(suf, logn, P, batch)
    plan = pifft.Plan(n, P, batch, PREC[suf], inverse=True)
    got = run(plan, torch.from_numpy(np.array(x)).to("cuda")).cpu().numpy()
    err = rel_l2(got, want)
    print(f"{suf} 2^{logn} P={P} batch={batch}: rel-L2 {err:.3e} (bound {tol(suf, n):.1e})")
    assert err <= tol(suf, n)


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("logn,P", [(20, 8), (22, 1)])
def test_round_trip(suf, logn, P):
    n = 1 << logn
    x = device_input(suf, n, n)
    X = run(pifft.Plan(n, P, 1, PREC[suf]), x)
    back = run(pifft.Plan(n, P, 1, PREC[suf], inverse=True), X) / n
    err = float(torch.linalg.vector_norm((back - x).to(torch.complex128)) /
                torch.linalg.vector_norm(x.to(torch.complex128)))
    print(f"{suf} 2^{logn} P={P}: round trip rel-L2 {err:.3e} (bound {2 * tol(suf, n):.1e})")
    assert err <= 2 * tol(suf, n)


def test_host_and_group_entry_points():
    """Plan.execute, execute_group over two slice plans on device 0 and
    allgather give the inverse too."""
    suf, logn, P = "f64", 16, 8
    n = 1 << logn
    x, want = reference_inverse(suf, logn, P, 1)
    out = np.zeros(n, dtype=DT[suf])
    pifft.Plan(n, P, 1, PREC[suf], inverse=True).execute(np.array(x), out)
    assert rel_l2(out, want) <= tol(suf, n)
    halves = [pifft.Plan(n, P, 1, PREC[suf], first=q, count=P // 2, device=0, flags=SL, inverse=True)
              for q in (0, P // 2)]
    out2 = np.zeros(n, dtype=DT[suf])
    pifft.execute_group(halves, np.array(x), out2)
    assert rel_l2(out2, want) <= tol(suf, n)
    t1, t2 = pifft.execute_group_kernel_times(halves)
    assert t1 >= 0 and t2 > 0
    # allgather of the two plans' device results
    d_in = torch.from_numpy(np.array(x)).to("cuda")
    sl = [run(p, d_in) for p in halves]
    nat = torch.empty(n, dtype=TDT[suf], device="cuda")
    pifft.allgather(halves, [s.data_ptr() for s in sl], [nat.data_ptr(), None])
    torch.cuda.synchronize()
    assert rel_l2(nat.cpu().numpy(), want) <= tol(suf, n)
    assert np.array_equal(nat.cpu().numpy(), out2)
    # the timed and profiled entry points run the same launches
    p = halves[0]
    d_out = torch.empty(p.info.out_elems, dtype=TDT[suf], device="cuda")
    ms = p.execute_device_timed(d_in.data_ptr(), d_out.data_ptr(), torch.cuda.current_stream())
    assert len(ms) == p.info.num_launches and torch.equal(bits(d_out), bits(sl[0]))
    p.tune_workspace(d_in.data_ptr(), d_out.data_ptr(), torch.cuda.current_stream(), 2)
    torch.cuda.synchronize()
    assert torch.equal(bits(d_out), bits(sl[0]))


def test_mixed_directions_are_refused():
    n, P = 1 << 12, 4
    f = pifft.Plan(n, P, 1, pifft.F64, first=0, count=2, device=0, flags=SL)
    i = pifft.Plan(n, P, 1, pifft.F64, first=2, count=2, device=0, flags=SL, inverse=True)
    x = oracle.generate(n, np.complex128)
    with pytest.raises(pifft.PifftError, match="share the direction"):
        pifft.execute_group([f, i], x, np.zeros_like(x))
    a = torch.zeros(n // 2, dtype=torch.complex128, device="cuda")
    b = torch.zeros(n // 2, dtype=torch.complex128, device="cuda")
    nat = torch.zeros(n, dtype=torch.complex128, device="cuda")
    with pytest.raises(pifft.PifftError, match="share the direction"):
        pifft.allgather([f, i], [a.data_ptr(), b.data_ptr()], [nat.data_ptr(), None])


def test_tree_device_is_forward_only():
    n, P = 1 << 12, 4
    inv = pifft.Plan(n, P, 1, pifft.F64, first=0, count=P, device=0, flags=SL, inverse=True)
    x = torch.zeros(n, dtype=torch.complex128, device="cuda")
    seg = torch.zeros(n, dtype=torch.complex128, device="cuda")
    with pytest.raises(pifft.PifftError, match="forward plans only"):
        inv.tree_device(x.data_ptr(), seg.data_ptr(), torch.cuda.current_stream())


def test_kernel_names():
    n = 1 << 28
    fwd = pifft.Plan(n, 1, 1, pifft.F64)
    names = [fwd.kernel_name(i) for i in range(fwd.info.num_launches)]
    assert len(names) == 3 and all(nm.startswith("void pifft::k_pass<double, ") for nm in names)
    assert names[-1] == "void pifft::k_pass<double, 1024, 8, 2, 1, 0, 16>(pifft::PassArgs)"
    inv = pifft.Plan(n, 1, 1, pifft.F64, inverse=True)
    inames = [inv.kernel_name(i) for i in range(inv.info.num_launches)]
    assert inames[1] == names[1]  # the middle launch is the forward kernel
    assert inames[0] != names[0] and inames[2] != names[2]
    assert inames[0] == names[0].replace("k_pass<", "k_pass_sw<").replace(">(pifft", ", 1>(pifft")
    assert inames[2] == "void pifft::k_pass_sw<double, 1024, 8, 2, 1, 0, 16, 2>(pifft::PassArgs)"


def test_cli_inverse(tmp_path):
    n, P, seed = 4096, 4, 7
    out = tmp_path / "inv.bin"
    r = subprocess.run([pifft.CLI_PATH, "-i", "-n", str(n), "-p", str(P), "-f", "64", "-s", str(seed), "-w", str(out)],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    cols = r.stdout.strip().splitlines()
    assert cols[0].split("\t") == ["n", "p", "time (total)", "time (stage 1)", "time (stage 2)"]
    assert cols[1].split("\t")[:2] == [str(n), str(P)] and len(cols[1].split("\t")) == 5
    got = np.fromfile(out, dtype=np.complex128)
    x = oracle.generate(n, np.complex128, seed=seed)
    want = np.fft.ifft(x) * n
    assert got.shape == want.shape and rel_l2(got, want) <= 1e-12
    # and the forward run of the same seed differs (the flag is not ignored)
    out_f = tmp_path / "fwd.bin"
    r = subprocess.run([pifft.CLI_PATH, "-n", str(n), "-p", str(P), "-f", "64", "-s", str(seed), "-w", str(out_f)],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert rel_l2(np.fromfile(out_f, dtype=np.complex128), np.fft.fft(x)) <= 1e-12
    usage = subprocess.run([pifft.CLI_PATH, "-n", "3", "-p", "1"], capture_output=True, text=True, timeout=60)
    assert "-i " in usage.stdout + usage.stderr
