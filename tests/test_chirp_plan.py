"""Chirp plans (pifft_plan_create_chirp) on the CPU: dry runs of the planner.
A chirp plan of batch rows of n values, n no power of two, is Bluestein's
chirp-z algorithm: the complex plan of (M, 1 worker, batch), M the smallest
power of two >= 2n - 1, forward, a pointwise product, the same plan with
PIFFT_INVERSE -- both inner plans untouched, whatever the planner chooses for
their shape -- between a chirp-pre and a chirp-post launch.  And the new
kernels' own per-thread code (csrc/pifft_chirp.h is __host__ __device__) run on
the host over exactly sized heap buffers, under the address and
undefined-behaviour sanitizers where the toolchain links them."""
import ctypes
import json
import os
import re
import subprocess

import pytest

import pifft

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PREC = {"f32": pifft.F32, "f64": pifft.F64}
ESZ = {"f32": 8, "f64": 16}
INV = pifft.INVERSE
NS = (3, 5, 7, 12, 1000, 1021, 8191, 8193, 40000, 786433, 10 ** 8, 2 ** 27 - 1)


def info_of(n, batch, prec, flags):
    info = pifft.PlanInfo()
    rc = pifft.lib().pifft_plan_dry_run_chirp(n, batch, prec, flags, ctypes.byref(info))
    assert rc == 0, pifft.last_error()
    return info


def first_use_ids(keys):
    """ids 0, 1, ... in order of first use: what launch_fn must be for launches named by `keys`."""
    seen = {}
    return [seen.setdefault(k, len(seen)) for k in keys]


def align(b):
    return (b + 255) & ~255


def chain_blob(d, m, esz):
    """The table blob of a one-worker chain of m values from its dry run d: w_R
    per distinct radix and, with more than one pass, the two-level w_M -- each
    table 256-B aligned (TableBuilder)."""
    off = 0
    for r in dict.fromkeys(d["radix"]):
        off = align(off) + r * esz
    if d["num_passes"] > 1:
        logm = m.bit_length() - 1
        h = (logm + 1) // 2
        off = align(off) + (1 << h) * esz
        off = align(off) + (m >> h) * esz
    return align(off)


def chirp_table(n, esz):
    """The two-level table of w_2n: 2^h entries, then ceil(2n / 2^h), h = ceil(ceil(log2 2n) / 2)."""
    h = ((2 * n - 1).bit_length() + 1) // 2
    return align((1 << h) * esz) + align(((2 * n + (1 << h) - 1) >> h) * esz)


def test_chirp_length():
    for n in range(3, 600):
        m = pifft.chirp_length(n)
        assert m & (m - 1) == 0 and m >= 2 * n - 1 > m // 2
    assert pifft.chirp_length(3) == 8
    for k in range(2, 27):
        assert pifft.chirp_length(2 ** k + 1) == 2 ** (k + 2) and pifft.chirp_length(2 ** k - 1) == 2 ** (k + 1)
    assert pifft.chirp_length(2 ** 27 - 1) == 2 ** 28 == pifft.chirp_length(10 ** 8)


def test_chain_blob_is_the_inner_plans_table_blob():
    """chain_blob above against the dry runs, where W is known: one launch has
    no W, and below 2 GiB W is batch * m values, unpadded."""
    for suf in ("f64", "f32"):
        for logm in range(3, 27):
            m = 1 << logm
            d = pifft.dry_run(m, 1, 1, PREC[suf])
            w = m * ESZ[suf] if d["num_launches"] > 1 else 0
            assert d["workspace_bytes"] == w + chain_blob(d, m, ESZ[suf]), (suf, logm)


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("n", NS)
def test_chirp_plan_is_the_two_inner_plans_and_three_launches(n, suf):
    prec, esz = PREC[suf], ESZ[suf]
    m = pifft.chirp_length(n)
    for batch in (1, 3):
        for inverse in (False, True):
            d = pifft.dry_run_chirp(n, batch, prec, inverse=inverse)
            f = pifft.dry_run(m, 1, batch, prec)
            i = pifft.dry_run(m, 1, batch, prec, inverse=True)
            nf, ni = f["num_launches"], i["num_launches"]
            assert d["local_n"] == m and d["n"] == n
            assert d["launch_kind"] == ["chirp_pre"] + f["launch_kind"] + ["spectrum_mul"] + i["launch_kind"] + ["chirp_post"]
            assert d["launch_mode"] == [0] + f["launch_mode"] + [0] + i["launch_mode"] + [0]
            assert d["launch_bytes"] == ([batch * (n + m) * esz] + f["launch_bytes"] + [(batch * 2 * m + m) * esz] +
                                         i["launch_bytes"] + [batch * 2 * n * esz])
            assert d["num_launches"] == nf + ni + 3
            assert d["num_passes"] == f["num_passes"] + i["num_passes"] <= 8
            for key in ("radix", "lines", "vpt"):
                assert d[key] == f[key] + i[key], key
            # launch_fn: numbered in order of first use.  Within a chain equal
            # kernels exactly where the inner plan has them; the inverse chain's
            # first and last launches are swapping twins, kernels of their own,
            # its launches between are the forward chain's; the three new
            # kernels are shared with nothing
            assert nf == ni
            keys = (["pre"] + [("F", k) for k in f["launch_fn"]] + ["mul"] +
                    [("F", f["launch_fn"][j]) if 0 < j < ni - 1 else ("I", k) for j, k in enumerate(i["launch_fn"])] +
                    ["post"])
            assert d["launch_fn"] == first_use_ids(keys)
            fn = d["launch_fn"]
            assert first_use_ids(fn[1:1 + nf]) == f["launch_fn"] and first_use_ids(fn[2 + nf:2 + nf + ni]) == i["launch_fn"]
            for at in (0, 1 + nf, 2 + nf + ni):
                assert fn.count(fn[at]) == 1
            assert d["worker_interleaved"] == (f["worker_interleaved"] or i["worker_interleaved"])
            assert d["natural_store"] == (f["natural_store"] or i["natural_store"])
            assert d["batch"] == batch and d["prec"] == prec
            assert d["workers"] == 1 and d["num_workers"] == 1 and d["first_worker"] == 0 and d["tree_launches"] == 0
            assert d["in_elems"] == d["out_elems"] == batch * n
            assert d["inverse"] == inverse and d["real"] == 0 and d["chirp"] and not f["chirp"]
            # workspace: Z and Y (batch * M values each), one W -- the larger of
            # the two chains', each its dry run's workspace less its table blob
            # -- both chains' table blobs, the two-level table of w_2n, and Bt
            # (M values).  Held exactly.
            assert f["radix"] == i["radix"]
            blob = chain_blob(f, m, esz)
            w = max(f["workspace_bytes"], i["workspace_bytes"]) - blob
            assert w >= 0 and (w > 0) == (nf > 1)
            assert d["workspace_bytes"] == 2 * batch * m * esz + w + 2 * blob + chirp_table(n, esz) + m * esz
        # an inverse plan's info: the forward plan's in every field but flags and launch_fn
        a, b = info_of(n, batch, prec, 0), info_of(n, batch, prec, INV)
        assert a.flags == 0 and b.flags == INV and a.device == b.device == -1
        for name, _ in pifft.PlanInfo._fields_:
            if name in ("flags", "launch_fn"):
                continue
            x, y = getattr(a, name), getattr(b, name)
            assert (list(x) == list(y)) if hasattr(x, "__len__") else (x == y), name


def test_pass_counts():
    """8191 is the largest n of one-pass chains (M = 2^14), 8193 the smallest of
    two-pass ones (M = 2^15); 786433 has three-pass chains (M = 2^21)."""
    for suf in ("f64", "f32"):
        assert pifft.dry_run_chirp(8191, 1, PREC[suf])["num_passes"] == 2
        assert pifft.dry_run_chirp(8193, 1, PREC[suf])["num_passes"] == 4
        assert pifft.dry_run_chirp(786433, 1, PREC[suf])["num_passes"] == 6


@pytest.mark.parametrize("args,msg", [
    ((2, 1, 64, 0), "use pifft_plan_create"),
    ((4, 1, 64, 0), "use pifft_plan_create"),
    ((1024, 1, 32, 0), "use pifft_plan_create"),
    ((1 << 27, 1, 64, 0), "use pifft_plan_create"),
    ((1 << 40, 1, 64, 0), "use pifft_plan_create"),
    ((0, 1, 64, 0), "a chirp plan needs 3 <= n <= 2^27"),
    ((1, 1, 64, 0), "a chirp plan needs 3 <= n <= 2^27"),
    (((1 << 27) + 1, 1, 64, 0), "a chirp plan needs 3 <= n <= 2^27"),
    ((3 << 40, 1, 64, 0), "a chirp plan needs 3 <= n <= 2^27"),
    ((1000, 0, 64, 0), "batch must be >= 1"),
    ((1000, 1, 48, 0), "prec must be PIFFT_F32 or PIFFT_F64"),
    ((1000, 1, 64, 1), "unknown flags 1"),
    ((1000, 1, 64, 4), "unknown flags 4"),
    ((1000, 1, 64, 12), "unknown flags 12"),
    ((1000, 1, 64, 16), "unknown flags 16"),
    ((1000, 1, 64, 24), "unknown flags 24"),
    ((1000, 1, 64, -1), "unknown flags -1"),
])
def test_refusals(args, msg):
    info = pifft.PlanInfo()
    assert pifft.lib().pifft_plan_dry_run_chirp(*args, ctypes.byref(info)) == -1
    assert msg in pifft.last_error()
    h = ctypes.c_void_p()
    n, batch, prec, flags = args
    assert pifft.lib().pifft_plan_create_chirp(ctypes.byref(h), n, batch, prec, 0, flags) == -1
    assert msg in pifft.last_error() and not h.value


def test_accepted_flags():
    for flags in (0, 8):
        assert info_of(1000, 2, pifft.F32, flags).flags == flags


def test_null_arguments():
    L = pifft.lib()
    assert L.pifft_plan_dry_run_chirp(1000, 1, 64, 0, None) == -1 and "info is NULL" in pifft.last_error()
    assert L.pifft_plan_create_chirp(None, 1000, 1, 64, 0, 0) == -1 and "plan pointer is NULL" in pifft.last_error()
    assert L.pifft_plan_is_chirp(None) == -1


@pytest.mark.parametrize("call", [
    lambda: pifft.ChirpPlan(-3),
    lambda: pifft.ChirpPlan(1 << 64),
    lambda: pifft.ChirpPlan(1000, batch=1 << 32),
    lambda: pifft.ChirpPlan(1000, batch=-1),
    lambda: pifft.ChirpPlan(1000.0),
    lambda: pifft.ChirpPlan(1000, prec=16),
    lambda: pifft.dry_run_chirp(-1000),
    lambda: pifft.dry_run_chirp(1000, 1 << 32),
    lambda: pifft.dry_run_chirp(1000, 1, 48),
    lambda: pifft.dry_run_chirp(1024),
])
def test_binding_argument_checks(call):
    """What ctypes would wrap into the C types (a batch of 2^32 becomes 0) is
    refused by the binding before the call."""
    with pytest.raises(pifft.PifftError):
        call()


def test_the_other_entry_points_refuse_a_length_that_is_no_power_of_two():
    """Unchanged: the 1-D, real and matrix entry points take 2^i only."""
    L = pifft.lib()
    h = ctypes.c_void_p()
    for n in (3, 12, 1000, 10007):
        with pytest.raises(pifft.PifftError, match=r"Invalid input size \(should be 2\^i for i>0\)"):
            pifft.dry_run(n, 1, 1, pifft.F64)
        with pytest.raises(pifft.PifftError, match=r"Invalid input size \(should be 2\^i for i>0\)"):
            pifft.dry_run(n, 1, 1, pifft.F32, inverse=True)
        assert L.pifft_plan_create(ctypes.byref(h), n, 1, 1, 64) == -1
        assert "Invalid input size (should be 2^i for i>0)" in pifft.last_error() and not h.value
        assert L.pifft_plan_create_slices(ctypes.byref(h), n, 1, 0, 1, 1, 64, 0, 0) == -1
        assert "Invalid input size (should be 2^i for i>0)" in pifft.last_error() and not h.value
        with pytest.raises(pifft.PifftError, match=r"Invalid input size \(a real plan needs 2\^i reals, i > 1\)"):
            pifft.dry_run_real(n, 1, 1, pifft.F64)
        assert L.pifft_plan_create_real(ctypes.byref(h), n, 1, 1, 64, 0, 0) == -1
        assert "Invalid input size (a real plan needs 2^i reals, i > 1)" in pifft.last_error() and not h.value
        for n0, n1 in ((n, 64), (64, n)):
            with pytest.raises(pifft.PifftError, match="Invalid matrix size"):
                pifft.dry_run_matrix(n0, n1)
            assert L.pifft_plan_create_matrix(ctypes.byref(h), n0, n1, 1, 64, 0, 0) == -1
            assert "Invalid matrix size" in pifft.last_error() and not h.value


def test_header_binding_and_abi():
    text = open(os.path.join(ROOT, "include", "pifft.h")).read()
    defs = dict(re.findall(r"#define (PIFFT_[A-Z_0-9]+) (\d+)", text))
    assert int(defs["PIFFT_ABI_VERSION"]) == pifft.ABI_VERSION == pifft.lib().pifft_abi_version() == 3
    assert ctypes.sizeof(pifft.PlanInfo) == 5312
    assert (pifft.KIND_NAMES[8], pifft.KIND_NAMES[9], pifft.KIND_NAMES[10]) == ("chirp_pre", "spectrum_mul", "chirp_post")
    for name in ("pifft_plan_create_chirp", "pifft_plan_dry_run_chirp", "pifft_plan_is_chirp"):
        assert name in pifft.SYMBOLS and name in pifft.header_symbols()
        assert hasattr(pifft.lib(), name)
    assert len(pifft.aux_kernels()) == 62
    # the new kernels live in the new header, which pifft.hip alone includes
    csrc = os.path.join(ROOT, "cs87project-msolano2_amd", "csrc")
    chirp = open(os.path.join(csrc, "pifft_chirp.h")).read()
    assert chirp.count("__global__") == 5 and "asm" not in chirp
    users = [f for f in sorted(os.listdir(csrc)) if f != "pifft_chirp.h" and os.path.isfile(os.path.join(csrc, f)) and
             '#include "pifft_chirp.h"' in open(os.path.join(csrc, f)).read()]
    assert users == ["pifft.hip"]
    mk = open(os.path.join(ROOT, "cs87project-msolano2_amd", "Makefile")).read()
    assert re.search(r"^build/pifft_abi\.o:.*csrc/pifft_chirp\.h", mk, re.M)


def test_chirp_plan_class_does_not_run_the_complex_constructor():
    assert issubclass(pifft.ChirpPlan, pifft.Plan)
    assert "__init__" in vars(pifft.ChirpPlan)
    assert pifft.ChirpPlan.__init__.__code__.co_names.count("pifft_plan_create_chirp") == 1
    assert "super" not in pifft.ChirpPlan.__init__.__code__.co_names


# --- the kernels' per-thread code on the host --------------------------------
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")


@pytest.fixture(scope="module")
def chirp(tmp_path_factory):
    """The program, built with the sanitizers where the toolchain links them."""
    out = str(tmp_path_factory.mktemp("cz") / "chirp")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-std=c++17", "-O1", "--offload-host-only", "-ffp-contract=off", "-Wall", "-o", out,
           os.path.join(HERE, "native", "chirp_main.hip")]
    if subprocess.run(cmd + SANITIZE, capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)
    return out


def native(prog, *args):
    r = subprocess.run([prog] + [str(a) for a in args], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0, (args, r.stderr[-2000:])
    return json.loads(r.stdout)


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("n", [3, 7, 12, 17, 100, 1021])
def test_kernel_code_on_the_host(chirp, n, suf):
    """Pre (SW 0, 1), mul and post (SW 0, 2), every thread of the launch in turn
    over heap rows of exactly batch * n and batch * M values: every value stored
    once with the bits of the same arithmetic done value by value (r in
    unsigned __int128), the pad zeros included; odd and even n, batch 1 and 3
    (an odd n puts fp32 row 1 at 8 mod 16), the library's grid and grids capped
    at 1 and 3 workgroups (second trips), and the caller's buffers shifted by
    one value.  A sanitizer report aborts the program."""
    for batch in (1, 3):
        for cap in (0, 1, 3):
            for mis in (0, 1):
                got = native(chirp, "kernels", n, batch, suf[1:], cap, mis)
                assert got == {"bad": 0, "unwritten": 0, "guard": 0}, (n, batch, cap, mis, got)


@pytest.mark.parametrize("n,samples", [(3, 0), (5, 0), (7, 0), (12, 0), (1000, 0), (1021, 0), (8193, 0), (40000, 0),
                                       (786433, 0), (10 ** 8, 1 << 20), (2 ** 27 - 1, 1 << 20)])
def test_square_mod_2n_is_exact(chirp, n, samples):
    """r = j^2 mod 2n (chirp_sq_mod) and the adjacent value's (chirp_sq_next)
    against unsigned __int128: every j, or 2^20 sampled j and the ends."""
    assert native(chirp, "sqmod", n, samples) == {"bad": 0}


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("n", [3, 5, 7, 12, 1000, 1021, 40000, 2 ** 27 - 1])
def test_two_level_chirp_twiddle(chirp, n, suf):
    """hi[r >> h] lo[r & mask] against long double e^{-i pi r/n}: two rounded
    table entries and a product, held to the 8 eps the real fix-ups' host test
    holds the same construction to (eps = 2^-52 / 2^-23)."""
    got = native(chirp, "tw", n, suf[1:])
    print(f"two-level w_2n, n = {n} {suf}: worst |w - exact| = {got['err']:.3f} eps")
    assert got["err"] <= 8


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("swapped", [0, 1], ids=["forward", "swapped"])
@pytest.mark.parametrize("n", [3, 5, 7, 12])
def test_whole_formula_on_the_host(chirp, n, swapped, suf):
    """Pre, a naive O(M^2) DFT, mul, a naive inverse and post -- Bt from the
    fill code, a naive DFT rounded to fp64 and the scale-and-round code --
    against the direct DFT (swapped: the unnormalised inverse).  The naive
    transforms are exact up to their one rounding to T, so the error is the
    kernels' own: a rounded w and a product in pre and in post, the rounded Bt
    and its product, and the two roundings of the transforms' results -- none
    amplified (the convolution's result has the norm of its inputs' product) --
    well under 8 eps in rel-L2."""
    got = native(chirp, "formula", n, suf[1:], swapped)
    print(f"formula n = {n} {suf} swapped = {swapped}: rel-L2 = {got['err']:.3f} eps")
    assert got["err"] <= 8
