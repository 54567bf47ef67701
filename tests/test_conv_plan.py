"""Convolution plans (pifft_plan_create_conv) on the CPU: dry runs of the planner.
A convolution plan of batch rows of n reals and one filter of taps reals is the
two chains of the real transforms of M reals -- the complex plan of (H = M/2, 1
worker, batch) forward and the same plan with PIFFT_INVERSE, both untouched,
whatever the planner chooses for their shape -- around the fused pair kernel,
between a pad and a crop launch (a cyclic plan: neither).  And the new kernels'
own per-thread code (csrc/pifft_conv.h is __host__ __device__) run on the host
over exactly sized heap buffers, under the address and undefined-behaviour
sanitizers where the toolchain links them."""
import ctypes
import json
import os
import re
import subprocess

import pytest

import pifft
from test_chirp_plan import align, chain_blob, first_use_ids

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PREC = {"f32": pifft.F32, "f64": pifft.F64}
ESZ = {"f32": 8, "f64": 16}
COR, CYC = pifft.CONV_CORRELATE, pifft.CONV_CYCLIC
SHAPES = ((1, 1), (2, 2), (5, 3), (3, 5), (1000, 25), (1000, 26), (1021, 17), (40000, 30000))
CYCLIC = ((4, 1), (4, 4), (16, 5), (1024, 1), (1024, 1024), (65536, 30000))


def info_of(n, taps, batch, prec, flags):
    info = pifft.PlanInfo()
    rc = pifft.lib().pifft_plan_dry_run_conv(n, taps, batch, prec, flags, ctypes.byref(info))
    assert rc == 0, pifft.last_error()
    return info


def pair_table(m, esz):
    """The two-level table of w_M: 2^h entries, then M >> h, h = ceil(log2 M / 2)."""
    h = (m.bit_length()) // 2
    return align((1 << h) * esz) + align(max(m >> h, 1) * esz)


def test_conv_length():
    for n in range(1, 70):
        for taps in range(1, 70):
            m = pifft.conv_length(n, taps)
            L = n + taps - 1
            assert m & (m - 1) == 0 and m >= max(L, 4) and (m == 4 or m // 2 < L)
    assert pifft.conv_length(1, 1) == pifft.conv_length(2, 2) == pifft.conv_length(2, 3) == 4
    assert pifft.conv_length(1000, 25) == 1024 and pifft.conv_length(1000, 26) == 2048
    assert pifft.conv_length(40000, 30000) == 1 << 17
    assert pifft.conv_length(1 << 27, (1 << 27) + 1) == 1 << 28


def check_plan(n, taps, batch, suf, correlate, cyclic):
    prec, esz = PREC[suf], ESZ[suf]
    L = n if cyclic else n + taps - 1
    m = n if cyclic else pifft.conv_length(n, taps)
    H = m // 2
    d = pifft.dry_run_conv(n, taps, batch, prec, correlate=correlate, cyclic=cyclic)
    f = pifft.dry_run(H, 1, batch, prec)
    i = pifft.dry_run(H, 1, batch, prec, inverse=True)
    f1 = pifft.dry_run(H, 1, 1, prec)
    nf, ni = f["num_launches"], i["num_launches"]
    pad, crop = ([] if cyclic else ["conv_pad"]), ([] if cyclic else ["conv_crop"])
    assert d["n"] == n and d["local_n"] == H
    assert d["launch_kind"] == pad + f["launch_kind"] + ["conv_pair"] + i["launch_kind"] + crop
    assert d["launch_mode"] == [0] * len(pad) + f["launch_mode"] + [0] + i["launch_mode"] + [0] * len(crop)
    rsz = esz // 2
    assert d["launch_bytes"] == ([batch * (n + m) * rsz] * len(pad) + f["launch_bytes"] +
                                 [(batch * 2 * H + H + 1) * esz] + i["launch_bytes"] +
                                 [batch * (m + L) * rsz] * len(crop))
    assert d["num_launches"] == nf + ni + 1 + len(pad) + len(crop)
    assert d["num_passes"] == f["num_passes"] + i["num_passes"] <= 8
    for key in ("radix", "lines", "vpt"):
        assert d[key] == f[key] + i[key], key
    # launch_fn: numbered in order of first use.  Within a chain equal kernels
    # exactly where the inner plan has them; the inverse chain's first and last
    # launches are swapping twins, kernels of their own, its launches between
    # are the forward chain's; the new kernels are shared with nothing
    assert nf == ni
    keys = (["pad"] * len(pad) + [("F", k) for k in f["launch_fn"]] + ["pair"] +
            [("F", f["launch_fn"][j]) if 0 < j < ni - 1 else ("I", k) for j, k in enumerate(i["launch_fn"])] +
            ["crop"] * len(crop))
    assert d["launch_fn"] == first_use_ids(keys)
    assert d["worker_interleaved"] == (f["worker_interleaved"] or i["worker_interleaved"])
    assert d["natural_store"] == (f["natural_store"] or i["natural_store"])
    assert d["batch"] == batch and d["prec"] == prec
    assert d["workers"] == 1 and d["num_workers"] == 1 and d["first_worker"] == 0 and d["tree_launches"] == 0
    # counted in reals
    assert d["in_elems"] == batch * n and d["out_elems"] == batch * L
    assert not d["inverse"] and d["real"] == 0 and not d["chirp"] and d["conv"] and not f["conv"]
    # workspace: Z (batch * H values; a cyclic plan's: one row) and Y (batch * H),
    # G (H + 1 values), one W -- the largest of the three chains', each its dry
    # run's workspace less its table blob -- the three chains' table blobs and
    # the two-level table of w_M.  Held exactly.
    blobs = [chain_blob(c, H, esz) for c in (f, i, f1)]
    w = max(c["workspace_bytes"] - b for c, b in zip((f, i, f1), blobs))
    assert w >= 0
    assert d["workspace_bytes"] == ((1 if cyclic else batch) * H * esz + batch * H * esz + (H + 1) * esz + w +
                                    sum(blobs) + pair_table(m, esz))
    info = info_of(n, taps, batch, prec, (COR if correlate else 0) | (CYC if cyclic else 0))
    assert info.flags == (COR if correlate else 0) | (CYC if cyclic else 0) and info.device == -1
    return d


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("n,taps", SHAPES)
def test_linear_plan_is_the_two_inner_plans_and_three_launches(n, taps, suf):
    for batch in (1, 3):
        a = check_plan(n, taps, batch, suf, False, False)
        b = check_plan(n, taps, batch, suf, True, False)
        assert a == b  # the correlate flag acts in pifft_conv_set_filter only
    # a correlation plan's info: the convolution plan's in every field but flags
    x, y = info_of(n, taps, 3, PREC[suf], 0), info_of(n, taps, 3, PREC[suf], COR)
    for name, _ in pifft.PlanInfo._fields_:
        if name != "flags":
            u, v = getattr(x, name), getattr(y, name)
            assert (list(u) == list(v)) if hasattr(u, "__len__") else (u == v), name


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("n,taps", CYCLIC)
def test_cyclic_plan_is_the_two_inner_plans_and_the_pair_launch(n, taps, suf):
    for batch in (1, 3):
        for correlate in (False, True):
            d = check_plan(n, taps, batch, suf, correlate, True)
            assert "conv_pad" not in d["launch_kind"] and "conv_crop" not in d["launch_kind"]


def test_lengths_at_the_power_of_two():
    """(1000, 25): L = M = 1024; (1000, 26): L = 1025, M = 2048."""
    for suf in ("f64", "f32"):
        a, b = pifft.dry_run_conv(1000, 25, 1, PREC[suf]), pifft.dry_run_conv(1000, 26, 1, PREC[suf])
        assert a["out_elems"] == 1024 and a["local_n"] == 512
        assert b["out_elems"] == 1025 and b["local_n"] == 1024
        # (40000, 30000): M = 2^17, chains of more than one pass
        c = pifft.dry_run_conv(40000, 30000, 1, PREC[suf])
        assert c["local_n"] == 1 << 16 and c["num_passes"] == 4


BIG = 1 << 28
REFUSALS = [
    ((0, 1, 1, 64, 0), "a convolution plan needs n >= 1 and taps >= 1"),
    ((1, 0, 1, 64, 0), "a convolution plan needs n >= 1 and taps >= 1"),
    ((0, 0, 1, 32, CYC), "a convolution plan needs n >= 1 and taps >= 1"),
    ((1000, 25, 0, 64, 0), "batch must be >= 1"),
    ((1000, 25, 1, 48, 0), "prec must be PIFFT_F32 or PIFFT_F64"),
    ((1000, 25, 1, 64, 8), "unknown flags 8"),
    ((1000, 25, 1, 64, 8 | COR), "unknown flags 40"),
    ((1000, 25, 1, 64, 16), "unknown flags 16"),
    ((1000, 25, 1, 64, 1), "unknown flags 1"),
    ((1000, 25, 1, 64, 4), "unknown flags 4"),
    ((1000, 25, 1, 64, 128), "unknown flags 128"),
    ((1000, 25, 1, 64, -1), "unknown flags -1"),
    ((BIG, 2, 1, 64, 0), "n + taps - 1 must not exceed 2^28"),
    ((2, BIG, 1, 32, 0), "n + taps - 1 must not exceed 2^28"),
    ((BIG + 1, 1, 1, 64, 0), "n + taps - 1 must not exceed 2^28"),
    ((1 << 63, 1 << 63, 1, 64, 0), "n + taps - 1 must not exceed 2^28"),
    (((1 << 64) - 1, 2, 1, 64, 0), "n + taps - 1 must not exceed 2^28"),
    ((1000, 25, 1, 64, CYC), "a cyclic convolution plan needs n = 2^i, i > 1"),
    ((2, 1, 1, 64, CYC), "a cyclic convolution plan needs n = 2^i, i > 1"),
    ((1, 1, 1, 64, CYC | COR), "a cyclic convolution plan needs n = 2^i, i > 1"),
    ((1 << 29, 1, 1, 64, CYC), "a cyclic plan needs n <= 2^28"),
    ((1024, 1025, 1, 64, CYC), "a cyclic convolution plan needs taps <= n"),
    ((4, 5, 1, 32, CYC | COR), "a cyclic convolution plan needs taps <= n"),
]


@pytest.mark.parametrize("args,msg", REFUSALS)
def test_refusals(args, msg):
    info = pifft.PlanInfo()
    assert pifft.lib().pifft_plan_dry_run_conv(*args, ctypes.byref(info)) == -1
    assert msg in pifft.last_error()
    h = ctypes.c_void_p()
    n, taps, batch, prec, flags = args
    assert pifft.lib().pifft_plan_create_conv(ctypes.byref(h), n, taps, batch, prec, 0, flags) == -1
    assert msg in pifft.last_error() and not h.value


def test_accepted_flags_and_limits():
    for flags in (0, COR, CYC, COR | CYC):
        assert info_of(1024, 25, 2, pifft.F32, flags).flags == flags
    assert info_of(BIG - 1, 2, 1, pifft.F32, 0).local_n == 1 << 27
    assert info_of(BIG, 1, 1, pifft.F32, 0).out_elems == BIG
    assert info_of(BIG, BIG, 1, pifft.F32, CYC).local_n == 1 << 27


def test_null_arguments():
    L = pifft.lib()
    assert L.pifft_plan_dry_run_conv(1000, 25, 1, 64, 0, None) == -1 and "info is NULL" in pifft.last_error()
    assert L.pifft_plan_create_conv(None, 1000, 25, 1, 64, 0, 0) == -1 and "plan pointer is NULL" in pifft.last_error()
    assert L.pifft_plan_is_conv(None) == -1
    assert L.pifft_conv_set_filter(None, None, None) == -1 and "plan is NULL" in pifft.last_error()
    v = ctypes.c_uint64()
    assert L.pifft_plan_conv_shape(None, ctypes.byref(v), ctypes.byref(v), ctypes.byref(v), ctypes.byref(v)) == -1
    assert "NULL argument" in pifft.last_error()


@pytest.mark.parametrize("call", [
    lambda: pifft.ConvPlan(-3, 1),
    lambda: pifft.ConvPlan(1 << 64, 1),
    lambda: pifft.ConvPlan(1000, -1),
    lambda: pifft.ConvPlan(1000, 1 << 64),
    lambda: pifft.ConvPlan(1000, 25, batch=1 << 32),
    lambda: pifft.ConvPlan(1000, 25, batch=-1),
    lambda: pifft.ConvPlan(1000.0, 25),
    lambda: pifft.ConvPlan(1000, 25, prec=16),
    lambda: pifft.dry_run_conv(-1000, 25),
    lambda: pifft.dry_run_conv(1000, 25, 1 << 32),
    lambda: pifft.dry_run_conv(1000, 25, 1, 48),
    lambda: pifft.dry_run_conv(1000, 25, cyclic=True),
])
def test_binding_argument_checks(call):
    """What ctypes would wrap into the C types (a batch of 2^32 becomes 0) is
    refused by the binding before the call."""
    with pytest.raises(pifft.PifftError):
        call()


def test_the_other_entry_points_refuse_the_new_flags():
    """Unchanged: flags 32 and 64 are unknown to the 1-D, real, matrix and chirp entry points."""
    L = pifft.lib()
    h = ctypes.c_void_p()
    info = pifft.PlanInfo()
    for flags in (COR, CYC, COR | CYC, COR | 8, CYC | 1):
        assert L.pifft_plan_dry_run(1024, 1, 0, 1, 1, 64, flags, ctypes.byref(info)) == -1
        assert f"unknown flags {flags}" in pifft.last_error()
        assert L.pifft_plan_create_slices(ctypes.byref(h), 1024, 1, 0, 1, 1, 64, 0, flags) == -1
        assert f"unknown flags {flags}" in pifft.last_error() and not h.value
        assert L.pifft_plan_dry_run_real(1024, 1, 1, 64, flags, ctypes.byref(info)) == -1
        assert "direction must be" in pifft.last_error()
        assert L.pifft_plan_create_real(ctypes.byref(h), 1024, 1, 1, 64, 0, flags) == -1
        assert "direction must be" in pifft.last_error() and not h.value
        assert L.pifft_plan_dry_run_matrix(32, 32, 1, 64, flags, ctypes.byref(info)) == -1
        assert f"unknown flags {flags}" in pifft.last_error()
        assert L.pifft_plan_create_matrix(ctypes.byref(h), 32, 32, 1, 64, 0, flags) == -1
        assert f"unknown flags {flags}" in pifft.last_error() and not h.value
        assert L.pifft_plan_dry_run_chirp(1000, 1, 64, flags, ctypes.byref(info)) == -1
        assert f"unknown flags {flags}" in pifft.last_error()
        assert L.pifft_plan_create_chirp(ctypes.byref(h), 1000, 1, 64, 0, flags) == -1
        assert f"unknown flags {flags}" in pifft.last_error() and not h.value


NEW_SYMBOLS = ("pifft_plan_create_conv", "pifft_plan_dry_run_conv", "pifft_conv_set_filter", "pifft_plan_is_conv",
               "pifft_plan_conv_shape")


def test_header_binding_and_abi():
    text = open(os.path.join(ROOT, "include", "pifft.h")).read()
    defs = dict(re.findall(r"#define (PIFFT_[A-Z_0-9]+) (\d+)", text))
    assert int(defs["PIFFT_ABI_VERSION"]) == pifft.ABI_VERSION == pifft.lib().pifft_abi_version() == 3
    assert ctypes.sizeof(pifft.PlanInfo) == 5312
    assert int(defs["PIFFT_CONV_CORRELATE"]) == COR == 32 and int(defs["PIFFT_CONV_CYCLIC"]) == CYC == 64
    assert (pifft.KIND_NAMES[11], pifft.KIND_NAMES[12], pifft.KIND_NAMES[13]) == ("conv_pad", "conv_pair", "conv_crop")
    for name in NEW_SYMBOLS:
        assert name in pifft.SYMBOLS and name in pifft.header_symbols()
        assert hasattr(pifft.lib(), name)
    assert sorted(pifft.SYMBOLS) == pifft.header_symbols()
    assert len(pifft.aux_kernels()) == 62  # the registry of the 1-D and real plans' kernels: as it was
    # the new kernels live in the new header, which pifft.hip alone includes
    csrc = os.path.join(ROOT, "cs87project-msolano2_amd", "csrc")
    conv = open(os.path.join(csrc, "pifft_conv.h")).read()
    assert conv.count("__global__") == 4 and "asm" not in conv and "k_pass" not in conv.replace("k_pass translation", "")
    users = [f for f in sorted(os.listdir(csrc)) if f != "pifft_conv.h" and os.path.isfile(os.path.join(csrc, f)) and
             '#include "pifft_conv.h"' in open(os.path.join(csrc, f)).read()]
    assert users == ["pifft.hip"]
    mk = open(os.path.join(ROOT, "cs87project-msolano2_amd", "Makefile")).read()
    assert re.search(r"^build/pifft_abi\.o:.*csrc/pifft_conv\.h", mk, re.M)


def test_no_new_pass_instance():
    """The library's k_pass registry is the committed instance lists, one row each: the plans add none."""
    csrc = os.path.join(ROOT, "cs87project-msolano2_amd", "csrc")
    rows = sum(len(re.findall(r"^\s*PKV?\(", open(os.path.join(csrc, f)).read(), re.M))
               for f in os.listdir(csrc) if re.fullmatch(r"pifft_instances_\d\.inc", f))
    assert rows == pifft.lib().pifft_instance_count() > 0


def test_conv_plan_class_does_not_run_the_complex_constructor():
    assert issubclass(pifft.ConvPlan, pifft.Plan)
    assert "__init__" in vars(pifft.ConvPlan)
    assert pifft.ConvPlan.__init__.__code__.co_names.count("pifft_plan_create_conv") == 1
    assert "super" not in pifft.ConvPlan.__init__.__code__.co_names
    assert "pifft_plan_create" not in pifft.ConvPlan.__init__.__code__.co_names


# --- the kernels' per-thread code on the host --------------------------------
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")


@pytest.fixture(scope="module")
def conv(tmp_path_factory):
    """The program, built with the sanitizers where the toolchain links them."""
    out = str(tmp_path_factory.mktemp("cv") / "conv")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-std=c++17", "-O1", "--offload-host-only", "-ffp-contract=off", "-Wall", "-o", out,
           os.path.join(HERE, "native", "conv_main.hip")]
    if subprocess.run(cmd + SANITIZE, capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)
    return out


def native(prog, *args):
    r = subprocess.run([prog] + [str(a) for a in args], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0, (args, r.stderr[-2000:])
    return json.loads(r.stdout)


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("n,taps", [(1, 1), (2, 2), (5, 3), (3, 5), (4, 1), (6, 3), (30, 4), (100, 29), (1000, 25),
                                    (1021, 17)])
def test_pad_crop_and_filter_code_on_the_host(conv, n, taps, suf):
    """Pad, crop and filter (forward and back to front), every thread of the
    launch in turn over heap rows of exactly batch * n, batch * L, taps and
    batch * M reals: every value stored once with the bits a plain loop gives,
    the pad zeros included.  Odd and even n and L, batch 1 and 3 (an odd n or L
    puts the rows at every residue), the caller's buffers shifted by 0 to 3
    reals on top, the library's thread count and 1, 3 and 7 threads in all
    (second and later trips of every thread).  A sanitizer report aborts the
    program."""
    for batch in (1, 3):
        for threads in (0, 1, 3, 7):
            for mis in range(4 if suf == "f32" else 2):
                got = native(conv, "stream", n, taps, batch, suf[1:], threads, mis)
                assert got == {"bad": 0, "unwritten": 0, "guard": 0}, (n, taps, batch, threads, mis, got)


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("H", [2, 4, 8, 16, 64, 1024])
def test_pair_code_equals_the_three_launches_bit_for_bit(conv, H, suf):
    """conv_pair_unit in place against real_unit<0>, a plain complex product and
    real_unit<1> over buffers of their own (Y of batch * H, G of H + 1, X of
    batch * (H + 1) values exactly).  H = 2: bins 0 and the self-paired 1 only;
    4 to 16: the fp32 two-pair items' edges (the first item, the last, the one
    holding H/2); 64 and 1024: the two-pair run between them.  Thread counts of
    1, 3 and 7 in all and the library's."""
    for batch in (1, 3):
        for threads in (0, 1, 3, 7):
            got = native(conv, "pair", H, batch, suf[1:], threads)
            assert got == {"bad": 0, "unwritten": 0}, (H, batch, threads, got)


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("correlate", [0, 1], ids=["convolve", "correlate"])
@pytest.mark.parametrize("n,taps,m", [(1, 1, 4), (2, 2, 4), (3, 2, 4), (5, 3, 8), (3, 5, 8), (8, 1, 8), (9, 8, 16),
                                      (1, 16, 16)])
def test_whole_formula_on_the_host(conv, n, taps, m, correlate, suf):
    """Filter, a naive O(H^2) DFT and the R2C fix-up for G; pad, a naive DFT,
    pair, a naive inverse and crop -- against the directly summed convolution
    in long double.  The naive transforms are exact up to their one rounding to
    T, so the error is the kernels' own: the rounded G, the three steps of the
    pair with their rounded w, and the roundings of the transforms' results --
    none amplified -- well under 8 eps in rel-L2 (eps = 2^-52 / 2^-23)."""
    got = native(conv, "formula", n, taps, suf[1:], correlate)
    print(f"formula n = {n} taps = {taps} {suf} correlate = {correlate}: rel-L2 = {got['err']:.3f} eps")
    assert got["m"] == m == pifft.conv_length(n, taps)
    assert got["err"] <= 8
