"""Real-input plans (pifft_plan_create_real) on the CPU: dry runs of the
planner.  A real plan of n samples is the complex plan of n/2 points --
untouched, whatever the planner chooses for that shape -- plus one fix-up
launch ("r2c" after the forward chain, "c2r" before the inverse one) and a
staging buffer of batch * n/2 values.  And the fix-up kernels' own per-thread
code (csrc/pifft_real.h is __host__ __device__) run on the host over guarded
buffers against a direct O(n^2) real DFT."""
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


def shapes():
    for logn in (2, 3, 4, 11, 16, 17, 22, 29):
        h = 1 << (logn - 1)
        for P in sorted({p for p in (1, 2, 32, h) if p <= h}):
            for batch in (1, 3):
                for suf in ("f64", "f32"):
                    yield logn, P, batch, suf


@pytest.mark.parametrize("logn,P,batch,suf", list(shapes()),
                         ids=lambda v: str(v))
@pytest.mark.parametrize("inverse", [False, True], ids=["r2c", "c2r"])
def test_real_plan_is_the_inner_plan_plus_one_launch(logn, P, batch, suf, inverse):
    n, h = 1 << logn, 1 << (logn - 1)
    d = pifft.dry_run_real(n, P, batch, PREC[suf], inverse=inverse)
    i = pifft.dry_run(h, P, batch, PREC[suf], inverse=inverse)
    nl = i["num_launches"]
    assert d["num_launches"] == nl + 1
    if inverse:
        assert d["launch_kind"] == ["c2r"] + i["launch_kind"]
        assert d["launch_mode"] == [0] + i["launch_mode"]
        assert d["launch_bytes"][1:] == i["launch_bytes"]
        # same kernel-function structure: the inner ids, after the new launch's
        assert d["launch_fn"] == [0] + [f + 1 for f in i["launch_fn"]]
        new = 0
    else:
        assert d["launch_kind"] == i["launch_kind"] + ["r2c"]
        assert d["launch_mode"] == i["launch_mode"] + [0]
        assert d["launch_bytes"][:-1] == i["launch_bytes"]
        assert d["launch_fn"] == i["launch_fn"] + [max(i["launch_fn"]) + 1]
        new = nl
    for key in ("radix", "lines", "vpt", "num_passes", "tree_launches", "worker_interleaved", "natural_store"):
        assert d[key] == i[key], key
    assert d["n"] == n and d["local_n"] == h // P and d["workers"] == P and d["num_workers"] == P
    assert d["batch"] == batch and d["prec"] == PREC[suf]
    assert d["inverse"] == inverse and d["real"] == (2 if inverse else 1) and i["real"] == 0
    assert (d["in_elems"], d["out_elems"]) == ((batch * (h + 1), batch * h) if inverse else (batch * h, batch * (h + 1)))
    assert d["workspace_bytes"] >= i["workspace_bytes"] + batch * h * ESZ[suf]
    assert d["launch_bytes"][new] == batch * (2 * h + 1) * ESZ[suf]


def test_flags_field():
    for inverse in (False, True):
        info = pifft.PlanInfo()
        rc = pifft.lib().pifft_plan_dry_run_real(1 << 10, 4, 2, pifft.F32, int(inverse), ctypes.byref(info))
        assert rc == 0 and info.device == -1
        assert info.flags == (pifft.OUT_NATURAL | (pifft.INVERSE if inverse else 0))


@pytest.mark.parametrize("args,msg", [
    ((2, 1, 1, 64, 0), "Invalid input size"),
    ((12, 1, 1, 64, 0), "Invalid input size"),
    ((1 << 10, 3, 1, 64, 0), "Invalid number of procs"),
    ((1 << 10, 1 << 10, 1, 64, 0), "More processors than inputs!"),
    ((1 << 10, 1, 0, 64, 0), "batch must be >= 1"),
    ((1 << 10, 1, 1, 48, 0), "prec must be PIFFT_F32 or PIFFT_F64"),
    ((1 << 10, 1, 1, 64, 2), "direction must be PIFFT_REAL_FORWARD or PIFFT_REAL_INVERSE"),
])
def test_refusals(args, msg):
    info = pifft.PlanInfo()
    assert pifft.lib().pifft_plan_dry_run_real(*args, ctypes.byref(info)) == -1
    assert msg in pifft.last_error()
    h = ctypes.c_void_p()
    assert pifft.lib().pifft_plan_create_real(ctypes.byref(h), args[0], args[1], args[2], args[3], 0, args[4]) == -1
    assert msg in pifft.last_error() and not h.value


def test_largest_worker_count_is_half_the_samples():
    assert pifft.dry_run_real(1 << 10, 1 << 9)["local_n"] == 1
    assert pifft.dry_run_real(4, 2)["launch_kind"][-1] == "r2c"


def test_null_arguments():
    assert pifft.lib().pifft_plan_dry_run_real(16, 1, 1, 64, 0, None) == -1
    assert pifft.lib().pifft_plan_create_real(None, 16, 1, 1, 64, 0, 0) == -1
    assert pifft.lib().pifft_plan_is_real(None) == -1


def test_header_binding_and_abi():
    text = open(os.path.join(ROOT, "include", "pifft.h")).read()
    defs = dict(re.findall(r"#define (PIFFT_[A-Z_0-9]+) (\d+)", text))
    assert int(defs["PIFFT_REAL_FORWARD"]) == pifft.REAL_FORWARD == 0
    assert int(defs["PIFFT_REAL_INVERSE"]) == pifft.REAL_INVERSE == 1
    assert int(defs["PIFFT_ABI_VERSION"]) == pifft.ABI_VERSION == pifft.lib().pifft_abi_version() == 3
    # the layout of pifft_plan_info as it was before real plans existed
    assert ctypes.sizeof(pifft.PlanInfo) == 5312
    assert pifft.KIND_NAMES[5] == "r2c" and pifft.KIND_NAMES[6] == "c2r"
    for name in ("pifft_plan_create_real", "pifft_plan_dry_run_real", "pifft_plan_is_real"):
        assert name in pifft.SYMBOLS and name in pifft.header_symbols()
    # the real direction is no flag bit: the complex entry points still refuse 16, 32, 64
    for bit in (16, 32, 64):
        with pytest.raises(pifft.PifftError, match="unknown flags"):
            pifft.dry_run(1 << 10, 1, 1, pifft.F64, flags=bit)


def test_real_plan_class_does_not_run_the_complex_constructor():
    assert issubclass(pifft.RealPlan, pifft.Plan)
    assert "__init__" in vars(pifft.RealPlan)
    assert pifft.RealPlan.__init__.__code__.co_names.count("pifft_plan_create_real") == 1
    assert "super" not in pifft.RealPlan.__init__.__code__.co_names


# --- the fix-up kernels' per-thread code on the host ------------------------
@pytest.fixture(scope="module")
def fixup(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rf") / "real_fixup")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "-std=c++17", "-O1", "--offload-host-only", "-ffp-contract=off", "-Wall", "-o", out,
                    os.path.join(HERE, "native", "real_fixup_main.hip")], check=True)
    return out


# (log2 n, batch, threads of the emulated launch): n = 4, 8 have only bin 0 and
# the self-paired bin; 16 the first true pair; thread counts below, at and far
# above the work items, so threads loop, cross rows and idle
HOST_CASES = [(2, 1, 64), (2, 3, 1), (3, 3, 7), (4, 3, 256), (5, 3, 5), (6, 3, 64), (8, 5, 100), (10, 3, 256),
              (7, 3, 100000)]


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("direction", [0, 1], ids=["r2c_post", "c2r_pre"])
def test_fixup_code_on_the_host(fixup, suf, direction):
    """Error bound: the kernel's own arithmetic is a handful of roundings per
    bin (8 eps is generous for them); the fp-type input adds its own rounding."""
    eps = 2.0 ** -52 if suf == "f64" else 2.0 ** -23
    for logn, batch, threads in HOST_CASES:
        for mis in (0, 1):
            r = subprocess.run([fixup, str(logn), str(batch), suf[1:], str(direction), str(threads), str(mis)],
                               check=True, capture_output=True, text=True)
            got = json.loads(r.stdout)
            assert got["unwritten"] == 0 and got["guard"] == 0, (logn, batch, threads, mis, got)
            assert got["err"] <= 8 * eps, (logn, batch, threads, mis, got)
