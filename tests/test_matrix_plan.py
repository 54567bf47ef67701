"""Matrix plans (pifft_plan_create_matrix) on the CPU: dry runs of the
planner.  A matrix plan of batch arrays of n0 x n1 values is the complex plan
of (n1, 1 worker, batch n0) for the rows, a transpose, the complex plan of
(n0, 1 worker, batch n1) for the columns and, unless the output stays
transposed, a second transpose -- both inner plans untouched, whatever the
planner chooses for their shapes.  And the transpose kernel's own index maps
(csrc/pifft_matrix.h is __host__ __device__) run on the host, phase by phase
over guarded buffers, under the address and undefined-behaviour sanitizers
where the toolchain links them."""
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
INV, TOUT = pifft.INVERSE, pifft.MATRIX_TRANSPOSED_OUT
DIMS = (2, 4, 64, 1 << 11, 1 << 15)


def info_of(n0, n1, batch, prec, flags):
    info = pifft.PlanInfo()
    rc = pifft.lib().pifft_plan_dry_run_matrix(n0, n1, batch, prec, flags, ctypes.byref(info))
    assert rc == 0, pifft.last_error()
    return info


def first_use_ids(keys):
    """ids 0, 1, ... in order of first use: what launch_fn must be for launches named by `keys`."""
    seen = {}
    return [seen.setdefault(k, len(seen)) for k in keys]


@pytest.mark.parametrize("suf", ["f64", "f32"])
@pytest.mark.parametrize("n1", DIMS)
@pytest.mark.parametrize("n0", DIMS)
def test_matrix_plan_is_the_two_inner_plans_and_the_transposes(n0, n1, suf):
    prec, esz = PREC[suf], ESZ[suf]
    for batch in (1, 3):
        for flags in (0, INV, TOUT, INV | TOUT):
            inverse, tout = bool(flags & INV), bool(flags & TOUT)
            d = pifft.dry_run_matrix(n0, n1, batch, prec, inverse=inverse, transposed_out=tout)
            r = pifft.dry_run(n1, 1, batch * n0, prec, inverse=inverse)
            c = pifft.dry_run(n0, 1, batch * n1, prec, inverse=inverse)
            total = batch * n0 * n1
            tail = [] if tout else ["transpose"]
            assert d["launch_kind"] == r["launch_kind"] + ["transpose"] + c["launch_kind"] + tail
            assert d["launch_mode"] == r["launch_mode"] + [0] + c["launch_mode"] + [0] * len(tail)
            tb = 2 * total * esz
            assert d["launch_bytes"] == r["launch_bytes"] + [tb] + c["launch_bytes"] + [tb] * len(tail)
            assert d["num_launches"] == r["num_launches"] + c["num_launches"] + 1 + len(tail)
            # launch_fn: numbered in order of first use; within a chain equal
            # kernels exactly where the inner plan has them, one id for the
            # transposes, which no pass shares (across the chains the ids may
            # coincide -- the same instance -- or not: tests/test_gpu_matrix.py
            # holds them to the kernels' names)
            fn = d["launch_fn"]
            nr = r["num_launches"]
            rows_fn, t_fn, cols_fn = fn[:nr], fn[nr], fn[nr + 1:nr + 1 + c["num_launches"]]
            assert first_use_ids(rows_fn) == r["launch_fn"] and first_use_ids(cols_fn) == c["launch_fn"]
            assert t_fn not in rows_fn + cols_fn and (tout or fn[-1] == t_fn)
            assert fn == first_use_ids(fn)
            assert d["num_passes"] == r["num_passes"] + c["num_passes"] <= 8
            for key in ("radix", "lines", "vpt"):
                assert d[key] == r[key] + c[key], key
            assert d["worker_interleaved"] == (r["worker_interleaved"] or c["worker_interleaved"])
            assert d["natural_store"] == (r["natural_store"] or c["natural_store"])
            assert d["n"] == n0 * n1 and d["local_n"] == n1 and d["batch"] == batch and d["prec"] == prec
            assert d["workers"] == 1 and d["num_workers"] == 1 and d["first_worker"] == 0 and d["tree_launches"] == 0
            assert d["in_elems"] == d["out_elems"] == total
            assert d["inverse"] == inverse and d["real"] == 0
            # workspace: Z, one W -- the larger of the two chains' -- and both
            # chains' table blobs.  A chain's blob depends on (n, prec) alone,
            # so it is the batch-1 dry run's workspace less that run's W
            # (n values where it has more than one launch, never padded at
            # these sizes); a chain's W is its workspace less its blob.  Held
            # exactly, and so to the bound "Z + the larger inner plan's
            # workspace + both table blobs": two Ws instead of the larger one
            # (only 2^15 x 2^15 has two) would miss both.
            z = total * esz
            blob = {}
            for n, chain in ((n1, r), (n0, c)):
                one = pifft.dry_run(n, 1, 1, prec, inverse=inverse)
                assert one["radix"] == chain["radix"]  # (the same passes, so the same tables)
                blob[n] = one["workspace_bytes"] - (n * esz if one["num_launches"] > 1 else 0)
                assert 0 < blob[n] <= chain["workspace_bytes"]
            w = max(r["workspace_bytes"] - blob[n1], c["workspace_bytes"] - blob[n0])
            assert d["workspace_bytes"] == z + w + blob[n1] + blob[n0]
            assert z <= d["workspace_bytes"] <= z + max(r["workspace_bytes"], c["workspace_bytes"]) + blob[n1] + blob[n0]
        # an inverse plan's info: the forward plan's in every field but flags and launch_fn
        for tout in (0, TOUT):
            f, i = info_of(n0, n1, batch, prec, tout), info_of(n0, n1, batch, prec, tout | INV)
            assert f.flags == tout and i.flags == tout | INV and f.device == i.device == -1
            for name, _ in pifft.PlanInfo._fields_:
                if name in ("flags", "launch_fn"):
                    continue
                a, b = getattr(f, name), getattr(i, name)
                assert (list(a) == list(b)) if hasattr(a, "__len__") else (a == b), name


@pytest.mark.parametrize("args,msg", [
    ((1, 64, 1, 64, 0), "Invalid matrix size"),
    ((64, 1, 1, 64, 0), "Invalid matrix size"),
    ((3, 64, 1, 64, 0), "Invalid matrix size"),
    ((64, 3, 1, 64, 0), "Invalid matrix size"),
    ((0, 64, 1, 64, 0), "Invalid matrix size"),
    ((64, 0, 1, 64, 0), "Invalid matrix size"),
    ((64, 64, 0, 64, 0), "batch must be >= 1"),
    ((64, 64, 1, 48, 0), "prec must be PIFFT_F32 or PIFFT_F64"),
    ((64, 64, 1, 64, 1), "unknown flags 1"),
    ((64, 64, 1, 64, 2), "unknown flags 2"),
    ((64, 64, 1, 64, 4), "unknown flags 4"),
    ((64, 64, 1, 64, 12), "unknown flags 12"),
    ((64, 64, 1, 64, 32), "unknown flags 32"),
    ((64, 64, 1, 64, -1), "unknown flags -1"),
    ((1 << 20, 2, 1 << 13, 64, 0), "must fit the row transforms' 32-bit batch"),
    ((2, 1 << 20, 1 << 13, 32, 16), "must fit the row transforms' 32-bit batch"),
    ((1 << 32, 2, 1, 64, 0), "must fit the row transforms' 32-bit batch"),
])
def test_refusals(args, msg):
    info = pifft.PlanInfo()
    assert pifft.lib().pifft_plan_dry_run_matrix(*args, ctypes.byref(info)) == -1
    assert msg in pifft.last_error()
    h = ctypes.c_void_p()
    n0, n1, batch, prec, flags = args
    assert pifft.lib().pifft_plan_create_matrix(ctypes.byref(h), n0, n1, batch, prec, 0, flags) == -1
    assert msg in pifft.last_error() and not h.value


def test_accepted_flags():
    for flags in (0, 8, 16, 24):
        assert info_of(64, 32, 2, pifft.F32, flags).flags == flags


def test_null_arguments():
    L = pifft.lib()
    assert L.pifft_plan_dry_run_matrix(16, 16, 1, 64, 0, None) == -1 and "info is NULL" in pifft.last_error()
    assert L.pifft_plan_create_matrix(None, 16, 16, 1, 64, 0, 0) == -1 and "plan pointer is NULL" in pifft.last_error()
    a, g = ctypes.c_uint64(), ctypes.c_uint32()
    assert L.pifft_plan_get_dims(None, ctypes.byref(a), ctypes.byref(a)) == -1 and "NULL" in pifft.last_error()
    assert L.pifft_plan_launch_grid(None, 0, ctypes.byref(g)) == -1 and "NULL" in pifft.last_error()


@pytest.mark.parametrize("call", [
    lambda: pifft.MatrixPlan(-2, 64),
    lambda: pifft.MatrixPlan(64, 1 << 64),
    lambda: pifft.MatrixPlan(64, 64, batch=1 << 32),
    lambda: pifft.MatrixPlan(64, 64, batch=-1),
    lambda: pifft.MatrixPlan(64.0, 64),
    lambda: pifft.MatrixPlan(64, 64, prec=16),
    lambda: pifft.dry_run_matrix(64, -64),
    lambda: pifft.dry_run_matrix(64, 64, 1 << 32),
    lambda: pifft.dry_run_matrix(64, 64, 1, 48),
    lambda: pifft.dry_run_matrix(3, 64),
])
def test_binding_argument_checks(call):
    """What ctypes would wrap into the C types (a batch of 2^32 becomes 0, -2
    a huge n0) is refused by the binding before the call."""
    with pytest.raises(pifft.PifftError):
        call()


def test_the_one_dimensional_entry_points_refuse_the_matrix_flag():
    for flags in (16, 24):
        with pytest.raises(pifft.PifftError, match="unknown flags"):
            pifft.dry_run(1 << 10, 1, 1, pifft.F64, flags=flags)
        with pytest.raises(pifft.PifftError, match="unknown flags"):
            pifft.dry_run_instances(1 << 10, 1, 1, pifft.F64, flags=flags)
        with pytest.raises(pifft.PifftError, match="unknown flags"):
            pifft.dry_run_aux(1 << 10, 1, 1, pifft.F64, flags=flags)
        h = ctypes.c_void_p()
        assert pifft.lib().pifft_plan_create_slices(ctypes.byref(h), 1 << 10, 1, 0, 1, 1, 64, 0, flags) == -1
        assert "unknown flags" in pifft.last_error() and not h.value


def test_header_binding_and_abi():
    text = open(os.path.join(ROOT, "include", "pifft.h")).read()
    defs = dict(re.findall(r"#define (PIFFT_[A-Z_0-9]+) (\d+)", text))
    assert int(defs["PIFFT_MATRIX_TRANSPOSED_OUT"]) == pifft.MATRIX_TRANSPOSED_OUT == 16
    assert int(defs["PIFFT_ABI_VERSION"]) == pifft.ABI_VERSION == pifft.lib().pifft_abi_version() == 3
    assert ctypes.sizeof(pifft.PlanInfo) == 5312
    assert pifft.KIND_NAMES[7] == "transpose"
    for name in ("pifft_plan_create_matrix", "pifft_plan_dry_run_matrix", "pifft_plan_get_dims",
                 "pifft_plan_launch_grid"):
        assert name in pifft.SYMBOLS and name in pifft.header_symbols()
        assert hasattr(pifft.lib(), name)
    assert len(pifft.aux_kernels()) == 62
    # the tile rule the tests compute grids from, as the header states it
    m = re.search(r"#define PIFFT_TRANSPOSE_TILE\(prec\) \(\(prec\) == PIFFT_F64 \? (\d+) : (\d+)\)", text)
    assert (int(m.group(1)), int(m.group(2))) == (pifft.transpose_tile(pifft.F64), pifft.transpose_tile(pifft.F32))
    assert pifft.transpose_tile(pifft.F64) * 16 == pifft.transpose_tile(pifft.F32) * 8 == 512
    assert pifft.transpose_tiles(2, 4096, 3, pifft.F64) == 3 * 128 and pifft.transpose_tiles(64, 64, 1, pifft.F32) == 1


def test_matrix_plan_class_does_not_run_the_complex_constructor():
    assert issubclass(pifft.MatrixPlan, pifft.Plan)
    assert "__init__" in vars(pifft.MatrixPlan)
    assert pifft.MatrixPlan.__init__.__code__.co_names.count("pifft_plan_create_matrix") == 1
    assert "super" not in pifft.MatrixPlan.__init__.__code__.co_names


# --- the transpose kernel's index maps on the host ---------------------------
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module")
def transpose(tmp_path_factory):
    """(program, sanitized): built with the sanitizers where the toolchain links them."""
    out = str(tmp_path_factory.mktemp("tr") / "transpose")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-std=c++17", "-O1", "--offload-host-only", "-ffp-contract=off", "-Wall", "-o", out,
           os.path.join(HERE, "native", "transpose_main.hip")]
    if subprocess.run(cmd + SANITIZE, capture_output=True).returncode == 0:
        return out, True
    subprocess.run(cmd, check=True)
    return out, False


def host_cases(prec):
    t = pifft.transpose_tile(prec)
    shapes = [(r, c) for r in (t // 2, t, 2 * t) for c in (t // 2, t, 2 * t)] + [(2, 2), (2, 4096), (4096, 2)]
    for rows, cols in shapes:
        for batch in (1, 3):
            tiles = pifft.transpose_tiles(rows, cols, batch, prec)
            for wgs in sorted({1, 3, tiles - 1, tiles, tiles + 5} - {0}):
                yield rows, cols, batch, wgs, tiles


@pytest.mark.parametrize("suf", ["f64", "f32"])
def test_transpose_maps_on_the_host(transpose, suf):
    """Every output value stored exactly once from the right source, the guard
    values around the output and the LDS stand-in intact, for grids of 1, 3,
    tiles - 1 and >= tiles workgroups; a sanitizer report aborts the program."""
    prog, _ = transpose
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")
    for rows, cols, batch, wgs, tiles in host_cases(PREC[suf]):
        r = subprocess.run([prog, str(rows), str(cols), str(batch), suf[1:], str(wgs)], capture_output=True, text=True,
                           env=env)
        assert r.returncode == 0, (rows, cols, batch, wgs, r.stderr[-2000:])
        got = json.loads(r.stdout)
        assert got == {"tiles": tiles, "unwritten": 0, "bad": 0, "guard": 0}, (rows, cols, batch, wgs, got)
