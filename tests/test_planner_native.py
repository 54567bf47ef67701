"""The planner's policy on its own (csrc/pifft_planner.h: choose_plan, no HIP)
against the library's dry runs: tests/native/planner_main.cpp, built with the
host compiler over a registry read from the committed instance lists, must
choose for every shape the passes, layout and natural-order store that
pifft_plan_dry_run reports -- and refuse the shapes it refuses, with the same
message.  (No GPU.)"""
import os
import subprocess
import sys

import pytest

import pifft

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "planner_main.cpp")
LISTS = [os.path.join(HERE, "golden", f"instances_{k}.txt") for k in ("default", "tests", "tests_cpu")]
sys.path.insert(0, os.path.join(ROOT, "tools"))

F64, F32 = pifft.F64, pifft.F32
NAT, SL, BR, SEP = pifft.OUT_NATURAL, pifft.OUT_SLICES, pifft.OUT_BITREV, pifft.SEPARATE_TREE


def planner_test_shapes():
    """The shapes tests/test_planner.py plans, as (n, P, first, count, batch, prec, flags)."""
    out = [(1 << 20, 1, 0, 1, 1, F64, NAT), (1 << 20, 8, 0, 8, 1, F64, NAT), (1 << 17, 1, 0, 1, 1, F32, NAT)]
    # test_fused_all_worker_rule
    out += [(1 << ln, P, 0, P, 1, F64, NAT) for ln, P in ((21, 8), (28, 8), (21, 2), (23, 16), (22, 16), (28, 16),
                                                          (20, 2), (22, 2), (22, 4), (22, 8), (23, 8), (21, 16))]
    out += [(1 << ln, P, 0, P, 1, F32, NAT) for ln, P in ((21, 2), (24, 8), (28, 8), (20, 8), (21, 8), (22, 8),
                                                          (22, 4), (22, 16), (21, 16))]
    out += [(1 << 18, 4, 0, 4, 4, F64, NAT), (1 << 19, 4, 0, 4, 4, F64, NAT)]
    # single-pass all-worker plans, one-launch plans
    out += [(1 << ln, P, 0, P, b, prec, NAT) for ln, P, prec, b in (
        (17, 8, F64, 1), (14, 2, F64, 1), (16, 16, F32, 1), (18, 16, F64, 1), (14, 8, F64, 1), (14, 16, F64, 1),
        (15, 16, F64, 1), (15, 4, F64, 4), (18, 16, F64, 2), (13, 2, F64, 1), (13, 2, F64, 64), (13, 2, F32, 1),
        (13, 32, F64, 1), (12, 32, F64, 1), (13, 32, F32, 1), (14, 32, F32, 1), (9, 2, F64, 1), (12, 8, F64, 2),
        (12, 4, F32, 4096))]
    out += [(n, P, 0, P, 1, prec, NAT) for prec in (F64, F32)
            for n, P in ((1 << 10, 2), (1 << 10, 16), (1 << 12, 8), (1 << 13, 4), (1 << 13, 16))]
    # natural-order store, the configurations, edge plans
    out += [(1 << 22, 8, 0, 8, 1, F64, NAT), (1 << 16, 8, 0, 8, 1, F64, NAT), (4096, 4, 0, 4, 8192, F32, NAT),
            (1 << 20, 8, 0, 1, 1, F64, SL), (4096, 1, 0, 1, 4096, F32, NAT), (1 << 28, 1, 0, 1, 1, F64, NAT),
            (1 << 29, 1, 0, 1, 1, F64, NAT), (1 << 32, 8, 5, 1, 1, F64, SL), (1 << 28, 8, 7, 1, 1, F64, SL),
            (1 << 28, 1, 0, 1, 1, F32, NAT), (1 << 26, 1, 0, 1, 1, F32, NAT), (1 << 32, 8, 7, 1, 1, F64, SL),
            (2, 1, 0, 1, 1, F64, NAT), (2, 2, 0, 2, 1, F64, NAT), (16, 16, 0, 16, 1, F64, NAT),
            (256, 256, 0, 256, 1, F64, NAT), (1 << 16, 32, 0, 32, 1, F64, NAT), (1 << 20, 32, 0, 32, 1, F64, NAT),
            (1 << 20, 8, 0, 4, 1, F64, SL), (1 << 29, 2, 0, 2, 1, F64, NAT), (1 << 27, 2, 0, 2, 1, F32, NAT)]
    out += [(1 << 28, P, P - 1, 1, 1, F64, SL) for P in (2, 4, 8, 16)]
    out += [(1 << 23, P, 0, P, 1, F64, fl) for P in (1, 8) for fl in (NAT, BR)]
    out += [(1 << 28, 8, 3, 1, 1, F64, BR), (1 << 24, 8, 0, 1, 1, F64, SL), (1 << 24, 8, 0, 1, 1, F64, SL | SEP)]
    out += [(1 << ln, P, P - 1, 1, 1, prec, SL) for prec in (F64, F32) for ln in range(16, 33) for P in (2, 4, 8, 16)]
    out += [(1 << 20, 8, 0, 1, 1, F64, SL), (1 << 21, 8, 7, 1, 1, F64, SL), (1 << 20, 2, 0, 1, 1, F64, SL),
            (1 << 23, 8, 0, 1, 1, F64, SL), (1 << 17, 1, 0, 1, 1, F64, NAT)]
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("planner") / "planner")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", out, SRC], check=True)
    return out


def test_policy_alone_chooses_the_librarys_plans(exe):
    import instance_sweep
    shapes = planner_test_shapes() + instance_sweep.random_shapes(300)
    text = "".join("%d %d %d %d %d %d %d\n" % s for s in shapes)
    lines = subprocess.run([exe] + LISTS, input=text, check=True, capture_output=True, text=True,
                           env=dict(os.environ)).stdout.splitlines()
    assert len(lines) == len(shapes)
    table = pifft.instances()
    plans = refused = 0
    for shp, line in zip(shapes, lines):
        n, P, first, count, batch, prec, flags = shp
        try:
            ids = pifft.dry_run_instances(n, P, batch, prec, first=first, count=count, flags=flags)
        except pifft.PifftError as e:
            assert line == "error " + str(e).split(": ", 1)[1], shp
            refused += 1
            continue
        d = pifft.dry_run(n, P, batch, prec, first=first, count=count, flags=flags)
        head, _, tail = line.partition(" :")
        assert head.startswith("plan "), (shp, line)
        got = dict(kv.split("=") for kv in head.split()[1:])
        passes = [tuple(int(v) for v in p.split()) for p in tail.split(";") if p.strip()]
        assert passes == [table[i] for i in ids if i >= 0], shp
        assert (got["wil"], got["ilv"]) == (str(int(d["worker_interleaved"])), str(int(d["natural_store"]))), shp
        assert (got["fused"] != "0") == ("tree+pass" in d["launch_kind"]), shp
        plans += 1
    assert plans > 300 and refused > 0  # (the random shapes include some no instance serves)


def test_every_default_plan_of_the_domain_is_the_recorded_one(exe):
    """Every shape of the planner's domain (tools/instance_sweep.py shapes, N =
    2^1 .. 2^32) under the default planner: the harness's output for each N
    has the SHA-256 recorded in tests/golden/planner_domain_sha256.txt ("log_n
    digest" per line, made from the header before its rules were split into
    functions).  Any change of any default plan, layout, tree table or refusal
    shows here, not only a change of the instance set."""
    import hashlib
    from concurrent.futures import ThreadPoolExecutor

    import instance_sweep
    with open(os.path.join(HERE, "golden", "planner_domain_sha256.txt")) as f:
        want = {int(ln.split()[0]): ln.split()[1] for ln in f if ln.strip()}
    assert sorted(want) == list(range(1, 33))
    env = {k: v for k, v in os.environ.items() if not k.startswith("PIFFT_")}  # the default planner

    def digest(log_n):
        text = "".join("%d %d %d %d %d %d %d\n" % s for s in instance_sweep.shapes(log_n))
        out = subprocess.run([exe] + LISTS, input=text.encode(), check=True, capture_output=True, env=env).stdout
        assert out.count(b"\n") == text.count("\n"), log_n
        return hashlib.sha256(out).hexdigest()

    with ThreadPoolExecutor(max_workers=4) as ex:  # (four harness processes at a time)
        got = dict(zip(want, ex.map(digest, want)))
    changed = [log_n for log_n in want if got[log_n] != want[log_n]]
    assert not changed, (f"default plans changed at N = 2^{changed}: compare tools/instance_sweep.py --plans FILE.json "
                         "of this build and of the previous one with --compare")
