"""tests/golden/partial_tile_cases.tsv (tools/partial_tile_cases.py) against the
registry and the planner: the table tests/test_gpu_partial_tile.py runs on an
MI355X names, for every compiled single-pass k_pass instance (MODE 0 and 4) of
C > 1 lines per workgroup and for the SW 3 and SW 2 twins of each, plans whose
last tile is partial -- the only launches that meet k_pass's tail path, and
the ones tests/golden/instance_cases.tsv's whole-tile rule keeps out.  Here,
without a GPU:

  * the targets are the registry's 214 instances and their 428 twins; every
    one has its rows (a forward instance and a SW 3 twin two P = 1 rows, at
    batch C + 1 and 2C - 1; a SW 2 twin one row behind a tree) or a reason in
    partial_tile_cases_exceptions.txt, none both, the exceptions within the
    project's 5 % cap;
  * every row, dry-run under its own tuning variables, launches the stated
    descriptor and SW at the stated launch, as the plan's only pass, with
    info.lines[0] == C, and its nlines = batch x count x M / R is no multiple
    of C: the table cannot drift back onto whole tiles;
  * the natural-order store's grid: both precisions, every C, P = 2 and 4
    where C does not divide P, forward and inverse, each planning the
    natural store;
  * no case exceeds 2 x 8192 values (fp32: 2 x 16384);
  * the committed files are what the tool writes, byte for byte;
  * a row without tuning variables plans the same with PIFFT_TUNING unset.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import pifft  # noqa: E402
import instance_cases as ic  # noqa: E402
import partial_tile_cases as pt  # noqa: E402

N_INSTANCES, N_TWINS = 214, 428


@pytest.fixture(scope="module")
def table():
    return [tuple(d) for d in pifft.instances()]


@pytest.fixture(scope="module")
def rows():
    return pt.read_cases()


@pytest.fixture(scope="module")
def exceptions():
    return pt.read_exceptions()


def is_natural(c):
    return c.P > 1 and c.count == c.P


def describe(c):
    return pifft.dry_run(c.n, c.P, c.batch, c.prec, first=c.first, count=c.count, flags=c.flags, inverse=c.inverse)


def test_targets(table):
    """Every MODE 0 / 4 instance of C > 1, and of each the two twins
    twin_reachable gives a single pass: SW 2 and SW 3."""
    targets = pt.universe(table)
    assert len(targets) == len(set(targets)) == N_INSTANCES + N_TWINS
    inst = {d for d, sw in targets if sw == 0}
    assert inst == {d for d in table if d[3] in (0, 4) and d[2] > 1} and len(inst) == N_INSTANCES
    assert {(d, sw) for d, sw in targets if sw} == {(d, sw) for d in inst for sw in (2, 3)}
    # (the 62 others of these modes run one line per workgroup: no tile to be partial)
    assert sum(1 for d in table if d[3] in (0, 4)) == 276


def test_every_target_has_its_rows_or_a_reason(table, rows, exceptions):
    targets = set(pt.universe(table))
    by = {}
    for c, cov in rows:
        if not is_natural(c):
            for _, d, sw in cov:
                by.setdefault((d, sw), []).append(c)
    assert set(by) <= targets, sorted(set(by) - targets)[:5]
    assert set(exceptions) <= targets, sorted(set(exceptions) - targets)[:5]
    both = set(by) & set(exceptions)
    assert not both, f"{len(both)} exceptions have rows, e.g. {sorted(both)[:3]}"
    missing = targets - set(by) - set(exceptions)
    assert not missing, f"{len(missing)} targets with neither rows nor a reason, e.g. {sorted(missing)[:5]}"
    assert sum(1 for _, sw in exceptions if sw == 0) <= N_INSTANCES * 5 // 100 == 10
    assert sum(1 for _, sw in exceptions if sw) <= N_TWINS * 5 // 100 == 21
    for key, reason in exceptions.items():
        assert len(reason) > 20 and "MISSING" not in reason, key
    for (d, sw), cs in by.items():
        prec, R, C, mode = d[:4]
        got = sorted((c.n, c.P, c.first, c.count, c.batch, c.prec, c.flags, c.inverse) for c in cs)
        if sw == 2:
            want = [(2 * R, 2, 1, 1, 2 * C - 1, prec, ic.BR if mode == 4 else ic.SL, True)]
        else:
            want = [(R, 1, 0, 1, b, prec, ic.BR if mode == 4 else ic.NAT, sw == 3)
                    for b in ((3, 5) if C == 2 else (C + 1, 2 * C - 1))]
        assert got == want, (d, sw)
        assert len({c.env for c in cs}) == 1
        if R > 8:
            assert cs[0].env == pt.steering(d), (d, sw)
        else:  # the planner gives C = 64 by itself
            assert C == 64 and cs[0].env == (() if d[4] == 0 else (("PIFFT_NT", "1"),)), (d, sw)


def test_rows_are_cases(rows):
    assert len({c for c, _ in rows}) == len({ic.case_id(c) for c, _ in rows}) == len(rows)  # no case, no name twice
    assert rows == sorted(rows, key=ic.sort_key)   # by (precision, log2 N, batch): the references' order
    for c, cov in rows:
        assert len(cov) == 1  # the plan's one pass
        assert all((sw == 0) != c.inverse for _, _, sw in cov), c
        assert c.env == tuple(sorted(c.env)) and all(k.startswith("PIFFT_") and k != "PIFFT_TUNING" for k, _ in c.env)
        assert c.n * c.batch <= 2 * (16384 if c.prec == 32 else 8192), c


def test_every_row_still_plans_its_launch_on_a_partial_tile(table, rows):
    """Under the row's variables (and PIFFT_TUNING=1, as conftest.py sets it
    for the GPU tests)."""
    for c, cov in rows:
        with ic.tuning(c.env or None):
            assert os.environ.get("PIFFT_TUNING") == "1"
            ids = ic.launches(c)
            d = describe(c)
        assert ic.covers(c, ids, table) == cov, (c, [table[k] if k >= 0 else None for k in ids])
        (i, desc, sw), = cov
        assert d["inverse"] == c.inverse and len(ids) == d["num_launches"]
        assert d["num_passes"] == 1 and [k >= 0 for k in ids] == [False] * i + [True] and i == (c.P > 1)
        assert d["launch_kind"] == ["tree"] * i + ["pass"], (c, d["launch_kind"])
        assert (d["radix"][0], d["lines"][0], d["vpt"][0], d["launch_mode"][i]) == (desc[1], desc[2], desc[6], desc[3])
        assert sw == ((3 if i == 0 else 2) if c.inverse else 0)
        R, C = desc[1], desc[2]
        assert c.n // c.P == R and C > 1
        nlines = c.batch * c.count * (c.n // c.P) // R
        assert nlines == pt.nlines(c, R) and nlines > C and nlines % C != 0, (c, nlines, C)
        assert d["natural_store"] == is_natural(c) and not d["worker_interleaved"], c


def test_natural_store_grid(table, rows):
    """ilv_log != 0 is a launch argument of the MODE 0, NTS 0 instances: per
    precision and C one R, P = 2 and 4 where C does not divide P, at the
    smallest odd batch whose batch x P lines are at least C and no multiple
    of it, forward and inverse."""
    nat = [(c, cov) for c, cov in rows if is_natural(c)]
    seen = {}
    for c, ((_, d, _),) in nat:
        assert c.flags == ic.NAT and d[3] == 0 and d[4] == 0 and dict(c.env)["PIFFT_ILV"] == "1"
        assert dict(c.env)["PIFFT_WORKER_IL"] == "0"
        C = d[2]
        assert c.batch == next(b for b in range(1, 2 * C, 2) if b * c.P >= C and b * c.P % C), c
        seen.setdefault((c.prec, C, c.P), set()).add(c.inverse)
        assert len({dd[1] for cc, ((_, dd, _),) in nat if cc.prec == c.prec and dd[2] == C}) == 1  # one R
    cs = {(d[0], d[2]) for d in table if d[3] in (0, 4) and d[2] > 1}
    assert set(seen) == {(prec, C, P) for prec, C in cs for P in pt.NATURAL_P if P % C}
    assert all(v == {False, True} for v in seen.values())


def test_committed_files_are_what_the_tool_writes(table):
    got, open_ = pt.search(table)
    assert pt.cases_text(got) == open(pt.CASES).read()
    assert pt.exceptions_text(open_, pt.read_exceptions()) == open(pt.EXCEPTIONS).read()


def test_untuned_rows_need_no_tuning(rows):
    """A row without variables gives the same plan with PIFFT_TUNING unset:
    a partial tile any caller with such a batch gets."""
    n = 0
    for c, _ in rows:
        if c.env:
            continue
        with ic.tuning(None):
            on = (ic.launches(c), describe(c))
        with ic.tuning(()):
            assert "PIFFT_TUNING" not in os.environ
            off = (ic.launches(c), describe(c))
        assert on == off, c
        n += 1
    assert 0 < n < len(rows)


def test_generator_is_prefix_stable():
    """tests/test_gpu_partial_tile.py compares a row with the same shape at a
    whole-tile batch, whose first transforms must be the row's: the
    generator's values for a fixed n and seed do not depend on the count."""
    import numpy as np
    import pifft_oracle as oracle
    for dt in (np.complex64, np.complex128):
        for n in (2, 64, 2048):
            long = oracle.generate(n, dt, seed=0xACC0 + ic.log2(n), count=6 * n)
            for k in (1, 3, 5):
                assert oracle.generate(n, dt, seed=0xACC0 + ic.log2(n), count=k * n).tobytes() == long[:k * n].tobytes()


def test_no_row_adds_an_instance(rows):
    """Every instance a row launches is already one of
    tests/golden/instances_*.txt, the lists the registry is generated from."""
    listed = set()
    for name in ("instances_default.txt", "instances_tests.txt", "instances_tests_cpu.txt"):
        with open(os.path.join(pt.GOLD, name)) as f:
            listed |= {ic.parse_desc(ln) for ln in f if ln.strip()}
    assert {d for _, cov in rows for _, d, _ in cov} <= listed
