"""tests/golden/instance_cases.tsv (tools/instance_cases.py) against the planner:
the table tests/test_gpu_instances.py runs on an MI355X names, for every
compiled k_pass instance and every swapping twin an inverse plan can reach, one
small plan that launches it -- or tests/golden/instance_cases_exceptions.txt
says why none does.  Here, without a GPU:

  * the table and the exceptions together are the registry (pifft.instances())
    and its twins (registry x SW 1..3 under csrc/pifft_table.h twin_reachable,
    asked of tests/native/twins_main.cpp), the exceptions within 5 % of each;
  * every row, dry-run under its own tuning variables, still launches the
    stated instances at the stated launches -- a planner change that moves a
    case fails here, not silently on the GPU;
  * every row's launch geometry obeys the rules the table was chosen under
    (instance_cases.preflight, on pifft.dry_run's radix and lines): N batch <=
    2^20, a forced case at most two passes, a multi-pass case N >= 2^14, every
    pass's lines a multiple of its lines per workgroup, which do not exceed
    the lines of one transform (times P worker-interleaved; of a single pass,
    whose lines are whole transforms, their number);
  * a row without tuning variables plans the same with PIFFT_TUNING unset.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import pifft  # noqa: E402
import instance_cases as ic  # noqa: E402

N_TWINS = 1163


@pytest.fixture(scope="module")
def table():
    return [tuple(d) for d in pifft.instances()]


@pytest.fixture(scope="module")
def rows():
    return ic.read_cases()


@pytest.fixture(scope="module")
def exceptions():
    return ic.read_exceptions()


def test_twin_rule(table):
    """twins_main.cpp's answers are the header's rule: by the pass MODE's
    place in a plan, 1163 twins in all -- every one of them compiled (an
    inverse dry run of a plan that needs a missing twin fails:
    tests/test_inverse_plan.py)."""
    twins = ic.twin_universe(table)
    assert len(twins) == len(set(twins)) == N_TWINS
    by = {}
    for d, sw in twins:
        by.setdefault(d, []).append(sw)
    assert set(by) == set(table)  # every instance has a twin
    for (prec, R, C, mode, nts, lp, vpt), sws in by.items():
        want = ([2, 3] if mode in (0, 4) else [1] if mode in (1, 3) else
                [1, 3] if mode == 11 and C == 1 << lp else [1] if mode == 11 else [2])
        assert sws == want, (mode, C, lp, sws)


def test_every_instance_and_twin_has_a_case_or_a_reason(table, rows, exceptions):
    targets = set(ic.universe(table))
    assert len(targets) == len(table) + N_TWINS
    covered = {(d, sw) for _, cov in rows for _, d, sw in cov}
    assert covered <= targets, sorted(covered - targets)[:5]
    assert set(exceptions) <= targets, sorted(set(exceptions) - targets)[:5]
    both = covered & set(exceptions)
    assert not both, f"{len(both)} exceptions have a row, e.g. {sorted(both)[:3]}"
    missing = targets - covered - set(exceptions)
    assert not missing, f"{len(missing)} instances / twins with neither a case nor a reason, e.g. {sorted(missing)[:5]}"
    # 5 % of each, a cap
    assert sum(1 for _, sw in exceptions if sw == 0) <= len(table) * 5 // 100 == 42
    assert sum(1 for _, sw in exceptions if sw) <= N_TWINS * 5 // 100 == 58
    for key, reason in exceptions.items():
        assert len(reason) > 20 and "MISSING" not in reason, key


def test_rows_are_cases(rows):
    assert len({c for c, _ in rows}) == len({ic.case_id(c) for c, _ in rows}) == len(rows)  # no case, no name twice
    assert rows == sorted(rows, key=ic.sort_key)   # by (precision, log2 N, batch): the references' order
    for c, cov in rows:
        assert cov and len({i for i, _, _ in cov}) == len(cov)
        assert all((sw == 0) != c.inverse for _, _, sw in cov), c
        assert c.env == tuple(sorted(c.env)) and all(k.startswith("PIFFT_") and k != "PIFFT_TUNING" for k, _ in c.env)
    # every row is needed: it launches an instance or twin no other row does
    times = {}
    for _, cov in rows:
        for t in {(d, sw) for _, d, sw in cov}:
            times[t] = times.get(t, 0) + 1
    for c, cov in rows:
        assert any(times[(d, sw)] == 1 for _, d, sw in cov), c


def describe(c):
    return pifft.dry_run(c.n, c.P, c.batch, c.prec, first=c.first, count=c.count, flags=c.flags, inverse=c.inverse)


def test_every_row_still_plans_its_launches(table, rows):
    """Under the row's variables (and PIFFT_TUNING=1, as conftest.py sets it
    for the GPU tests): the stated instance at each stated launch, and exactly
    the launches the coverage rule gives."""
    for c, cov in rows:
        with ic.tuning(c.env or None):
            assert os.environ.get("PIFFT_TUNING") == "1"
            ids = ic.launches(c)
            d = describe(c)
        assert ic.covers(c, ids, table) == cov, (c, [table[k] if k >= 0 else None for k in ids])
        assert d["inverse"] == c.inverse and len(ids) == d["num_launches"]
        # dry_run's own description of the covered launches
        passes = [i for i, k in enumerate(ids) if k >= 0]
        assert len(passes) == d["num_passes"]
        for i, desc, _ in cov:
            p = passes.index(i)
            assert (d["radix"][p], d["lines"][p], d["vpt"][p], d["launch_mode"][i]) == (desc[1], desc[2], desc[6], desc[3])
            assert d["launch_kind"][i] in ("pass", "tree+pass")


def test_launch_geometry(rows):
    for c, _ in rows:
        with ic.tuning(c.env or None):
            d = describe(c)
        why = ic.preflight(c, list(zip(d["radix"], d["lines"])), d["worker_interleaved"])
        assert why is None, (c, why)
        assert len(d["radix"]) == d["num_passes"] <= 8


def test_preflight_refuses_what_it_should():
    mk = lambda **kw: ic.Case(**{**dict(n=1 << 16, P=1, first=0, count=1, batch=1, prec=64, flags=0, inverse=False,
                                        env=()), **kw})
    assert ic.preflight(mk(), [(256, 16), (256, 16)], False) is None
    assert "2^20" in ic.preflight(mk(batch=32), [(256, 16), (256, 16)], False)
    assert "2^14" in ic.preflight(mk(n=1 << 12), [(64, 16), (64, 16)], False)
    assert "two passes" in ic.preflight(mk(n=1 << 18, env=(("PIFFT_NT", "1"),)), [(64, 4)] * 3, False)
    assert ic.preflight(mk(n=1 << 18), [(64, 4)] * 3, False) is None
    assert "multiple" in ic.preflight(mk(n=1 << 10, batch=3), [(1024, 2)], False)
    assert "exceeds" in ic.preflight(mk(batch=2), [(4096, 32), (16, 64)], False)
    assert ic.preflight(mk(P=4, count=4), [(1024, 64), (16, 64)], True) is None   # 16 lines x P
    assert "multiple" in ic.preflight(mk(n=1 << 10), [(1024, 4)], False)  # one transform, four lines
    assert ic.preflight(mk(n=1 << 10, batch=4), [(1024, 4)], False) is None


def test_untuned_rows_need_no_tuning(rows):
    """A row without variables gives the same plan with PIFFT_TUNING unset:
    a plan any caller gets."""
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
