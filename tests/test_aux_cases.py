"""tests/golden/aux_cases.tsv (tools/aux_cases.py) against the planner and the
library's registry of auxiliary kernels -- every kernel that is not a k_pass
instance: k_tree, k_tree_wil, k_interleave, k_interleave_tile with their
swapping twins, the real plans' fix-ups, the generator.  Here, without a GPU:

  * the registry (pifft.aux_kernels()) is the 26 forward kernels and 36 twins
    the sources define, each named as the demangler prints it;
  * the table and tests/golden/aux_cases_exceptions.txt together name every
    plan-launched registry entry (all but the generator's two) exactly once,
    the exceptions within the project's 5 % cap: at most 3;
  * every row, dry-run under its own tuning variables, launches the kernel it
    claims at the launch index it claims;
  * the committed table and exceptions equal what the tool regenerates;
  * a row without tuning variables plans the same with PIFFT_TUNING unset;
  * PIFFT_STRIDE_GRID_MAX caps the grid of every auxiliary launch of a plan,
    and of none without PIFFT_TUNING=1.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import pifft  # noqa: E402
import aux_cases as ac  # noqa: E402
import instance_cases as ic  # noqa: E402


@pytest.fixture(scope="module")
def table():
    return [tuple(d) for d in pifft.aux_kernels()]


@pytest.fixture(scope="module")
def rows():
    return ac.read_cases()


@pytest.fixture(scope="module")
def exceptions():
    return ac.read_exceptions()


def test_registry(table):
    """Counted from csrc/pifft_kernels.h and csrc/pifft_real.h: per precision
    and L = 1..4 k_tree with SW 1, 2, 3 and k_tree_wil with SW 1; per precision
    the two interleaves with SW 2, the two fix-ups and the generator."""
    want = set()
    for prec in (32, 64):
        for L in (1, 2, 3, 4):
            want |= {(pifft.AUX_TREE, prec, L, sw) for sw in (0, 1, 2, 3)}
            want |= {(pifft.AUX_TREE_WIL, prec, L, sw) for sw in (0, 1)}
        for fam in (pifft.AUX_INTERLEAVE, pifft.AUX_INTERLEAVE_TILE):
            want |= {(fam, prec, 0, 0), (fam, prec, 0, 2)}
        want |= {(pifft.AUX_R2C, prec, 0, 0), (pifft.AUX_C2R, prec, 0, 0), (pifft.AUX_GENERATE, prec, 0, 0)}
    assert len(table) == len(set(table)) == 62 and set(table) == want
    assert sum(1 for d in table if d[3] == 0) == 26 and sum(1 for d in table if d[3]) == 36
    assert len({pifft.aux_kernel_name(d) for d in table}) == 62
    assert pifft.aux_kernel_name((pifft.AUX_TREE, 32, 2, 2)) == "void pifft::k_tree_sw<float, 2, 2>(pifft::TreeArgs)"
    with pytest.raises(pifft.PifftError, match="out of range"):
        pifft._check(pifft.lib().pifft_aux_desc(62, (pifft.ctypes.c_int32 * 4)()), "pifft_aux_desc")


def test_every_kernel_has_a_case_or_a_reason(table, rows, exceptions):
    targets = {d for d in table if d[0] != ac.GENERATE}
    assert len(targets) == 60
    named = [d for _, cov in rows for _, d in cov] + list(exceptions)
    assert sorted(named) == sorted(targets), "the table and the exceptions name every plan-launched kernel exactly once"
    assert len(exceptions) <= ac.MAX_EXCEPTIONS == 3 == len(targets) * 5 // 100
    for key, reason in exceptions.items():
        assert len(reason) > 20 and "MISSING" not in reason, key


def test_rows_are_cases(rows):
    assert len({c for c, _ in rows}) == len({ac.case_id(c) for c, _ in rows}) == len(rows)  # no case, no name twice
    assert rows == sorted(rows, key=ac.sort_key)
    for c, cov in rows:
        assert cov and len({i for i, _ in cov}) == len(cov)
        assert c.batch in (1, 3) and ac.values(c) <= 1 << 16
        assert c.env == tuple(sorted(c.env)) and all(k.startswith("PIFFT_") and k != "PIFFT_TUNING" for k, _ in c.env)


def test_every_row_still_launches_its_kernels(table, rows):
    """Under the row's variables (and PIFFT_TUNING=1, as conftest.py sets it
    for the GPU tests): the stated kernel at each stated launch, a k_pass
    launch (-1) exactly where pifft.dry_run says pass, and the rules the
    table was chosen under."""
    for c, cov in rows:
        with ic.tuning(c.env or None):
            assert os.environ.get("PIFFT_TUNING") == "1"
            ids = ac.launches(c)
            d = ac.describe(c)
        for i, desc in cov:
            assert table[ids[i][0]] == desc, (c, i, desc)
            assert i == [k for k, _ in ids].index(ids[i][0]), "the first launch of that kernel"
        assert len(ids) == d["num_launches"]
        assert [k < 0 for k, _ in ids] == [kind in ("pass", "tree+pass") for kind in d["launch_kind"]]
        assert d["inverse"] == (c.direction in ("inv", "c2r")) and d["real"] == {"r2c": 1, "c2r": 2}.get(c.direction, 0)
        assert ac.preflight(c, d) is None, c
        # a twin only where make_inverse puts one: the launch reading d_in (SW bit 1), the one writing d_out (bit 2)
        real = c.direction in ("r2c", "c2r")
        chain = ids[1:] if c.direction == "c2r" else ids[:-1] if c.direction == "r2c" else ids
        for j, (k, _) in enumerate(chain):
            want = ((1 if j == 0 else 0) | (2 if j == len(chain) - 1 else 0)) if d["inverse"] else 0
            assert k < 0 or table[k][3] == want, (c, j)
        assert not real or table[ids[0 if c.direction == "c2r" else -1][0]][0] in (pifft.AUX_R2C, pifft.AUX_C2R)


def test_committed_files_are_what_the_tool_writes(table):
    best, open_ = ac.search(table)
    assert ac.cases_text(ac.rows_of(best, table)) == open(ac.CASES).read()
    assert ac.exceptions_text(open_, table, ac.read_exceptions()) == open(ac.EXCEPTIONS).read()


def test_untuned_rows_need_no_tuning(rows):
    n = 0
    for c, _ in rows:
        if c.env:
            continue
        with ic.tuning(None):
            on = (ac.launches(c), ac.describe(c))
        with ic.tuning(()):
            assert "PIFFT_TUNING" not in os.environ
            off = (ac.launches(c), ac.describe(c))
        assert on == off, c
        n += 1
    assert 0 < n < len(rows)


CAPPED = [ac.Case(1 << 16, 1 << 16, 0, 1 << 16, 1, 64, ic.NAT, "inv", ()),   # four tree launches, k_interleave
          ac.Case(1 << 16, 32, 0, 32, 3, 32, ic.NAT | ic.SEP, "fwd", ()),    # two tree launches, a pass, k_interleave_tile
          ac.Case(1 << 16, 16, 0, 16, 1, 64, ic.NAT, "fwd", ()),             # k_tree_wil
          ac.Case(1 << 12, 1, 0, 1, 3, 64, ic.NAT, "r2c", ()),
          ac.Case(1 << 13, 2, 0, 2, 3, 32, ic.NAT, "c2r", ())]


@pytest.mark.parametrize("case", CAPPED, ids=ac.case_id)
def test_stride_grid_max_caps_every_auxiliary_launch(case, monkeypatch):
    """PIFFT_STRIDE_GRID_MAX: the cap of stride_grid, at every plan launch that
    goes through it -- and only there, only under PIFFT_TUNING=1, and never
    above the built-in 262144."""
    free = ac.launches(case)
    assert any(k >= 0 and g > 3 for k, g in free), free
    for cap in (1, 3, 7):
        monkeypatch.setenv("PIFFT_STRIDE_GRID_MAX", str(cap))
        got = ac.launches(case)
        assert got == [(k, min(g, cap) if k >= 0 else g) for k, g in free], (cap, got)
    monkeypatch.setenv("PIFFT_STRIDE_GRID_MAX", str(1 << 30))
    assert ac.launches(case) == free
    monkeypatch.setenv("PIFFT_STRIDE_GRID_MAX", "0")
    assert ac.launches(case) == [(k, 1 if k >= 0 else g) for k, g in free]
    monkeypatch.setenv("PIFFT_STRIDE_GRID_MAX", "1")
    monkeypatch.delenv("PIFFT_TUNING")
    assert ac.launches(case) == free
