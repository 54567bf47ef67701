#!/usr/bin/env python3
"""tools/partial_tile_cases.py -- every single-pass k_pass instance and twin on a
partial last tile (no GPU: pifft.dry_run_instances only).

k_pass has one tail path: where a launch's line count is no multiple of the
tile's C lines, the last workgroup runs with idle lines (csrc/pifft_kernels.h:
fp32 idle lanes load the last line again, fp64 ones load nothing, and every
store is guarded by line < nlines).  Only the single pass (MODE 0 and 4) can
meet it -- in a multi-pass plan C divides a transform's lines -- and there the
lines are whole transforms: nlines = batch x workers of the plan.
tools/instance_cases.py runs whole tiles only (its preflight), so this tool
names, for every registry instance of MODE 0 or 4 with C > 1 and for the two
twins of each (twin_reachable: SW 3 the only launch, SW 2 behind a tree),
plans whose last tile is partial, and writes

  tests/golden/partial_tile_cases.tsv             one row per case
  tests/golden/partial_tile_cases_exceptions.txt  targets without rows, with reasons

in tools/instance_cases.py's formats.  tests/test_partial_tile_cases.py holds
the table to the planner (CPU); tests/test_gpu_partial_tile.py runs every row.

The plans are steered as instance_cases.directed does for these modes:
PIFFT_MIN_WORKGROUPS=1, PIFFT_SINGLE_C{32,64}=C, PIFFT_NT=NTS (and
PIFFT_SINGLE_MAX_LOG above R = 2^14, PIFFT_SINGLE_VPT off 16).  At R <= 8 the
planner gives C = 64 by itself: those rows carry no variable where the default
NTS is the instance's, else PIFFT_NT alone.

Rows per forward instance (n = R, P = 1; natural order for MODE 0, bit-reversed
for MODE 4): batch C + 1 -- a whole tile, then a tile with one live line -- and
batch 2C - 1 -- one idle line, so whole waves idle at small R (C = 2: 3 and 5).
Per SW 3 twin the same two rows, inverse.  Per SW 2 twin one inverse row behind
a tree: n = 2R, P = 2, the second worker alone, slice-major (MODE 0) or
bit-reversed (MODE 4), batch 2C - 1.

The last pass's natural-order store (PassArgs::ilv_log, a launch argument, not
an instance) gets a small grid of its own: per precision and C one R (the
largest with a MODE 0, NTS 0 instance inside the single pass's default tile,
R C <= 4096 -- the C the planner itself pairs with that R; else the smallest),
P = 2 and 4, all workers, natural order, PIFFT_ILV=1 PIFFT_WORKER_IL=0, forward and
inverse, at the smallest odd batch with batch P >= C and batch P mod C != 0
(none where C divides P).

  python tools/partial_tile_cases.py [--check] [--figures LOG]
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cs87project-msolano2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import instance_cases as ic  # noqa: E402
from instance_cases import Case, NAT, SL, BR  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
CASES = os.path.join(GOLD, "partial_tile_cases.tsv")
EXCEPTIONS = os.path.join(GOLD, "partial_tile_cases_exceptions.txt")
TOOL = "tools/partial_tile_cases.py"

SINGLE = (0, 4)  # the single pass: natural / slice-major store, bit-reversed store
NATURAL_P = (2, 4)
NATURAL_TILE = 4096  # pick_lines' default single-pass tile (PIFFT_SINGLE_TILE{32,64}): C = 4096 / R


def single_instances(table: list) -> list:
    return [tuple(d) for d in table if d[3] in SINGLE and d[2] > 1]


def universe(table: list) -> list:
    """Every target: (descriptor, 0) per single-pass instance of C > 1,
    (descriptor, SW) per twin of one the library holds."""
    mine = set(single_instances(table))
    return [(d, 0) for d in single_instances(table)] + [(d, sw) for d, sw in ic.twin_universe(table) if d in mine]


def steering(desc: tuple) -> tuple:
    """The tuning variables that make the single pass of an R-point local FFT
    this instance (instance_cases.directed's, MODE 0 and 4), sorted by name."""
    prec, R, C, _, nts, _, vpt = desc
    env = {"PIFFT_NT": str(nts), "PIFFT_MIN_WORKGROUPS": "1", f"PIFFT_SINGLE_C{prec}": str(C)}
    if ic.log2(R) > 14:
        env["PIFFT_SINGLE_MAX_LOG"] = str(ic.log2(R))
    if vpt != 16:
        env["PIFFT_SINGLE_VPT"] = str(vpt)
    return tuple(sorted(env.items()))


def batches(C: int) -> tuple:
    return (3, 5) if C == 2 else (C + 1, 2 * C - 1)


def shapes(desc: tuple, sw: int) -> list:
    """(n, P, first, count, batch, prec, flags, inverse) of a target's rows."""
    prec, R, C, mode = desc[:4]
    if sw == 2:
        return [(2 * R, 2, 1, 1, 2 * C - 1, prec, BR if mode == 4 else SL, True)]
    return [(R, 1, 0, 1, b, prec, BR if mode == 4 else NAT, sw != 0) for b in batches(C)]


def nlines(case: Case, R: int) -> int:
    """Lines of a single-pass launch: whole transforms of M = R points."""
    return case.batch * case.count * (case.n // case.P) // R


def plans_target(case: Case, desc: tuple, sw: int, table: list):
    """The case's covers under its own variables if its plan launches the
    target on a partial last tile of C lines, else None."""
    import pifft
    with ic.tuning(case.env):
        try:
            ids = ic.launches(case)
            d = pifft.dry_run(case.n, case.P, case.batch, case.prec, first=case.first, count=case.count,
                              flags=case.flags, inverse=case.inverse)
        except pifft.PifftError:
            return None
    cov = ic.covers(case, ids, table)
    if d["num_passes"] != 1 or d["lines"][0] != desc[2] or nlines(case, desc[1]) % desc[2] == 0:
        return None
    return cov if any(t == desc and s == sw for _, t, s in cov) else None


def rows_of_target(desc: tuple, sw: int, table: list):
    """[(Case, covers)] of one target under the fewest variables, or None."""
    full = steering(desc)
    envs = [(), tuple(kv for kv in full if kv[0] == "PIFFT_NT"), full] if desc[1] <= 8 else [full]
    for env in envs:
        rows = []
        for shp in shapes(desc, sw):
            case = Case(*shp, env)
            cov = plans_target(case, desc, sw, table)
            if cov is None:
                break
            rows.append((case, cov))
        else:
            return rows
    return None


def natural_rows(table: list) -> list:
    """The natural-order store's grid (module docstring)."""
    rows = []
    for prec in (32, 64):
        by_c = {}
        for d in single_instances(table):
            if d[0] == prec and d[3] == 0 and d[4] == 0 and d[6] == 16:
                by_c.setdefault(d[2], []).append(d)
        for C in sorted(by_c):
            within = [d for d in by_c[C] if d[1] * C <= NATURAL_TILE]
            desc = max(within, key=lambda d: d[1]) if within else min(by_c[C], key=lambda d: d[1])
            env = dict(steering(desc))
            env.update({"PIFFT_ILV": "1", "PIFFT_WORKER_IL": "0"})
            env = tuple(sorted(env.items()))
            for P in NATURAL_P:
                if P % C == 0:
                    continue
                batch = next(b for b in range(1, 2 * C, 2) if b * P >= C and b * P % C)
                for inverse in (False, True):
                    case = Case(desc[1] * P, P, 0, P, batch, prec, NAT, inverse, env)
                    cov = plans_target(case, desc, 2 if inverse else 0, table)
                    assert cov is not None, f"the natural-store case {case} does not plan {ic.fmt(desc)}"
                    with ic.tuning(case.env):
                        import pifft
                        assert pifft.dry_run(case.n, P, batch, prec, flags=NAT, inverse=inverse)["natural_store"], case
                    rows.append((case, cov))
    return rows


def search(table: list) -> tuple:
    """([(Case, covers)] sorted, [(descriptor, SW)] without rows)."""
    rows, open_ = [], []
    for desc, sw in universe(table):
        got = rows_of_target(desc, sw, table)
        if got is None:
            open_.append((desc, sw))
        else:
            rows += got
    rows += natural_rows(table)
    assert len({c for c, _ in rows}) == len(rows)
    return sorted(rows, key=ic.sort_key), sorted(open_)


# ----------------------------------------------------------------- files ---
def read_cases(path: str = CASES) -> list:
    return ic.read_cases(path)


def read_exceptions(path: str = EXCEPTIONS) -> dict:
    return ic.read_exceptions(path)


def cases_text(rows: list) -> str:
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cases.tsv")
        ic.write_cases(path, rows, TOOL)
        return open(path).read()


def exceptions_text(open_: list, old: dict) -> str:
    out = ["# single-pass instances of C > 1 (sw=0) and their twins (sw=2, 3) without a row in\n"
           "# tests/golden/partial_tile_cases.tsv: <descriptor> sw=<SW> : <reason>\n"]
    for d, sw in open_:
        out.append(f"{ic.fmt(d)} sw={sw} : {old.get((d, sw), 'REASON MISSING')}\n")
    return "".join(out)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--check", action="store_true", help="compare with the committed files, write nothing")
    ap.add_argument("--figures", metavar="LOG", help="print the ACC lines of a GPU run's log as a table, by row")
    args = ap.parse_args()
    if args.figures:
        sys.stdout.write(ic.figures(args.figures, label="ptl", rows=read_cases()))
        return 0
    import pifft
    table = [tuple(d) for d in pifft.instances()]
    rows, open_ = search(table)
    old = read_exceptions() if os.path.exists(EXCEPTIONS) else {}
    texts = {CASES: cases_text(rows), EXCEPTIONS: exceptions_text(open_, old)}
    targets = universe(table)
    print(f"{sum(1 for _, sw in targets if sw == 0)} single-pass instances of C > 1, "
          f"{sum(1 for _, sw in targets if sw)} twins: {len(rows)} cases "
          f"({sum(1 for c, _ in rows if not c.env)} without tuning variables, "
          f"{sum(1 for c, _ in rows if c.P > 1 and c.count == c.P)} natural-store), {len(open_)} exceptions")
    if args.check:
        stale = [p for p, t in texts.items() if not os.path.exists(p) or open(p).read() != t]
        for p in stale:
            print(f"stale: {os.path.relpath(p, ROOT)}")
        return 1 if stale else 0
    for p, t in texts.items():
        with open(p, "w") as f:
            f.write(t)
    return 0


if __name__ == "__main__":
    sys.exit(main())
