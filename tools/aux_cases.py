#!/usr/bin/env python3
"""tools/aux_cases.py -- the smallest plan that launches each auxiliary kernel
(no GPU: pifft.dry_run_aux only).

The auxiliary kernels are everything libpifft compiles that is not a k_pass
instance: k_tree, k_tree_wil, k_interleave, k_interleave_tile with their
swapping twins, the real plans' fix-ups and the generator (pifft.aux_kernels(),
the library's own registry).  All but the generator can be launched by a plan.
This tool sweeps dry runs over

  both precisions, log2 N <= 16, every P up to N (M = 1 plans, which have no
  pass at all, included), the worker ranges (all, the first worker, the last,
  the aligned upper half), the three output orders, PIFFT_SEPARATE_TREE,
  forward and inverse, R2C and C2R (N reals, every P up to N/2), batch 1 and 3

and writes

  tests/golden/aux_cases.tsv             per kernel, the smallest plan launching it
  tests/golden/aux_cases_exceptions.txt  kernels no swept plan launches, with reasons

tests/test_aux_cases.py holds the table to the planner (CPU);
tests/test_gpu_aux.py runs every row on the GPU.

A row: n P first count batch prec flags dir env covers
  dir     fwd / inv (complex plans), r2c / c2r (real plans: n reals)
  env     the case's tuning variables, NAME=VALUE joined by ' ' ('-': none)
  covers  launch:family/prec/L/SW joined by ';' (pifft_aux_desc's descriptor)

Smallest: fewest tuning variables first (FORCED below, tried only for kernels
no untuned plan launches), then the fewest complex values N batch, then the
order of the sweep.  A case obeys tools/instance_cases.py's preflight where it
has passes: a multi-pass plan has N >= 2^14 (the accuracy bounds' derivation),
every pass's line count is a multiple of its lines per workgroup.

  python tools/aux_cases.py [--check]
"""
from __future__ import annotations

import argparse
import os
import sys
import time
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cs87project-msolano2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import instance_cases as ic  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
CASES = os.path.join(GOLD, "aux_cases.tsv")
EXCEPTIONS = os.path.join(GOLD, "aux_cases_exceptions.txt")

MAX_LOG = 16
NAT, SL, BR, SEP = ic.NAT, ic.SL, ic.BR, ic.SEP
DIRS = ("fwd", "inv", "r2c", "c2r")
GENERATE = 6  # pifft.AUX_GENERATE: launched by pifft_generate_device, by no plan
MAX_EXCEPTIONS = 3  # the project's 5 % cap, of the 60 plan-launched kernels

# direction: one of DIRS; env: a tuple of (name, value) pairs sorted by name
Case = namedtuple("Case", "n P first count batch prec flags direction env")

# The tuning variables tried, in this order, for kernels no untuned plan
# launches: each forces a plan structure the default planner keeps for larger
# transforms (a multi-pass local FFT, the tree as a launch of its own).
FORCED = ([(("PIFFT_WIL_FUSE", "0"),), (("PIFFT_WORKER_IL", "0"),), (("PIFFT_ILV", "0"),),
           (("PIFFT_WIL_ONE_LAUNCH", "0"),), (("PIFFT_WIL_SINGLE", "0"),)] +
          [(("PIFFT_SINGLE_MAX_LOG", str(k)),) for k in range(13, 6, -1)] +
          [(("PIFFT_SINGLE_MAX_LOG", str(k)), ("PIFFT_WIL_FUSE", "0")) for k in range(13, 6, -1)])


def fmt(desc) -> str:
    return "family=%d prec=%d L=%d sw=%d" % tuple(desc)


def values(c: Case) -> int:
    """Complex values of the case's input."""
    return (c.n // 2 if c.direction in ("r2c", "c2r") else c.n) * c.batch


def launches(c: Case) -> list:
    """(registry index or -1, grid) per launch under the current environment."""
    import pifft
    if c.direction in ("r2c", "c2r"):
        return pifft.dry_run_aux_real(c.n, c.P, c.batch, c.prec, inverse=c.direction == "c2r")
    return pifft.dry_run_aux(c.n, c.P, c.batch, c.prec, first=c.first, count=c.count, flags=c.flags,
                             inverse=c.direction == "inv")


def describe(c: Case) -> dict:
    import pifft
    if c.direction in ("r2c", "c2r"):
        return pifft.dry_run_real(c.n, c.P, c.batch, c.prec, inverse=c.direction == "c2r")
    return pifft.dry_run(c.n, c.P, c.batch, c.prec, first=c.first, count=c.count, flags=c.flags,
                         inverse=c.direction == "inv")


def preflight(c: Case, d: dict):
    """None, or why the case breaks a rule (instance_cases.preflight on the
    complex plan inside; a plan without passes has none to break)."""
    if not d["radix"]:
        return None
    inner = ic.Case(c.n // 2 if c.direction in ("r2c", "c2r") else c.n, c.P, c.first, c.count, c.batch, c.prec,
                    c.flags, c.direction in ("inv", "c2r"), c.env)
    return ic.preflight(inner, list(zip(d["radix"], d["lines"])), d["worker_interleaved"])


def covers(ids: list, table: list, mine) -> tuple:
    """((launch, descriptor), ...): the first launch of each auxiliary kernel
    of a plan that is among the registry indices `mine` -- those this case is
    the smallest for, so the table names every kernel once."""
    seen, out = set(), []
    for i, (k, _) in enumerate(ids):
        if k in mine and k not in seen:
            seen.add(k)
            out.append((i, table[k]))
    return tuple(out)


def grid():
    """Every swept shape, smallest first."""
    out = []
    for prec in (32, 64):
        for logn in range(1, MAX_LOG + 1):
            n = 1 << logn
            for lp in range(0, logn + 1):
                P = 1 << lp
                ranges = [(0, P)] if P == 1 else [(0, P), (0, 1), (P - 1, 1)] + ([(P // 2, P // 2)] if P >= 4 else [])
                for first, count in ranges:
                    for order in ((NAT, SL, BR) if count == P else (SL, BR)):
                        for sep in ((0, SEP) if P > 1 else (0,)):
                            for b in (1, 3):
                                for direction in ("fwd", "inv"):
                                    out.append(Case(n, P, first, count, b, prec, order | sep, direction, ()))
                if logn >= 2 and lp < logn:  # n reals: the n/2-point plan splits over P <= n/2 workers
                    for b in (1, 3):
                        for direction in ("r2c", "c2r"):
                            out.append(Case(n, P, 0, P, b, prec, NAT, direction, ()))
    out.sort(key=lambda c: (values(c), c.prec, c.n, c.P, c.count, c.first, c.flags, DIRS.index(c.direction)))
    return out


def search(table: list) -> tuple:
    """({registry index: (Case, launch ids)}, the plan-launched indices with no case)."""
    import pifft
    targets = {k for k, d in enumerate(table) if d[0] != GENERATE}
    best = {}
    shapes = grid()
    for env in [()] + FORCED:
        if not targets - set(best):
            break
        with ic.tuning(env):
            for shp in shapes:
                c = shp._replace(env=env)
                try:
                    ids = launches(c)
                except pifft.PifftError:
                    continue
                new = {k for k, _ in ids if k >= 0} - set(best)
                if new and preflight(c, describe(c)) is None:
                    for k in new:
                        best[k] = (c, ids)
    return best, sorted(targets - set(best))


def rows_of(best: dict, table: list) -> list:
    """[(Case, covers)]: a chosen case once, covering the kernels it is the smallest plan for."""
    mine = {}
    for k, (c, _) in best.items():
        mine.setdefault(c, set()).add(k)
    rows = {c: covers(ids, table, mine[c]) for c, ids in best.values()}
    return sorted(rows.items(), key=sort_key)


def sort_key(row):
    c = row[0]
    return (c.prec, ic.log2(c.n), c.batch, c.P, c.first, c.count, c.flags, DIRS.index(c.direction), c.env)


def case_id(c: Case) -> str:
    env = "-" + ",".join(f"{k[len('PIFFT_'):]}={v}" for k, v in c.env) if c.env else ""
    return f"f{c.prec}-2^{ic.log2(c.n)}-P{c.P}-q{c.first}+{c.count}-fl{c.flags}-b{c.batch}-{c.direction}{env}"


# ----------------------------------------------------------------- files ---
def cases_text(rows: list) -> str:
    out = ["# tools/aux_cases.py: n P first count batch prec flags dir env covers(launch:family/prec/L/SW)\n"]
    for c, cov in rows:
        cv = ";".join("%d:%s" % (i, "/".join(str(v) for v in d)) for i, d in cov)
        out.append("\t".join(str(v) for v in (c.n, c.P, c.first, c.count, c.batch, c.prec, c.flags, c.direction,
                                              ic.env_text(c.env), cv)) + "\n")
    return "".join(out)


def read_cases(path: str = CASES) -> list:
    rows = []
    with open(path) as f:
        for ln in f:
            if not ln.strip() or ln.startswith("#"):
                continue
            n, P, first, count, batch, prec, flags, direction, env, cv = ln.rstrip("\n").split("\t")
            assert direction in DIRS, ln
            e = () if env == "-" else tuple(tuple(kv.split("=", 1)) for kv in env.split(" "))
            cov = []
            for item in cv.split(";"):
                i, d = item.split(":")
                cov.append((int(i), tuple(int(v) for v in d.split("/"))))
            rows.append((Case(int(n), int(P), int(first), int(count), int(batch), int(prec), int(flags), direction, e),
                         tuple(cov)))
    return rows


def read_exceptions(path: str = EXCEPTIONS) -> dict:
    """{descriptor: reason}; a line: family=F prec=P L=L sw=S : <reason>"""
    out = {}
    with open(path) as f:
        for ln in f:
            if not ln.strip() or ln.startswith("#"):
                continue
            head, _, reason = ln.strip().partition(" : ")
            key = ic.parse_desc(head)
            assert key not in out, ln
            out[key] = reason.strip()
    return out


def exceptions_text(open_: list, table: list, old: dict) -> str:
    out = ["# auxiliary kernels (pifft_aux_desc) no plan of tools/aux_cases.py's sweep launches:\n"
           "# family=<PIFFT_AUX_*> prec=<32|64> L=<levels> sw=<SW> : <reason>\n"]
    for k in open_:
        out.append(f"{fmt(table[k])} : {old.get(tuple(table[k]), 'REASON MISSING')}\n")
    return "".join(out)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--check", action="store_true", help="compare with the committed files, write nothing")
    args = ap.parse_args()
    import pifft
    t0 = time.time()
    table = [tuple(d) for d in pifft.aux_kernels()]
    best, open_ = search(table)
    rows = rows_of(best, table)
    old = read_exceptions() if os.path.exists(EXCEPTIONS) else {}
    texts = {CASES: cases_text(rows), EXCEPTIONS: exceptions_text(open_, table, old)}
    print(f"{len(table)} auxiliary kernels, {sum(1 for d in table if d[0] != GENERATE)} of them plan-launched: "
          f"{len(rows)} cases ({sum(1 for c, _ in rows if not c.env)} without tuning variables) cover {len(best)}, "
          f"{len(open_)} exceptions; {time.time() - t0:.0f} s")
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
