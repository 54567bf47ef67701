#!/usr/bin/env python3
"""tools/instance_cases.py -- one small plan for every compiled k_pass instance
and every swapping twin (no GPU: pifft.dry_run_instances only).

Searches (shape, flags, direction, tuning variables) for plans of at most 2^20
complex values that launch each registry instance (a forward case covers the
instance of each of its pass launches) and each twin an inverse plan can reach
(csrc/pifft_table.h twin_reachable, asked of tests/native/twins_main.cpp: an
inverse case covers the twin of the launch that reads d_in, SW bit 1, and of
the launch that writes d_out, SW bit 2 -- the SW csrc/pifft.hip make_inverse
passes to find_twin), and writes

  tests/golden/instance_cases.tsv             one row per case
  tests/golden/instance_cases_exceptions.txt  what no case reaches, with reasons

tests/test_instance_cases.py holds the table to the planner (CPU);
tests/test_gpu_instances.py runs every row against the long-double reference.

A row: n P first count batch prec flags dir env covers
  dir     fwd / inv
  env     the case's tuning variables, NAME=VALUE joined by ' ' ('-': none)
  covers  launch:prec/R/C/mode/nts/lp/vpt:SW joined by ';'

The rules a case obeys (preflight): N batch <= 2^20 and batch <= 2^10 (the GPU
test checks transform by transform); a forced case has at most
two passes; a multi-pass case has N >= 2^14 (the accuracy bounds' derivation
holds from there); every pass's line count is a multiple of its lines per
workgroup C, and C does not exceed the lines of one transform (times P for the
worker-interleaved layout; a single pass's lines are whole transforms, so
there C is capped by their number, as single_pass asks of pick_lines).

The search: every default plan of the shape grid first; then, per instance or
twin still open, the shapes its descriptor allows under the subsets of the
tuning variables that could steer the planner to it, fewest variables first.
The table is a greedy cover: cases without tuning variables first, then one
variable, two, ...; in a tier the case covering most, then the smallest.

  python tools/instance_cases.py [--jobs 8] [--check] [--figures LOG]
"""
from __future__ import annotations

import argparse
import contextlib
import itertools
import os
import subprocess
import sys
import tempfile
import time
from collections import namedtuple
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cs87project-msolano2_amd"))

GOLD = os.path.join(ROOT, "tests", "golden")
CASES = os.path.join(GOLD, "instance_cases.tsv")
EXCEPTIONS = os.path.join(GOLD, "instance_cases_exceptions.txt")
TWINS_SRC = os.path.join(ROOT, "tests", "native", "twins_main.cpp")

MAX_VALUES = 1 << 20   # N batch of a case
MULTI_MIN_N = 1 << 14  # a multi-pass case's smallest N
MAX_BATCH = 1 << 10    # the GPU test checks (and computes references) transform by transform
NAT, SL, BR, SEP = 0, 1, 2, 4  # pifft.OUT_* and pifft.SEPARATE_TREE

# env: a tuple of (name, value) pairs sorted by name; inverse: bool
Case = namedtuple("Case", "n P first count batch prec flags inverse env")


def fmt(desc) -> str:
    return "prec=%d R=%d C=%d mode=%d nts=%d lp=%d vpt=%d" % tuple(desc)


def parse_desc(text: str) -> tuple:
    return tuple(int(kv.split("=")[1]) for kv in text.split())


@contextlib.contextmanager
def tuning(env):
    """The process environment of a case: no PIFFT_* variable but the
    library's path; with tuning variables, PIFFT_TUNING=1 and those.
    env None leaves PIFFT_TUNING as the caller set it (tests)."""
    saved = {k: v for k, v in os.environ.items() if k.startswith("PIFFT_") and k != "PIFFT_LIB"}
    keep = saved.get("PIFFT_TUNING") if env is None else None
    for k in saved:
        del os.environ[k]
    try:
        if keep is not None:
            os.environ["PIFFT_TUNING"] = keep
        if env:
            os.environ["PIFFT_TUNING"] = "1"
            for k, v in env:
                os.environ[k] = v
        yield
    finally:
        for k in [k for k in os.environ if k.startswith("PIFFT_") and k != "PIFFT_LIB"]:
            del os.environ[k]
        os.environ.update(saved)


def launches(case: Case) -> list:
    """Registry index per launch (-1: tree / interleave) of the case's plan
    under the current environment; PifftError where the planner refuses."""
    import pifft
    return pifft.dry_run_instances(case.n, case.P, case.batch, case.prec, first=case.first, count=case.count,
                                   flags=case.flags, inverse=case.inverse)


def covers(case: Case, ids: list, table: list) -> tuple:
    """((launch, descriptor, SW), ...) a case with these launches covers."""
    if not case.inverse:
        return tuple((i, table[k], 0) for i, k in enumerate(ids) if k >= 0)
    last = len(ids) - 1
    out = []
    for i in sorted({0, last}):
        sw = (1 if i == 0 else 0) | (2 if i == last else 0)
        if ids[i] >= 0:
            out.append((i, table[ids[i]], sw))
    return tuple(out)


def preflight(case: Case, passes: list, wil: bool):
    """None, or why the case breaks a rule.  passes: (R, C) per pass, in order
    (pifft.dry_run's radix and lines); wil: its worker_interleaved."""
    if case.n * case.batch > MAX_VALUES:
        return "N batch > 2^20"
    if case.batch > MAX_BATCH:
        return "batch > 2^10"
    if not passes:
        return "no pass launch"
    if len(passes) > 2 and case.env:
        return "a forced plan of more than two passes"
    if len(passes) >= 2 and case.n < MULTI_MIN_N:
        return "a multi-pass plan below N = 2^14"
    m = case.n // case.P
    ntrans = case.batch * case.count
    for R, C in passes:
        per = m // R  # lines of one transform
        if per < 1 or per * R != m:
            return f"R = {R} does not divide M = {m}"
        if (ntrans * per) % C:
            return f"{ntrans * per} lines are no multiple of C = {C}"
        # a single pass's lines are whole transforms: pick_lines caps C by their number (single_pass)
        cap = ntrans if len(passes) == 1 and not wil else per * case.P if wil else per
        if C > cap:
            return f"C = {C} exceeds the {cap} lines it may span"
    return None


def twin_universe(table: list) -> list:
    """[(descriptor, SW)] of every twin an inverse plan can reach: the
    registry x SW 1..3 under twin_reachable, from the header itself."""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "twins")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, TWINS_SRC], check=True)
        text = "".join("%d %d %d %d %d %d %d\n" % tuple(d) for d in table)
        lines = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(table)
    out = []
    for d, line in zip(table, lines):
        head, _, tail = line.partition(" : ")
        assert tuple(int(v) for v in head.split()) == tuple(d), line
        out += [(tuple(d), sw) for sw, on in zip((1, 2, 3), tail.split()) if on == "1"]
    return out


def universe(table: list) -> list:
    """Every target: (descriptor, 0) per instance, (descriptor, SW) per twin."""
    return [(tuple(d), 0) for d in table] + twin_universe(table)


# ----------------------------------------------------------------- files ---
def env_text(env) -> str:
    return " ".join(f"{k}={v}" for k, v in env) if env else "-"


def write_cases(path: str, rows: list, tool: str = "tools/instance_cases.py") -> None:
    """rows: [(Case, covers)]; tool: the writer the header line names"""
    with open(path, "w") as f:
        f.write(f"# {tool}: n P first count batch prec flags dir env covers(launch:prec/R/C/mode/nts/lp/vpt:SW)\n")
        for c, cov in rows:
            cv = ";".join("%d:%s:%d" % (i, "/".join(str(v) for v in d), sw) for i, d, sw in cov)
            f.write("\t".join(str(v) for v in (c.n, c.P, c.first, c.count, c.batch, c.prec, c.flags,
                                               "inv" if c.inverse else "fwd", env_text(c.env), cv)) + "\n")


def read_cases(path: str = CASES) -> list:
    rows = []
    with open(path) as f:
        for ln in f:
            if not ln.strip() or ln.startswith("#"):
                continue
            n, P, first, count, batch, prec, flags, direction, env, cv = ln.rstrip("\n").split("\t")
            assert direction in ("fwd", "inv"), ln
            e = () if env == "-" else tuple(tuple(kv.split("=", 1)) for kv in env.split(" "))
            cov = []
            for item in cv.split(";"):
                i, d, sw = item.split(":")
                cov.append((int(i), tuple(int(v) for v in d.split("/")), int(sw)))
            rows.append((Case(int(n), int(P), int(first), int(count), int(batch), int(prec), int(flags),
                              direction == "inv", e), tuple(cov)))
    return rows


def read_exceptions(path: str = EXCEPTIONS) -> dict:
    """{(descriptor, SW): reason}; a line: <descriptor> sw=<SW> : <reason>"""
    out = {}
    with open(path) as f:
        for ln in f:
            if not ln.strip() or ln.startswith("#"):
                continue
            head, _, reason = ln.strip().partition(" : ")
            d, _, sw = head.rpartition(" sw=")
            key = (parse_desc(d), int(sw))
            assert key not in out, ln
            out[key] = reason.strip()
    return out


# ---------------------------------------------------------------- search ---
def log2(x: int) -> int:
    return x.bit_length() - 1


def batches(n: int) -> list:
    return [1 << k for k in range(0, log2(min(MAX_VALUES // n, MAX_BATCH)) + 1)] if n <= MAX_VALUES else []


def try_case(case: Case, table: list):
    """The case's covers if it plans and passes the preflight, else None
    (the caller has set the environment)."""
    import pifft
    try:
        ids = launches(case)
    except pifft.PifftError:
        return None
    ps = [(table[k][1], table[k][2]) for k in ids if k >= 0]
    wil = any(table[k][3] & 8 for k in ids if k >= 0)
    if preflight(case, ps, wil):
        return None
    return covers(case, ids, table)


def default_grid():
    """Shapes of the untuned tier: every N up to 2^20, P up to 64 (P = 32 and
    64 plan tree launches only beyond the one-launch form), whole and
    one-worker ranges, every order, with and without a separate tree."""
    for prec in (32, 64):
        for logn in range(1, 21):
            n = 1 << logn
            for lp in range(0, min(logn, 6) + 1):
                P = 1 << lp
                for count, first in ((P, 0),) if P == 1 else ((P, 0), (1, 0), (1, P - 1)):
                    for order in ((NAT, SL, BR) if count == P else (SL, BR)):
                        for sep in ((0, SEP) if P > 1 else (0,)):
                            for b in batches(n):
                                yield n, P, first, count, b, prec, order | sep


def search_default(part: int, parts: int, table: list) -> dict:
    pool = {}
    with tuning(()):
        for k, shp in enumerate(default_grid()):
            if k % parts != part:
                continue
            for inverse in (False, True):
                case = Case(*shp, inverse, ())
                cov = try_case(case, table)
                if cov:
                    pool[case] = cov
    return pool


def directed(desc: tuple, sw: int, table: list) -> list:
    """Shapes that could make a plan launch the target, each with the tuning
    variables that could steer the planner there:
    (n, P, first, count, batch, flags, {name: value})."""
    prec, R, C, mode, nts, lp, vpt = desc
    sfx = str(prec)
    lr = log2(R)
    env = {"PIFFT_NT": str(nts), "PIFFT_MIN_WORKGROUPS": "1"}
    shapes = []

    def add(e, n, P, first, count, flags):
        for b in batches(n):
            shapes.append((n, P, first, count, b, flags, e))

    if mode in (0, 4):  # the single pass: M = R
        env["PIFFT_SINGLE_C" + sfx] = str(C)
        if lr > 14:
            env["PIFFT_SINGLE_MAX_LOG"] = str(lr)
        if vpt != 16:
            env["PIFFT_SINGLE_VPT"] = str(vpt)
        last = BR if mode == 4 else SL
        if sw in (0, 3):  # the only launch
            add(env, R, 1, 0, 1, BR if mode == 4 else NAT)
        if sw in (0, 2):  # behind a separate tree
            for P in (2, 4):
                add(env, R * P, P, 0, 1, last)
                add(env, R * P, P, 0, P, last)
                add(env, R * P, P, P - 1, 1, last | SEP)
        return shapes
    first_pass = mode in (1, 3, 11)
    for l2 in range(4, 12):  # the other pass of a two-pass plan
        logm = lr + l2
        if logm > 20:
            continue
        e = dict(env)
        e["PIFFT_RADIX_LOGS"] = f"{lr},{l2}" if first_pass else f"{l2},{lr}"
        if logm <= 14:
            e["PIFFT_SINGLE_MAX_LOG"] = str(logm - 1)
        e["PIFFT_COL_C" + sfx] = str(C)
        if C < 4:
            e["PIFFT_STRIDED_CMIN"] = str(C)
        if vpt == 32:
            e["PIFFT_VPT32"] = "1"
        m = 1 << logm
        sh = []
        if mode == 1:
            sh = [(m, 1, 0, 1, NAT), (m * 2, 2, 0, 2, SL), (m * 2, 2, 1, 1, SL | SEP)]
        elif mode == 3:
            e["PIFFT_FUSED_VPT"] = str(vpt)
            sh = [(m << lp, 1 << lp, 0, 1, SL), (m << lp, 1 << lp, (1 << lp) - 1, 1, SL)]
        elif mode in (2, 6):
            e["PIFFT_LAST_VPT"] = str(vpt)
            e["PIFFT_LAST_C"] = str(C)
            o = BR if mode == 6 else None
            sh = [(m, 1, 0, 1, NAT if o is None else o), (m * 2, 2, 1, 1, SL if o is None else o),
                  (m * 4, 4, 0, 4, SL if o is None else o)]
        elif mode == 10:  # behind a separate tree launch
            e["PIFFT_WIL_VPT"] = str(vpt)
            e["PIFFT_WIL_CMIN"] = str(C)
            e["PIFFT_WIL_FUSE"] = "0"
            e["PIFFT_WIL_SINGLE_MIN_LOG"] = "4"
            sh = [(m << q, 1 << q, 0, 1 << q, NAT) for q in range(1, 5)]
        elif mode == 11:
            P = 1 << lp
            if C % P:
                continue
            e["PIFFT_WIL_FUSE_J"] = str(C // P)
            e["PIFFT_WIL_FUSE_TILE"] = str(R * C)
            e["PIFFT_WIL_FUSE_VPT"] = str(vpt)
            e["PIFFT_WIL_SINGLE_MIN_LOG"] = "4"
            del e["PIFFT_RADIX_LOGS"], e["PIFFT_COL_C" + sfx]
            sh = [(m << lp, P, 0, P, NAT)]
        for shp in sh:
            add(e, *shp)
    if mode == 10:  # behind a fused first pass (MODE 11) of the registry: N = R1 R P
        for p2, R1, C1, m1, n1, lp1, v1 in table:
            if (p2, m1, n1) != (prec, 11, nts):
                continue
            e = dict(env)
            e.update({"PIFFT_WIL_FUSE_J": str(C1 >> lp1), "PIFFT_WIL_FUSE_TILE": str(R1 * C1),
                      "PIFFT_WIL_FUSE_VPT": str(v1), "PIFFT_WIL_VPT": str(vpt), "PIFFT_WIL_CMIN": str(C),
                      "PIFFT_COL_C" + sfx: str(C), "PIFFT_WIL_SINGLE_MIN_LOG": "4"})
            add(e, (R1 * R) << lp1, 1 << lp1, 0, 1 << lp1, NAT)
    if mode == 11 and C == 1 << lp:  # the one-launch form: the tile of C = P lines of R = M points
        e = dict(env)
        if R << lp > 8192:
            e["PIFFT_WIL_ONE_MAX"] = str(R << lp)
        add(e, R << lp, 1 << lp, 0, 1 << lp, NAT)
    return shapes


def search_target(args) -> dict:
    """Every valid case found for one open target at the fewest variables
    (with everything else those cases cover)."""
    (desc, sw), table, max_vars = args
    shapes = directed(desc, sw, table)
    found = {}
    names = sorted({k for s in shapes for k in s[6]})
    for size in range(1, min(max_vars, len(names)) + 1):
        for subset in itertools.combinations(names, size):
            by_env = {}
            for s in shapes:
                if all(k in s[6] for k in subset):
                    by_env.setdefault(tuple((k, s[6][k]) for k in subset), []).append(s)
            for e, group in by_env.items():
                with tuning(e):
                    for n, P, first, count, b, flags, _ in group:
                        case = Case(n, P, first, count, b, desc[0], flags, sw != 0, e)
                        if case in found:
                            continue
                        cov = try_case(case, table)
                        if cov and any(d == desc and s == sw for _, d, s in cov):
                            found[case] = cov
        if found:
            break
    # the smallest few are enough for the cover to choose from
    keep = sorted(found, key=lambda c: (c.n * c.batch, c))[:24]
    return {c: found[c] for c in keep}


def greedy(pool: dict, targets: set) -> tuple:
    """Tiers by number of variables; in a tier the case covering most open
    targets, then the smallest N batch, then the table's order."""
    open_ = set(targets)
    rows = []
    tiers = sorted({len(c.env) for c in pool})
    for tier in tiers:
        cand = {c: {(d, sw) for _, d, sw in cov} for c, cov in pool.items() if len(c.env) == tier}
        while True:
            best, gain = None, 0
            for c in sorted(cand, key=lambda c: (c.n * c.batch, c)):
                g = len(cand[c] & open_)
                if g > gain:
                    best, gain = c, g
            if not best:
                break
            rows.append((best, pool[best]))
            open_ -= cand.pop(best)
            cand = {c: t for c, t in cand.items() if t & open_}
    # drop what later choices made redundant, the cases of most variables first
    times = {}
    for _, cov in rows:
        for t in {(d, sw) for _, d, sw in cov}:
            times[t] = times.get(t, 0) + 1
    kept = []
    for c, cov in sorted(rows, key=lambda r: (-len(r[0].env), -r[0].n * r[0].batch, r[0])):
        if all(times[(d, sw)] > 1 for _, d, sw in cov):
            for t in {(d, sw) for _, d, sw in cov}:
                times[t] -= 1
        else:
            kept.append((c, cov))
    return kept, open_


def sort_key(row):
    c = row[0]
    return (c.prec, log2(c.n), c.batch, c.P, c.first, c.count, c.flags, c.inverse, c.env)


def case_id(case: Case) -> str:
    """The case's name in tests/test_gpu_instances.py (its pytest id and the label of its ACC line)."""
    env = "-" + ",".join(f"{k[len('PIFFT_'):]}={v}" for k, v in case.env) if case.env else ""
    return (f"f{case.prec}-2^{log2(case.n)}-P{case.P}-q{case.first}+{case.count}-fl{case.flags}-b{case.batch}-"
            f"{'inv' if case.inverse else 'fwd'}{env}")


def figures(log: str, per_line: int = 5, label: str = "ins", rows: list | None = None) -> str:
    """The ACC lines of a `pytest -s tests/test_gpu_instances.py` log as a
    table, one entry per case: the table's row (1-based, comment lines not
    counted), the rel-L2 and worst-bin ratios to the oracle's, and the
    worst-bin bound (the rel-L2 bound is 4 throughout).  label, rows: the ACC
    lines' label and the table of another file of cases (default: this one's)."""
    import re
    row_of = {case_id(c): k + 1 for k, (c, _) in enumerate(read_cases() if rows is None else rows)}
    got = {}
    with open(log) as f:
        for ln in f:
            m = re.search(r"ACC " + label + r" (\S+): .*?\(([\d.]+)x\) .*?\(([\d.]+)x\)\s+bounds 4x ([\d.]+)x", ln)
            if m:
                got[row_of[m.group(1)]] = "%4d %4.2f %4.2f %4.2f" % (row_of[m.group(1)], float(m.group(2)),
                                                                       float(m.group(3)), float(m.group(4)))
    assert sorted(got) == list(range(1, len(row_of) + 1)), "the log does not hold every case once"
    cells = [got[k] for k in sorted(got)]
    return "\n".join(" | ".join(cells[i:i + per_line]) for i in range(0, len(cells), per_line)) + "\n"


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--figures", metavar="LOG", help="print the ACC lines of a GPU run's log as a table, by row")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--max-vars", type=int, default=6, help="the most tuning variables of a case")
    ap.add_argument("--check", action="store_true", help="report the committed table's coverage, write nothing")
    args = ap.parse_args()
    if args.figures:
        sys.stdout.write(figures(args.figures))
        return 0
    import pifft
    t0 = time.time()
    table = [tuple(d) for d in pifft.instances()]
    targets = set(universe(table))
    n_inst = len(table)
    print(f"{n_inst} instances, {len(targets) - n_inst} twins")
    if args.check:
        rows = read_cases()
        got = {(d, sw) for _, cov in rows for _, d, sw in cov}
        exc = read_exceptions()
        print(f"{len(rows)} cases ({sum(1 for c, _ in rows if not c.env)} without tuning variables) cover "
              f"{sum(1 for t in got if t[1] == 0)} instances and {sum(1 for t in got if t[1])} twins; "
              f"{len(exc)} exceptions; {len(targets - got - set(exc))} neither")
        return 0
    pool = {}
    with ProcessPoolExecutor(max_workers=args.jobs) as ex:
        for part in ex.map(search_default, range(args.jobs), [args.jobs] * args.jobs, [table] * args.jobs):
            pool.update(part)
        done = {(d, sw) for cov in pool.values() for _, d, sw in cov}
        print(f"untuned plans: {len(pool)} valid cases reach {len(done & targets)} of {len(targets)} "
              f"({time.time() - t0:.0f} s)")
        todo = sorted(targets - done)
        for part in ex.map(search_target, [(t, table, args.max_vars) for t in todo], chunksize=4):
            pool.update(part)
    rows, open_ = greedy(pool, targets)
    rows.sort(key=sort_key)
    write_cases(CASES, rows)
    old = read_exceptions() if os.path.exists(EXCEPTIONS) else {}
    with open(EXCEPTIONS, "w") as f:
        f.write("# instances (sw=0) and twins (sw=1..3) no case of tests/golden/instance_cases.tsv launches under the\n"
                "# rules of tools/instance_cases.py: <descriptor> sw=<SW> : <reason>\n")
        for d, sw in sorted(open_):
            f.write(f"{fmt(d)} sw={sw} : {old.get((d, sw), 'REASON MISSING')}\n")
    got = targets - open_
    print(f"{len(rows)} cases ({sum(1 for c, _ in rows if not c.env)} without tuning variables) cover "
          f"{sum(1 for t in got if t[1] == 0)} of {n_inst} instances and {sum(1 for t in got if t[1])} of "
          f"{len(targets) - n_inst} twins; {len(open_)} exceptions; {time.time() - t0:.0f} s")
    return 0


if __name__ == "__main__":
    sys.exit(main())
