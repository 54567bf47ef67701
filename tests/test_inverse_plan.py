"""Inverse plans (PIFFT_INVERSE) without a device: dry runs only.

An inverse plan is the forward plan of the same arguments whose first launch
(reading the caller's input) and last launch (writing the caller's output)
are the swapping twins of the forward kernels.  So its description must equal
the forward plan's in every field but the flags and launch_fn (the twins are
kernel functions of their own), its launches must derive from the same
registry instances, and every twin an inverse plan needs must be compiled: no
"no inverse twin" error anywhere in the planner's domain.
"""
import ctypes

import pytest

import pifft

NAT, SL, BR, SEP, INV = pifft.OUT_NATURAL, pifft.OUT_SLICES, pifft.OUT_BITREV, pifft.SEPARATE_TREE, pifft.INVERSE


def combos(P):
    """(count, flags) of the issue's grid."""
    return [(P, NAT), (P, SL), (P, BR), (1, SL), (1, BR), (P, NAT | SEP), (1, SL | SEP)]


def check_pair(n, P, batch, prec, first, count, flags):
    try:
        fwd = pifft.dry_run(n, P, batch, prec, first=first, count=count, flags=flags)
    except pifft.PifftError as e:
        # a shape the forward planner itself refuses (the packed fp32 passes
        # have no bit-reversed form): the inverse answers the same, and never
        # with a missing twin
        with pytest.raises(pifft.PifftError) as ei:
            pifft.dry_run(n, P, batch, prec, first=first, count=count, flags=flags, inverse=True)
        assert str(ei.value) == str(e) and "twin" not in str(e)
        return False
    inv = pifft.dry_run(n, P, batch, prec, first=first, count=count, flags=flags, inverse=True)
    assert not fwd["inverse"] and inv["inverse"]
    same = {k: v for k, v in fwd.items() if k not in ("inverse", "launch_fn")}
    assert {k: v for k, v in inv.items() if k not in ("inverse", "launch_fn")} == same, (n, P, batch, prec, count, flags)
    assert len(inv["launch_fn"]) == len(fwd["launch_fn"])
    ids_f = pifft.dry_run_instances(n, P, batch, prec, first=first, count=count, flags=flags)
    ids_i = pifft.dry_run_instances(n, P, batch, prec, first=first, count=count, flags=flags, inverse=True)
    assert ids_i == ids_f, (n, P, batch, prec, count, flags)
    # flags | INVERSE spelled out equals inverse=True
    assert pifft.dry_run(n, P, batch, prec, first=first, count=count, flags=flags | INV) == inv
    return True


@pytest.mark.parametrize("prec", [pifft.F32, pifft.F64])
@pytest.mark.parametrize("batch", [1, 3])
def test_inverse_dry_run_equals_forward_over_the_grid(prec, batch):
    for logn in range(1, 25):
        n = 1 << logn
        for lp in range(0, 8):
            P = 1 << lp
            if P > n:
                continue
            for count, flags in combos(P):
                assert check_pair(n, P, batch, prec, 0, count, flags), (n, P, count, flags)


@pytest.mark.parametrize("prec,logn", [(pifft.F32, 27), (pifft.F32, 28), (pifft.F64, 28)])
def test_inverse_dry_run_large(prec, logn):
    n = 1 << logn
    for P in (1, 2, 8, 16):
        for count, flags in combos(P):
            ok = check_pair(n, P, 1, prec, 0, count, flags)
            assert ok or (prec == pifft.F32 and flags & BR), (P, count, flags)


@pytest.mark.parametrize("prec", [pifft.F32, pifft.F64])
def test_inverse_dry_run_2_32_one_worker_of_8(prec):
    assert check_pair(1 << 32, 8, 1, prec, 7, 1, SL)


def test_info_flags_carry_the_bit():
    info = pifft.PlanInfo()
    L = pifft.lib()
    assert L.pifft_plan_dry_run(1 << 20, 8, 0, 8, 1, pifft.F64, NAT | INV, ctypes.byref(info)) == 0
    assert info.flags == NAT | INV
    assert L.pifft_plan_dry_run(1 << 20, 8, 3, 1, 1, pifft.F32, SL | SEP | INV, ctypes.byref(info)) == 0
    assert info.flags == SL | SEP | INV
    assert L.pifft_plan_dry_run(1 << 20, 8, 0, 8, 1, pifft.F64, NAT, ctypes.byref(info)) == 0
    assert info.flags == NAT


def test_first_and_last_launch_are_kernels_of_their_own():
    # fp64 2^28, P = 1: three passes 1, 2, 2 -- forward launch_fn [0, 1, 2]
    # or [0, 1, 1] by radices; the inverse plan's last launch never shares a
    # function with the middle one
    fwd = pifft.dry_run(1 << 28, 1, 1, pifft.F64)
    inv = pifft.dry_run(1 << 28, 1, 1, pifft.F64, inverse=True)
    assert fwd["launch_mode"] == inv["launch_mode"] == [1, 2, 2]
    assert len(set(inv["launch_fn"])) == 3
    # a multi-launch tree (P = 32 slices, M = 1): in on the first, out on the second
    inv = pifft.dry_run(32, 32, 1, pifft.F64, flags=SL, inverse=True)
    assert inv["launch_kind"] == ["tree", "tree"] and inv["launch_fn"] == [0, 1]


@pytest.mark.parametrize("flags", [16, 16 | INV, 32, 3, 3 | INV, NAT | 64, -1])
def test_unknown_flag_bits_are_still_refused(flags):
    with pytest.raises(pifft.PifftError, match="unknown flags"):
        pifft.dry_run(1 << 10, 4, 1, pifft.F64, flags=flags)
    with pytest.raises(pifft.PifftError, match="unknown flags"):
        pifft.dry_run_instances(1 << 10, 4, 1, pifft.F64, flags=flags)


def test_inverse_keeps_the_order_rules():
    # natural order still needs every worker on the plan
    for flags in (NAT, NAT | INV):
        with pytest.raises(pifft.PifftError, match="unknown flags .*natural-order output needs all workers"):
            pifft.dry_run(1 << 10, 4, 1, pifft.F64, count=1, flags=flags)


def test_binding_and_header_agree_on_the_flag():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(pifft.HERE), "include", "pifft.h")).read()
    assert int(re.search(r"#define PIFFT_INVERSE (\d+)", hdr).group(1)) == pifft.INVERSE == 8
    assert int(re.search(r"#define PIFFT_ABI_VERSION (\d+)", hdr).group(1)) == 3
