// tests/native/twins_main.cpp -- the twin rule (csrc/pifft_table.h,
// twin_reachable) on a CPU, for tools/instance_cases.py and
// tests/test_instance_cases.py: which swapping twins (k_pass_sw, SW 1..3) of a
// k_pass instance an inverse plan can reach.  Host-only: no HIP, no libpifft.
//   usage: twins < descriptors
//   a descriptor, one per line: prec R C mode nts lp vpt
//   its answer: the descriptor, then twin_reachable at SW 1, 2 and 3 (0 / 1)
#include <stdio.h>

#include "../../cs87project-msolano2_amd/csrc/pifft_table.h"

int main() {
    int prec, R, C, mode, nts, lp, vpt;
    while (scanf("%d %d %d %d %d %d %d", &prec, &R, &C, &mode, &nts, &lp, &vpt) == 7)
        printf("%d %d %d %d %d %d %d : %d %d %d\n", prec, R, C, mode, nts, lp, vpt,
               (int)pifft::twin_reachable(mode, C, lp, 1), (int)pifft::twin_reachable(mode, C, lp, 2),
               (int)pifft::twin_reachable(mode, C, lp, 3));
    return 0;
}
