// tests/native/planner_main.cpp -- the planner's policy (csrc/pifft_planner.h,
// choose_plan) on a CPU, for tests/test_planner_native.py (host-only: no HIP,
// no GPU, no libpifft).  The registry find_pass searches is read from lists of
// instance descriptors (tests/golden/instances_*.txt: their union is the
// compiled registry, tests/test_instances.py).
//   usage: planner [--found] LIST... < shapes
//   a shape, one per line: n workers first count batch prec flags (valid ones:
//   the argument checks are pifft.hip's)
//   a plan: "plan wil=W ilv=I tree_tw=T fused=F : prec R C mode nts lp vpt ; ..."
//   a refused shape: "error <the planner's message>"
//   --found: after the plans, "found prec=.. R=.. ..." for every instance
//   find_pass returned while planning, sorted (the library's
//   pifft_instance_found: the set gen_instances.py must compile)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "../../cs87project-msolano2_amd/csrc/pifft_planner.h"
#include "../../include/pifft.h"

static std::vector<pifft::PassKernel> g_registry;
static std::vector<char> g_found;  // by registry index; empty while the lists are read

const pifft::PassKernel* pifft::find_pass(int prec, int R, int C, int mode, int nts, int lp, int vpt) {
    for (const PassKernel& k : g_registry)
        if (k.prec == prec && k.R == R && k.C == C && k.mode == mode && k.nts == nts && k.lp == lp && k.vpt == vpt) {
            if (!g_found.empty()) g_found[&k - g_registry.data()] = 1;
            return &k;
        }
    return nullptr;
}

int main(int argc, char** argv) {
    const bool found = argc > 1 && !strcmp(argv[1], "--found");
    if (argc < (found ? 3 : 2)) return 2;
    for (int a = found ? 2 : 1; a < argc; a++) {
        FILE* f = fopen(argv[a], "r");
        if (!f) return 2;
        pifft::PassKernel k{};
        while (fscanf(f, " prec=%d R=%d C=%d mode=%d nts=%d lp=%d vpt=%d", &k.prec, &k.R, &k.C, &k.mode, &k.nts, &k.lp,
                      &k.vpt) == 7) {
            // threads per workgroup, as the kernels' PassCfg: C lines of R points at Q values per thread
            const int q = k.R >= k.vpt ? k.vpt : (k.R >= 16 ? 16 : k.R);
            k.nt = k.C * k.R / q;
            if (!pifft::find_pass(k.prec, k.R, k.C, k.mode, k.nts, k.lp, k.vpt)) g_registry.push_back(k);
        }
        fclose(f);
    }
    g_found.assign(g_registry.size(), 0);
    unsigned long long n;
    unsigned workers, first, count, batch;
    int prec, flags;
    while (scanf("%llu %u %u %u %u %d %d", &n, &workers, &first, &count, &batch, &prec, &flags) == 7) {
        const int order = flags & ~(PIFFT_SEPARATE_TREE | PIFFT_INVERSE);
        const pifft::PlanShape s = pifft::plan_shape(n, workers, first, count, batch, prec, order == PIFFT_OUT_NATURAL,
                                                     order == PIFFT_OUT_BITREV, (flags & PIFFT_SEPARATE_TREE) != 0);
        pifft::PlanChoice ch;
        if (pifft::choose_plan(s, ch)) {
            printf("error %s\n", pifft::g_err.c_str());
            continue;
        }
        printf("plan wil=%d ilv=%d tree_tw=%d fused=%d :", ch.wil, ch.ilv, ch.tree_tw, ch.fused);
        for (size_t i = 0; i < ch.passes.size(); i++) {
            const pifft::PassKernel& k = *ch.passes[i];
            printf("%s %d %d %d %d %d %d %d", i ? " ;" : "", k.prec, k.R, k.C, k.mode, k.nts, k.lp, k.vpt);
        }
        printf("\n");
    }
    if (found) {
        std::vector<std::string> lines;
        for (size_t i = 0; i < g_registry.size(); i++) {
            const pifft::PassKernel& k = g_registry[i];
            char buf[128];
            snprintf(buf, sizeof buf, "prec=%d R=%d C=%d mode=%d nts=%d lp=%d vpt=%d", k.prec, k.R, k.C, k.mode, k.nts,
                     k.lp, k.vpt);
            if (g_found[i]) lines.push_back(buf);
        }
        std::sort(lines.begin(), lines.end());
        for (const std::string& l : lines) printf("found %s\n", l.c_str());
    }
    return 0;
}
