// cs87project-msolano2_amd/csrc/pifft_passes.hip -- one slice of the k_pass
// instantiations (compiled PIFFT_NPART times with -DPIFFT_PART=k, in parallel).
// Compiled a second time per part with -DPIFFT_TWINS, the same instance list
// expands to the slice's swapping twins (k_pass_sw, inverse plans) instead.
#include "pifft_kernels.h"
#include "pifft_table.h"

#if !defined(PIFFT_PART) || !defined(PIFFT_INC)
#error "compile with -DPIFFT_PART=<k> -DPIFFT_INC='\"pifft_instances_<k>.inc\"'"
#endif
#define PIFFT_CAT2(a, b) a##b
#define PIFFT_CAT(a, b) PIFFT_CAT2(a, b)

using namespace pifft;

#ifdef PIFFT_TWINS
// (instance, SW) -> its twin, or null where no inverse plan reaches it (twin_reachable)
template <typename T, int R, int C, int MODE, int NTS, int LP, int VPT, int SW>
const void* twin_fn() {
    if constexpr (SW != 0 && twin_reachable(MODE, C, LP, SW))
        return reinterpret_cast<const void*>(&k_pass_sw<T, R, C, MODE, NTS, LP, VPT, SW>);
    else
        return nullptr;
}
#define PIFFT_TWIN(T, PREC, R, C, MODE, NTS, LP, VPT, SLOT)                                   \
    TwinKernel {                                                                              \
        PREC, R, C, MODE, NTS, LP, VPT, twin_sw(MODE, SLOT),                                  \
            twin_fn<T, R, C, MODE, NTS, LP, VPT, twin_sw(MODE, SLOT)>()                       \
    }
// two slots per instance; the empty ones (fn == null) are dropped by the registry
#define PKV(T, PREC, R, C, MODE, NTS, LP, VPT) \
    PIFFT_TWIN(T, PREC, R, C, MODE, NTS, LP, VPT, 0), PIFFT_TWIN(T, PREC, R, C, MODE, NTS, LP, VPT, 1)
#define PK(T, PREC, R, C, MODE, NTS, LP) PKV(T, PREC, R, C, MODE, NTS, LP, 16)

namespace {
const TwinKernel kTwins[] = {
#include PIFFT_INC
};
}  // namespace

extern "C" const TwinKernel* PIFFT_CAT(pifft_twin_table_, PIFFT_PART)(int* n) {
    *n = (int)(sizeof(kTwins) / sizeof(kTwins[0]));
    return kTwins;
}
#else
#define PKV(T, PREC, R, C, MODE, NTS, LP, VPT)                                                          \
    PassKernel {                                                                                        \
        PREC, R, C, MODE, NTS, LP, reinterpret_cast<const void*>(&k_pass<T, R, C, MODE, NTS, LP, VPT>), \
            PassCfg<R, C, VPT>::NT, pass_lds_bytes<T, R, C, MODE, VPT>(), VPT                           \
    }
#define PK(T, PREC, R, C, MODE, NTS, LP) PKV(T, PREC, R, C, MODE, NTS, LP, 16)

namespace {
const PassKernel kTable[] = {
#include PIFFT_INC
};
}  // namespace

extern "C" const PassKernel* PIFFT_CAT(pifft_pass_table_, PIFFT_PART)(int* n) {
    *n = (int)(sizeof(kTable) / sizeof(kTable[0]));
    return kTable;
}
#endif  // PIFFT_TWINS
