// cs87project-msolano2_amd/csrc/pifft.hip -- libpifft.so: plan construction + C-ABI shim.
//
// Implements include/pifft.h.  The host side plans (the policy: pifft_planner.h) the reference's two stages
// (CPU.c:419-448 tree, CPU.c:463-478 cylinder) as a short list of kernel
// launches (pifft_kernels.h) over device buffers:
//
//   tree    : input (batch x N, HBM-resident)  -> Z (batch x count x N/P)
//   passes  : Z -> ... -> Z'   Stockham passes of the N/P-point local FFT,
//             each an LDS-resident R-point sub-FFT over C adjacent lines
//   [interleave: slice-major -> natural order, whole transform on one GPU]
//   [real plans: the N/2-point chain above plus one fix-up launch (create_real, pifft_real.h)]
//   [matrix plans: two such chains, rows and columns, with transposes between them (create_matrix, pifft_matrix.h)]
//   [chirp plans: any length N, two chains of M >= 2N - 1 around a pointwise product (create_chirp, pifft_chirp.h)]
//   [convolution plans: real rows times one filter, the two chains of a real transform around a fused pair kernel
//    (create_conv, pifft_conv.h)]
//
// Buffers ping-pong between the caller's output and one plan-owned workspace.
// Twiddles are host-built tables in HBM (w_R per pass, two-level w_M and w_N;
// the tree uses the reference's own omega(N,k) formula up to N = 2^22 so that
// its output is bit-identical to the reference's post-tree segment).
#ifndef _GNU_SOURCE
#define _GNU_SOURCE  // sincos (reference_omega_levels)
#endif
#include "pifft_chirp.h"
#include "pifft_conv.h"
#include "pifft_gather.h"
#include "pifft_kernels.h"
#include "pifft_matrix.h"
#include "pifft_planner.h"
#include "pifft_real.h"
#include "pifft_table.h"
#include "../../include/pifft.h"

#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <cxxabi.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

using namespace pifft;

namespace {

#define HIPCHK(expr)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) return fail("%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// Test-only fault injection for the multi-GPU error paths, which a one-GPU
// box cannot otherwise reach (tests/test_gpu_parity.py): PIFFT_FAULT=<site>
// (enable_peer, peer_copy, broadcast), read only under PIFFT_TUNING=1, makes
// that call fail as a HIP error would.
bool fault_at(const char* site) {
    if (!tuning_on()) return false;
    const char* s = getenv("PIFFT_FAULT");
    const size_t n = strlen(site);
    if (!s || strncmp(s, site, n)) return false;
    if (s[n] == '\0') return true;  // <site>: every time it is reached
    if (s[n] != ':') return false;
    // <site>:K -- only the K-th time it is reached under this setting (e.g.
    // peer_copy:3 fails the third copy, after two were enqueued)
    static std::mutex mu;
    static std::string last;
    static long count = 0;
    std::lock_guard<std::mutex> lk(mu);
    if (last != s) {
        last = s;
        count = 0;
    }
    return ++count == atol(s + n + 1);
}

// Timing events only time (pifft_execute_device_timed, pifft_profile_*,
// pifft_execute_group's stage timers): no system-scope fence when they are
// recorded, so a timed kernel does not pay an L2 write-back at its end (a
// bound stop event otherwise made C3's 44-us kernel read 50 us)
constexpr unsigned kTimingEventFlags = hipEventDisableSystemFence;


// 1-D grid for a grid-stride kernel of `total` items at 256 threads/block:
// capped so the launch's work-item count stays far below 2^32.
// PIFFT_STRIDE_GRID_MAX (tuning, tests): a smaller cap, so that a small launch
// makes second and later trips of its grid-stride loop (tests/test_gpu_aux.py)
constexpr int kStrideGridMax = 262144;
unsigned stride_grid(uint64_t total) {
    const uint64_t cap = (uint64_t)std::min(std::max(env_int("PIFFT_STRIDE_GRID_MAX", kStrideGridMax), 1), kStrideGridMax);
    const uint64_t blocks = (total + 255) / 256;
    return (unsigned)(blocks < cap ? (blocks ? blocks : 1) : cap);
}
uint32_t bitrev(uint32_t x, int m) { return m ? (__builtin_bitreverse32(x) >> (32 - m)) : 0u; }

// ---------------------------------------------------------------------------
// pass kernel instantiations (tables from the pifft_passes.hip parts)
// ---------------------------------------------------------------------------
}  // namespace
#define PIFFT_DECL_PART(k) extern "C" const PassKernel* pifft_pass_table_##k(int* n);
PIFFT_DECL_PART(0)
PIFFT_DECL_PART(1)
PIFFT_DECL_PART(2)
PIFFT_DECL_PART(3)
PIFFT_DECL_PART(4)
PIFFT_DECL_PART(5)
PIFFT_DECL_PART(6)
PIFFT_DECL_PART(7)
#define PIFFT_DECL_TWINS(k) extern "C" const TwinKernel* pifft_twin_table_##k(int* n);
PIFFT_DECL_TWINS(0)
PIFFT_DECL_TWINS(1)
PIFFT_DECL_TWINS(2)
PIFFT_DECL_TWINS(3)
PIFFT_DECL_TWINS(4)
PIFFT_DECL_TWINS(5)
PIFFT_DECL_TWINS(6)
PIFFT_DECL_TWINS(7)
namespace {
static_assert(PIFFT_NPART == 8, "update the part list");

const std::vector<PassKernel>& pass_kernels() {
    static const std::vector<PassKernel> all = [] {
        std::vector<PassKernel> v;
        const PassKernel* (*parts[])(int*) = {pifft_pass_table_0, pifft_pass_table_1, pifft_pass_table_2,
                                               pifft_pass_table_3, pifft_pass_table_4, pifft_pass_table_5,
                                               pifft_pass_table_6, pifft_pass_table_7};
        for (auto f : parts) {
            int n = 0;
            const PassKernel* t = f(&n);
            v.insert(v.end(), t, t + n);
        }
        return v;
    }();
    return all;
}

// every instance find_pass has returned in this process (pifft_instance_found):
// the planner probes instances to choose between plans, so the instances a
// plan depends on are those it found, launched or not (tests/test_instances.py)
std::atomic<unsigned char>* found_log() {
    static std::atomic<unsigned char>* f = new std::atomic<unsigned char>[pass_kernels().size()]();
    return f;
}

}  // namespace

// the planner's registry lookup (pifft_planner.h)
const PassKernel* pifft::find_pass(int prec, int R, int C, int mode, int nts, int lp, int vpt) {
    const auto& all = pass_kernels();
    for (size_t i = 0; i < all.size(); i++) {
        const PassKernel& k = all[i];
        if (k.prec == prec && k.R == R && k.C == C && k.mode == mode && k.nts == nts && k.lp == lp && k.vpt == vpt) {
            found_log()[i].store(1, std::memory_order_relaxed);  // (plans may be built on several host threads)
            return &k;
        }
    }
    return nullptr;
}

namespace {

// The swapping twins of the instances (inverse plans), a table of their own:
// the registry above, pifft_instance_* and the committed instance lists know
// the forward instances only.
const std::vector<TwinKernel>& twin_kernels() {
    static const std::vector<TwinKernel> all = [] {
        std::vector<TwinKernel> v;
        const TwinKernel* (*parts[])(int*) = {pifft_twin_table_0, pifft_twin_table_1, pifft_twin_table_2,
                                               pifft_twin_table_3, pifft_twin_table_4, pifft_twin_table_5,
                                               pifft_twin_table_6, pifft_twin_table_7};
        for (auto f : parts) {
            int n = 0;
            const TwinKernel* t = f(&n);
            for (int i = 0; i < n; i++)
                if (t[i].fn) v.push_back(t[i]);  // (empty slots: twins no inverse plan reaches)
        }
        return v;
    }();
    return all;
}

// the twin of forward instance k with swaps sw (1 in, 2 out, 3 both), or null
const TwinKernel* find_twin(const PassKernel& k, int sw) {
    for (const TwinKernel& t : twin_kernels())
        if (t.sw == sw && t.prec == k.prec && t.R == k.R && t.C == k.C && t.mode == k.mode && t.nts == k.nts &&
            t.lp == k.lp && t.vpt == k.vpt)
            return &t;
    return nullptr;
}

// The registry of the auxiliary kernels -- every kernel that is not a k_pass
// instance: the forward kernels (sw 0) and their swapping twins (inverse
// plans).  The one place this file names them: assemble_steps, interleave_fn,
// add_real_step, make_inverse and pifft_generate_device take their kernels
// from here (find_aux), so none can be launched without being listed, and
// pifft_aux_count / pifft_aux_desc / pifft_plan_dry_run_aux describe exactly
// what can be launched (tests/test_aux_cases.py, tests/test_gpu_aux.py).
// The one exception: the matrix plans' k_transpose, which build_matrix takes
// from the two-row table of its own in pifft_matrix.h (transpose_fn).
struct AuxKernel {
    int family, prec, L, sw;  // PIFFT_AUX_*; 32 / 64; tree levels (0: the family has none); 0 or the twin's swaps
    const void* fn;
};
#define PIFFT_AUX_TREE_ROWS(T, PREC, L)                                                            \
    {PIFFT_AUX_TREE, PREC, L, 0, (const void*)&k_tree<T, L>},                                      \
        {PIFFT_AUX_TREE, PREC, L, 1, (const void*)&k_tree_sw<T, L, 1>},                            \
        {PIFFT_AUX_TREE, PREC, L, 2, (const void*)&k_tree_sw<T, L, 2>},                            \
        {PIFFT_AUX_TREE, PREC, L, 3, (const void*)&k_tree_sw<T, L, 3>},                            \
        {PIFFT_AUX_TREE_WIL, PREC, L, 0, (const void*)&k_tree_wil<T, L>},                          \
        {PIFFT_AUX_TREE_WIL, PREC, L, 1, (const void*)&k_tree_wil_sw<T, L, 1>}
#define PIFFT_AUX_INTERLEAVE_ROWS(FAMILY, K, T, PREC) \
    {FAMILY, PREC, 0, 0, (const void*)&K<T>}, {FAMILY, PREC, 0, 2, (const void*)&K##_sw<T, 2>}
const AuxKernel kAux[] = {
    PIFFT_AUX_TREE_ROWS(double, 64, 1), PIFFT_AUX_TREE_ROWS(double, 64, 2), PIFFT_AUX_TREE_ROWS(double, 64, 3),
    PIFFT_AUX_TREE_ROWS(double, 64, 4), PIFFT_AUX_TREE_ROWS(float, 32, 1),  PIFFT_AUX_TREE_ROWS(float, 32, 2),
    PIFFT_AUX_TREE_ROWS(float, 32, 3),  PIFFT_AUX_TREE_ROWS(float, 32, 4),
    PIFFT_AUX_INTERLEAVE_ROWS(PIFFT_AUX_INTERLEAVE, k_interleave, double, 64),
    PIFFT_AUX_INTERLEAVE_ROWS(PIFFT_AUX_INTERLEAVE, k_interleave, float, 32),
    PIFFT_AUX_INTERLEAVE_ROWS(PIFFT_AUX_INTERLEAVE_TILE, k_interleave_tile, double, 64),
    PIFFT_AUX_INTERLEAVE_ROWS(PIFFT_AUX_INTERLEAVE_TILE, k_interleave_tile, float, 32),
    {PIFFT_AUX_C2R, 64, 0, 0, (const void*)&k_c2r_pre<double>},
    {PIFFT_AUX_R2C, 64, 0, 0, (const void*)&k_r2c_post<double>},
    {PIFFT_AUX_C2R, 32, 0, 0, (const void*)&k_c2r_pre<float>},
    {PIFFT_AUX_R2C, 32, 0, 0, (const void*)&k_r2c_post<float>},
    {PIFFT_AUX_GENERATE, 64, 0, 0, (const void*)&k_generate<double>},
    {PIFFT_AUX_GENERATE, 32, 0, 0, (const void*)&k_generate<float>},
};
#undef PIFFT_AUX_TREE_ROWS
#undef PIFFT_AUX_INTERLEAVE_ROWS
constexpr int kAuxCount = (int)(sizeof kAux / sizeof kAux[0]);

const AuxKernel* find_aux(int family, int prec, int L, int sw) {
    for (const AuxKernel& a : kAux)
        if (a.family == family && a.prec == prec && a.L == L && a.sw == sw) return &a;
    return nullptr;
}
// a forward kernel a plan cannot do without (every (family, precision, L) it asks for is listed above)
const void* aux_fn(int family, int prec, int L = 0) {
    const AuxKernel* a = find_aux(family, prec, L, 0);
    return a ? a->fn : nullptr;
}
// the registry index of a launch's kernel, or -1 (a k_pass instance or twin)
int aux_index(const void* fn) {
    for (int i = 0; i < kAuxCount; i++)
        if (kAux[i].fn == fn) return i;
    return -1;
}

// the twins of the tree and interleave kernels: (forward kernel, sw) -> twin
const void* find_aux_twin(const void* fn, int sw) {
    const int i = aux_index(fn);
    if (i < 0 || kAux[i].sw != 0) return nullptr;
    const AuxKernel* t = find_aux(kAux[i].family, kAux[i].prec, kAux[i].L, sw);
    return t ? t->fn : nullptr;
}

// ---------------------------------------------------------------------------
// plan
// ---------------------------------------------------------------------------
enum { STEP_TREE = 1, STEP_PASS = 2, STEP_INTERLEAVE = 3, STEP_TREE_PASS = 4, STEP_R2C_POST = 5, STEP_C2R_PRE = 6,
       STEP_TRANSPOSE = 7, STEP_CHIRP_PRE = 8, STEP_SPECTRUM_MUL = 9, STEP_CHIRP_POST = 10,
       STEP_CONV_PAD = 11, STEP_CONV_PAIR = 12, STEP_CONV_CROP = 13,
       STEP_CONV_FILTER = 14 };  // (14: of pifft_conv_set_filter only, never among a plan's launches)
// BUF_Z: a real plan's staging buffer, batch x N/2 values (create_real); a
// matrix plan's, batch x n0 x n1 values (build_matrix); a chirp plan's Z, and
// BUF_Y its Y, batch x M values each (build_chirp); a convolution plan's Z and
// Y, batch x H values each (a cyclic plan's Z: one row), and BUF_G its filter
// spectrum G, H + 1 values (build_conv)
enum { BUF_IN = 0, BUF_OUT = 1, BUF_W = 2, BUF_TA = 3, BUF_Z = 4, BUF_Y = 5, BUF_G = 6, NBUF = 7 };

// a step's twiddle tables as byte offsets into the plan's blob (kNoTable:
// none); materialise resolves them into pa / ta / ra once, launch_step never
constexpr size_t kNoTable = (size_t)-1;
struct StepTables {
    // a pass's w_R and two-level w_M; a real step's two-level w_N; a chirp step's two-level w_2N
    size_t r = kNoTable, lo = kNoTable, hi = kNoTable;
    size_t tree_direct = kNoTable, tree_lo = kNoTable, tree_hi = kNoTable;  // TreeTw
};

struct Step {
    int kind = 0;
    const void* fn = nullptr;
    const PassKernel* pk = nullptr;  // STEP_PASS / STEP_TREE_PASS: the instance
    dim3 grid, block;
    size_t lds = 0;
    int src = -1, dst = -2;  // -1 / -2: the chain element's input / output buffer
    uint64_t src_off = 0, dst_off = 0;  // elements
    PassArgs pa{};
    int nts = 0;  // STEP_PASS / STEP_TREE_PASS: the instance's streaming form
    TreeArgs ta{};
    uint64_t il_total = 0;
    uint32_t il_log_n = 0, il_log_p = 0;
    RealArgs ra{};  // STEP_R2C_POST / STEP_C2R_PRE
    TransposeArgs xa{};  // STEP_TRANSPOSE
    ChirpArgs ca{};  // STEP_CHIRP_PRE / STEP_SPECTRUM_MUL / STEP_CHIRP_POST
    ConvArgs va{};   // STEP_CONV_*
    StepTables tab;
    uint64_t bytes = 0;
};

}  // namespace

struct pifft_plan : pifft::PlanShape {  // (the shape it was planned for, pifft_planner.h)
    int device = 0, flags = 0;
    bool ilv = false;     // the last pass stores natural order itself (PassArgs::ilv_log)
    bool wil = false;     // worker-interleaved layout (PassArgs::wil, MODE | 8 passes)
    bool inverse = false;        // PIFFT_INVERSE: the first / last launch swap re/im (make_inverse)
    // pifft_plan_create_real: 0 complex, 1 R2C, 2 C2R.  Every field above and
    // below describes the inner N/2-point complex plan (n = real_n / 2)
    int real = 0;
    uint64_t real_n = 0;
    size_t bytes_z = 0;
    size_t rtw_bytes = 0;  // the fix-up step's two-level w_N table (in the blob, after the inner plan's tw_bytes)
    // pifft_plan_create_matrix: batch arrays of n0 x n1 values.  The shape
    // above is (n0 n1, one worker, batch); steps, tables and W are those of
    // the row and the column chain (build_matrix)
    bool matrix = false;
    uint64_t n0 = 0, n1 = 0;
    // pifft_plan_create_chirp: batch rows of chirp_n values, chirp_n no power
    // of two.  The shape above is (M, one worker, batch), M = chirp_length;
    // steps, tables and W are those of the forward and the inverse chain of M
    // (build_chirp); d_bt: Bt = DFT_M(b) / M, M values
    uint64_t chirp_n = 0;
    size_t bytes_y = 0, bytes_bt = 0;
    void* d_bt = nullptr;
    // pifft_plan_create_conv: batch rows of conv_n reals times one filter of
    // conv_taps reals, conv_len results per row, over transforms of conv_m
    // reals.  The shape above is (H = conv_m / 2, one worker, batch); steps,
    // tables and W are those of the forward and the inverse chain of H
    // (build_conv).  filter_steps: the launches of pifft_conv_set_filter, with
    // the forward chain planned for batch 1; conv_ready: G holds a filter
    bool conv = false, conv_ready = false;
    uint64_t conv_n = 0, conv_taps = 0, conv_len = 0, conv_m = 0;
    size_t bytes_g = 0;
    std::vector<Step> filter_steps;
    std::vector<Step> steps;
    int tree_steps = 0, npasses = 0;
    bool fused_tree = false;  // tree evaluated inside the first pass (STEP_TREE_PASS)
    std::vector<Step> tree_only;  // the tree stage alone, for pifft_tree_device
    std::vector<hipEvent_t> prof_ev;  // pifft_profile_*: per recorded execution, a start and a stop per timed launch
#ifdef PIFFT_WG_CLOCK
    unsigned long long* dbg_clk = nullptr;  // pifft_debug_wg_clock: the clocked launch's words (diagnostics build)
#endif
    int prof_steps = 0, prof_used = 0, prof_mode = 0;
    int radix[8] = {0}, lines[8] = {0}, vpt[8] = {0};
    void* buf[NBUF] = {nullptr};
    size_t bytes_w = 0, bytes_ta = 0;
    void* d_tw = nullptr;
    size_t tw_bytes = 0;
    hipStream_t stream = nullptr;
    std::vector<hipEvent_t> ev;  // 2 per launch: its start and stop (launch_steps)
    hipEvent_t sev[3] = {nullptr, nullptr, nullptr};  // stage markers: start, end of stage 1, end of stage 2
    void* d_hin = nullptr;   // pifft_execute's staging copies
    void* d_hout = nullptr;
    void* d_gather = nullptr;  // pifft_allgather: every worker's slices on this plan's device
    std::vector<char> host_tmp;
    std::vector<int> peer_on;  // devices this plan's device has peer access to (pifft_allgather)
    std::vector<hipStream_t> gst;  // pifft_allgather: one copy stream per source plan
    std::vector<hipEvent_t> gdone;  // ... and its completion event
    hipEvent_t gev[2] = {nullptr, nullptr};  // gather start / end on `stream`
};

namespace {

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (dev < 0) return;  // dry-run plans touch no device
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// Host twiddle tables, appended to one blob (offsets 256-B aligned).
struct TableBuilder {
    std::vector<char> blob;
    size_t esz;
    bool size_only = false;  // a dry run: the blob's layout and size only (no memory, no values)
    size_t sized = 0;        // the blob's size in a size_only run
    explicit TableBuilder(size_t e) : esz(e) {}
    size_t size() const { return size_only ? sized : blob.size(); }
    void grow_to(size_t bytes) {
        if (size_only) sized = bytes;
        else blob.resize(bytes);
    }
    size_t align() {
        size_t off = (size() + 255) & ~(size_t)255;
        grow_to(off);
        return off;
    }
    void put(double re, double im) {
        size_t o = blob.size();
        blob.resize(o + esz);
        if (esz == 16) {
            double v[2] = {re, im};
            memcpy(&blob[o], v, 16);
        } else {
            float v[2] = {(float)re, (float)im};
            memcpy(&blob[o], v, 8);
        }
    }
    // w_L^(e*stride), e < count, accurate (long double) -- the Stockham tables
    size_t roots(uint64_t L, uint64_t count, uint64_t stride) {
        size_t off = align();
        if (size_only) {
            grow_to(off + count * esz);
            return off;
        }
        const long double two_pi = 6.283185307179586476925286766559005768L;
        for (uint64_t e = 0; e < count; e++) {
            const uint64_t x = (e * stride) % L;
            const long double ang = two_pi * ((long double)x / (long double)L);
            put((double)cosl(ang), (double)(-sinl(ang)));
        }
        return off;
    }
    // omega(N,k) with the reference's own formula (CPU.c:644-651), packed by
    // tree level (TreeTw::direct): level t < levels holds omega(N, k 2^t),
    // k < N >> (t+1), at N - (N >> t) + k (level 0 = every k < N/2)
    size_t reference_omega_levels(uint64_t N, int levels) {
        size_t off = align();
        if (size_only) {
            grow_to(off + (N - (N >> (levels > 0 ? levels : 1))) * esz);
            return off;
        }
        // gcc -O1 and up folds the reference's cos()/sin() pair into one glibc
        // sincos() call; glibc's sincos and its separate cos/sin disagree in
        // the last fp64 bit for ~1e-3 of the angles (43 of 2^15 at N=2^16).
        // The reference build the fixtures pin (-O2) is the sincos one, so the
        // table is built the same way (clang keeps the pair separate).
        for (uint64_t k = 0; k < N / 2; k++) {
            double s, c;
            sincos(2.0 * M_PI / (double)N * (double)k, &s, &c);
            put(c, -s);
        }
        // the higher levels: byte copies of level-0 entries k 2^t
        blob.resize(off + (N - (N >> (levels > 0 ? levels : 1))) * esz);
        for (int t = 1; t < levels; t++) {
            const uint64_t base = N - (N >> t);
            for (uint64_t k = 0; k < (N >> (t + 1)); k++)
                memcpy(&blob[off + (base + k) * esz], &blob[off + (k << t) * esz], esz);
        }
        return off;
    }
};

struct TwoLevel {
    size_t lo = kNoTable, hi = kNoTable;
    uint32_t h = 0;
};

TwoLevel two_level(TableBuilder& tb, uint64_t L) {
    TwoLevel t;
    const int logl = ilog2u(L);
    t.h = (uint32_t)((logl + 1) / 2);
    t.lo = tb.roots(L, 1ull << t.h, 1);
    t.hi = tb.roots(L, (L >> t.h) ? (L >> t.h) : 1, 1ull << t.h);
    return t;
}

// the same for an L that is no power of two (a chirp plan's w_2N): 2^h ~ sqrt L
// entries of w_L^e, then ceil(L / 2^h) of w_L^(e 2^h)
TwoLevel two_level_any(TableBuilder& tb, uint64_t L) {
    TwoLevel t;
    t.h = (uint32_t)((ilog2u(L - 1) + 2) / 2);
    t.lo = tb.roots(L, 1ull << t.h, 1);
    t.hi = tb.roots(L, (L + (1ull << t.h) - 1) >> t.h, 1ull << t.h);
    return t;
}

// slice-major -> natural order: k_interleave_tile (LDS tile of all P slices,
// P <= 2048) from P = 2^5 at fp64 and P = 2 at fp32, else k_interleave (one
// thread per output element, any P); profiles/r02_interleave_ab.log
bool interleave_tiled(int prec, int lp, uint64_t n) {
    const int lo = env_int(prec == 64 ? "PIFFT_INTERLEAVE_TILE_MIN64" : "PIFFT_INTERLEAVE_TILE_MIN32", prec == 64 ? 5 : 1);
    return lo > 0 && lp >= lo && lp <= 11 && n >= (uint64_t)IL_TILE;
}
const void* interleave_fn(int prec, int lp, uint64_t n) {
    return aux_fn(interleave_tiled(prec, lp, n) ? PIFFT_AUX_INTERLEAVE_TILE : PIFFT_AUX_INTERLEAVE, prec);
}
uint64_t interleave_threads(uint64_t total, int lp, int prec, uint64_t n) {
    return interleave_tiled(prec, lp, n) ? (total / IL_TILE) * 256 : total;
}

void release(pifft_plan* p) {
    if (!p) return;
    DeviceGuard g(p->device);
    for (int b = BUF_W; b < NBUF; b++)
        if (p->buf[b]) (void)hipFree(p->buf[b]);
    if (p->d_tw) (void)hipFree(p->d_tw);
    if (p->d_bt) (void)hipFree(p->d_bt);
    if (p->d_hin) (void)hipFree(p->d_hin);
    if (p->d_hout) (void)hipFree(p->d_hout);
    if (p->d_gather) (void)hipFree(p->d_gather);
    for (auto st : p->gst) (void)hipStreamDestroy(st);
    for (auto e : p->gdone) (void)hipEventDestroy(e);
    for (auto e : p->gev)
        if (e) (void)hipEventDestroy(e);
    for (auto e : p->ev) (void)hipEventDestroy(e);
    for (auto e : p->sev)
        if (e) (void)hipEventDestroy(e);
    for (auto e : p->prof_ev) (void)hipEventDestroy(e);
    if (p->stream) (void)hipStreamDestroy(p->stream);
    delete p;
}


// Step 2 of a plan, the table layout: where each twiddle table choose_plan's
// choice needs sits in the plan's one blob (offsets only; the builder fills
// in the values unless it is size_only).
struct TableLayout {
    size_t tree_direct = kNoTable;  // the reference-formula tree table
    TwoLevel tree2;                 // two-level w_N (the tree)
    std::vector<size_t> tw_r;       // per pass: w_R
    TwoLevel pass2;                 // two-level w_M (plans of >= 2 passes)
};

TableLayout layout_tables(const PlanShape& s, const PlanChoice& ch, TableBuilder& tb) {
    TableLayout tl;
    // --- tree tables (w_N) ---
    if (ch.tree_tw == TREE_TW_DIRECT || ch.tree_tw == TREE_TW_WIL_FACTORED)
        tl.tree_direct = tb.reference_omega_levels(s.n, s.lp);
    if (ch.tree_tw == TREE_TW_FACTORED || ch.tree_tw == TREE_TW_WIL_FACTORED) tl.tree2 = two_level(tb, s.n);
    // --- pass tables ---
    tl.tw_r.resize(ch.passes.size());
    for (size_t i = 0; i < ch.passes.size(); i++) {
        size_t found = kNoTable;
        for (size_t j = 0; j < i; j++)
            if (ch.passes[j]->R == ch.passes[i]->R) found = tl.tw_r[j];
        tl.tw_r[i] = (found != kNoTable) ? found : tb.roots(ch.passes[i]->R, ch.passes[i]->R, 1);
    }
    if (ch.passes.size() > 1) tl.pass2 = two_level(tb, s.m);  // (every worker-interleaved plan has >= 2 passes)
    tb.align();
    return tl;
}

// Step 3, the launches: [tree] [passes] [interleave] over the ping-pong
// buffers, every argument but the device pointers (tables are offsets into
// the blob, Step::tab).  A dry run ends here.
int assemble_steps(pifft_plan* p, const PlanChoice& ch, const TableLayout& tl) {
    const size_t esz = p->esz;
    const uint64_t ntrans = (uint64_t)p->batch * p->nq;  // local transforms
    const size_t npass = ch.passes.size();
    const bool need_tree = p->P > 1;
    const bool fused = ch.fused != FUSED_NONE;
    p->wil = ch.wil;
    p->ilv = ch.ilv;
    p->fused_tree = fused;
    TreeTw ttw{};
    if (need_tree) {
        ttw.h = tl.tree2.h;
        ttw.log_n = (uint32_t)p->log_n;
    }
    // the tree's twiddles: the reference table where the plan has one; the
    // worker-interleaved plan's own tree (its k_tree_wil launch or its fused
    // first pass) the two-level one from 2^21 values up (TREE_TW_WIL_FACTORED)
    auto tree_tables = [&](Step& s, bool wil) {
        const bool direct = tl.tree_direct != kNoTable && !(wil && ch.tree_tw == TREE_TW_WIL_FACTORED);
        s.tab.tree_direct = direct ? tl.tree_direct : kNoTable;
        s.tab.tree_lo = direct ? kNoTable : tl.tree2.lo;
        s.tab.tree_hi = direct ? kNoTable : tl.tree2.hi;
    };

    // --- chain: [tree] [passes] [interleave]; an element's launches share its buffers ---
    std::vector<std::vector<Step>> chain;
    const uint64_t M = p->m;
    if (need_tree) {
        std::vector<Step> e;
        // ceil(log2 P / 4) launches of up to 4 levels each; in place over
        // one position-space buffer between launches (see k_tree)
        const int nl = (p->lp + 3) / 4;
        // number of level-t blocks (P >> t workers each) holding a requested worker
        auto blocks_needed = [&](int t) -> uint64_t {
            const uint64_t w = (uint64_t)p->P >> t;
            return ((uint64_t)p->q0 + p->nq - 1) / w - (uint64_t)p->q0 / w + 1;
        };
        int t0 = 0;
        for (int l = 0; l < nl; l++) {
            const int L = (p->lp - t0 + (nl - l) - 1) / (nl - l);  // spread levels evenly
            const bool first = (l == 0), last = (l == nl - 1);
            Step s;
            s.kind = STEP_TREE;
            s.fn = aux_fn(PIFFT_AUX_TREE, p->prec, L);  // (1 <= L <= 4: the registry holds every one)
            s.src = first ? -1 : BUF_TA;  // -1: chain input
            s.dst = last ? -2 : BUF_TA;   // -2: chain output (slice-major)
            s.ta.tw = ttw;
            tree_tables(s, false);
            s.ta.in_bstride = p->n;
            s.ta.out_bstride = last ? (uint64_t)p->nq * M : p->n;
            s.ta.out_shift = last ? -(int64_t)((uint64_t)p->q0 * M) : 0;
            s.ta.total = (uint64_t)p->batch * (p->n >> L);
            s.ta.log_n = (uint32_t)p->log_n;
            s.ta.log_p = (uint32_t)p->lp;
            s.ta.t0 = (uint32_t)t0;
            s.ta.q0 = p->q0;
            s.ta.nq = p->nq;
            s.block = dim3(256);
            s.grid = dim3(stride_grid(s.ta.total / (uint64_t)std::max(1, env_int("PIFFT_TREE_GRID_DIV", 1))));
            s.bytes = (uint64_t)p->batch * esz *
                      (blocks_needed(t0) * (p->n >> t0) + blocks_needed(t0 + L) * (p->n >> (t0 + L)));
            e.push_back(s);
            t0 += L;
        }
        if (nl > 1) p->bytes_ta = (size_t)p->batch * p->n * esz;
        // the stand-alone tree (pifft_tree_device) reads d_in and writes d_seg
        // (slice-major, always)
        for (Step t : e) {
            if (t.src == -1) t.src = BUF_IN;
            if (t.dst == -2) t.dst = BUF_OUT;
            p->tree_only.push_back(t);
        }
        if (p->wil && p->lp <= 4) {  // one launch over all workers: the passes' interleaved layout
            Step& t = e.back();
            t.fn = aux_fn(PIFFT_AUX_TREE_WIL, p->prec, p->lp);
            tree_tables(t, true);
            t.ta.out_bstride = p->n;
            t.lds = (size_t)tree_wil_pad(256u << p->lp) * esz;
        }
        if (!fused) {
            p->tree_steps = (int)e.size();
            chain.push_back(e);
        }
    }
    uint64_t ns = 1;
    p->npasses = (int)npass;
    for (size_t i = 0; i < npass; i++) {
        const bool fuse_here = (i == 0 && fused);
        const bool last_pass = i + 1 == npass && npass > 1;
        const PassKernel* k = ch.passes[i];
        Step s;
        s.kind = fuse_here ? STEP_TREE_PASS : STEP_PASS;
        s.fn = k->fn;
        s.pk = k;
        s.nts = k->nts;
        const int logr = ilog2u((uint64_t)k->R);
        s.tab.r = tl.tw_r[i];
        s.tab.lo = tl.pass2.lo;
        s.tab.hi = tl.pass2.hi;
        s.pa.tw_h = tl.pass2.h;
        s.pa.in_bstride = (i == 0 && (!need_tree || fuse_here)) ? p->n : M;
        if (fuse_here) {
            s.pa.tree = ttw;
            tree_tables(s, p->wil);
            s.pa.worker = p->q0;
            s.pa.log_nq = (uint32_t)ilog2u(p->nq);
        }
        s.pa.out_bstride = M;
        s.pa.nlines = ntrans * (M >> logr);
        s.pa.log_lb = (uint32_t)(p->log_m - logr);
        s.pa.log_ns = (uint32_t)ilog2u(ns);
        s.pa.tw_shift = (uint32_t)(p->log_m - ilog2u(ns) - logr);
        s.pa.log_xg = (uint32_t)env_int((k->mode & 3) == 0 ? "PIFFT_XCD_GROUP_SINGLE" : "PIFFT_XCD_GROUP",
                                        (k->mode & 3) == 0 ? 0 : 2);
        if (last_pass) s.pa.log_xg = (uint32_t)env_int("PIFFT_LAST_XCD_GROUP", (int)s.pa.log_xg);
        if (p->wil) {
            s.pa.wil = (uint32_t)p->lp;
            s.pa.wbrev = (i + 1 == npass) ? 1u : 0u;  // the last pass: natural order
            s.pa.in_bstride = s.pa.out_bstride = p->n;  // a transform's P interleaved workers
        }
        if (p->ilv && i + 1 == npass) {
            s.pa.ilv_log = (uint32_t)p->lp;
            s.pa.out_bstride = p->n;
            s.pa.log_xg = std::max<uint32_t>(s.pa.log_xg, (uint32_t)env_int("PIFFT_ILV_XCD_GROUP", p->lp));
        }
        s.block = dim3((unsigned)k->nt);
        s.grid = dim3((unsigned)((s.pa.nlines + (uint64_t)k->C - 1) / (uint64_t)k->C));  // (< 2^32 work-items: choose_plan)
        s.lds = (size_t)k->lds_bytes;
        // (a one-worker fused pass reads every leaf of its worker's transform:
        // N per worker; the all-worker one, MODE 11, each leaf once)
        s.bytes = (!fuse_here || p->wil) ? 2 * ntrans * M * esz : (uint64_t)p->batch * p->nq * (p->n + M) * esz;
        if (i < 8) {
            p->radix[i] = k->R;
            p->lines[i] = k->C;
            p->vpt[i] = k->vpt;
        }
        ns *= (uint64_t)k->R;
        chain.push_back({s});
    }
    if (p->natural && p->P > 1 && !p->ilv && !p->wil) {
        Step s;
        s.kind = STEP_INTERLEAVE;
        s.fn = interleave_fn(p->prec, p->lp, p->n);
        s.il_total = (uint64_t)p->batch * p->n;
        s.il_log_n = (uint32_t)p->log_n;
        s.il_log_p = (uint32_t)p->lp;
        s.block = dim3(256);
        s.grid = dim3(stride_grid(interleave_threads(s.il_total, p->lp, p->prec, p->n)));
        s.bytes = 2 * s.il_total * esz;
        chain.push_back({s});
    }
    if (chain.empty()) return fail("empty plan");
    // destinations, backwards: last -> OUT, then W, OUT, W, ...
    std::vector<int> dst(chain.size());
    for (size_t i = chain.size(); i-- > 0;) dst[i] = ((chain.size() - 1 - i) % 2 == 0) ? BUF_OUT : BUF_W;
    bool need_w = false;
    for (size_t i = 0; i < chain.size(); i++) {
        const int src = (i == 0) ? BUF_IN : dst[i - 1];
        if (dst[i] == BUF_W || src == BUF_W) need_w = true;
        for (auto& s : chain[i]) {
            if (s.src == -1) s.src = src;
            if (s.dst == -2) s.dst = dst[i];
            p->steps.push_back(s);
        }
    }
    if (p->steps.size() > 4096) return fail("plan too large (%zu launches)", p->steps.size());
    // Padded workspace rows (PassArgs::in_pad / out_pad): where one k_pass
    // writes W and a later pass (BM 2) reads it, W's rows are spread by
    // w_pad elements each, so their offsets no longer coincide with the
    // caller's output rows that the same passes read or write.  Measured on
    // MI355X over fresh (W, output) allocation pairs (tools/probe_wpad.py,
    // profiles/r02_wpad.log): C4 fp64 2^28 4.88 -> 4.73 ms mean (worst 5.03
    // -> 4.82), fp32 2^28 3.22 -> 3.19 ms, with 16 KiB + 256 B per row;
    // 1 MiB + 256 B ties at fp64 and loses 4 % at fp32.  Only for W >= 2 GiB:
    // at 512 MiB (fp64 2^25, the worker of 8 at 2^28) padding cost 1.5-2.5 %,
    // at 1 GiB it ties, at 2 GiB (the worker of 2 at 2^28, of 8 at 2^30) it
    // gains ~0.5 % (profiles/r02_wpad.log, tools/gpu_wpad_shapes.sh).
    uint64_t w_tr = M;  // elements per transform in W
    const uint64_t w_pad = (uint64_t)env_int("PIFFT_W_PAD", (int)((16384 + 256) / esz));
    const uint64_t w_min = (uint64_t)env_int("PIFFT_W_PAD_MIN_MIB", 2048) << 20;
    if (w_pad && !p->wil && (uint64_t)p->batch * p->nq * M * esz >= w_min) {
        for (size_t i = 0; i + 1 < p->steps.size(); i++) {
            Step& a = p->steps[i];
            Step& b = p->steps[i + 1];
            if (a.dst != b.src || a.dst != BUF_W || (a.kind != STEP_PASS && a.kind != STEP_TREE_PASS) ||
                b.kind != STEP_PASS || b.pa.log_ns == 0 || a.pa.ilv_log)
                continue;
            const uint64_t rows = M >> b.pa.log_lb;  // the reading pass's radix
            const uint64_t tr = M + rows * w_pad;
            const uint32_t logr_a = (uint32_t)(p->log_m - a.pa.log_lb);  // the writing pass's radix
            a.pa.out_pad = b.pa.in_pad = (uint32_t)w_pad;
            a.pa.out_pad_log = b.pa.log_lb - logr_a;
            a.pa.out_bstride = b.pa.in_bstride = tr;
            w_tr = std::max(w_tr, tr);
        }
    }
    p->bytes_w = need_w ? (size_t)p->batch * p->nq * w_tr * esz : 0;
    return 0;
}

// the one added launch of a real plan (create_real), after the inner chain is
// final: its w_N^k table, k <= N/4, two-level at every size -- 2^h ~ sqrt N
// entries per level (256 KiB each at fp64 2^28), against N/4 + 1 of a direct
// table -- joins the plan's blob
void add_real_step(pifft_plan* p, TableBuilder& tb, uint64_t n, bool c2r) {
    const uint64_t H = n / 2;
    p->real = c2r ? 2 : 1;
    p->real_n = n;
    p->bytes_z = (size_t)p->batch * H * p->esz;
    const size_t before = tb.size();
    const TwoLevel tw = two_level(tb, n);
    tb.align();
    p->rtw_bytes = tb.size() - before;
    Step s;
    s.kind = c2r ? STEP_C2R_PRE : STEP_R2C_POST;
    s.fn = aux_fn(c2r ? PIFFT_AUX_C2R : PIFFT_AUX_R2C, p->prec);
    s.tab.lo = tw.lo;
    s.tab.hi = tw.hi;
    s.ra.tw_h = tw.h;
    s.ra.batch = p->batch;
    s.ra.h = H;
    s.ra.units = p->prec == PIFFT_F64 ? real_units<double>(H) : real_units<float>(H);
    s.block = dim3(256);
    s.grid = dim3(stride_grid((uint64_t)p->batch * s.ra.units));
    const uint64_t threads = (uint64_t)s.grid.x * 256;
    s.ra.step_rows = threads / s.ra.units;
    s.ra.step_units = threads % s.ra.units;
    s.bytes = (uint64_t)p->batch * (2 * H + 1) * p->esz;
    if (c2r) {
        s.src = BUF_IN;
        s.dst = BUF_Z;
        for (Step& t : p->steps)
            if (t.src == BUF_IN) t.src = BUF_Z;
        p->steps.insert(p->steps.begin(), s);
    } else {
        for (Step& t : p->steps) {
            if (t.src == BUF_OUT) t.src = BUF_Z;
            if (t.dst == BUF_OUT) t.dst = BUF_Z;
        }
        s.src = BUF_Z;
        s.dst = BUF_OUT;
        p->steps.push_back(s);
    }
    p->tree_only.clear();  // (pifft_tree_device refuses real plans)
}

// Step 4, real (non-dry) plans only: the table blob on the device and every
// step's offsets resolved to pointers into it, the plan's buffers, stream and
// events, and the LDS attribute of the kernels the final steps launch.
int materialise(pifft_plan* p, const TableBuilder& tb) {
    HIPCHK(hipMalloc(&p->d_tw, p->tw_bytes + p->rtw_bytes));
    if (p->bytes_bt) HIPCHK(hipMalloc(&p->d_bt, p->bytes_bt));
    if (p->bytes_g) HIPCHK(hipMalloc(&p->buf[BUF_G], p->bytes_g));
    if (!tb.blob.empty()) HIPCHK(hipMemcpy(p->d_tw, tb.blob.data(), tb.blob.size(), hipMemcpyHostToDevice));
    auto at = [&](size_t off) { return off == kNoTable ? nullptr : (const void*)((const char*)p->d_tw + off); };
    auto resolve = [&](Step& s) {
        if (s.kind == STEP_TRANSPOSE) return;  // (no table, static LDS)
        if (s.kind >= STEP_CONV_PAD) {
            s.va.tw_lo = at(s.tab.lo), s.va.tw_hi = at(s.tab.hi), s.va.g = p->buf[BUF_G];
            return;
        }
        if (s.kind >= STEP_CHIRP_PRE) {
            s.ca.tw_lo = at(s.tab.lo), s.ca.tw_hi = at(s.tab.hi), s.ca.bt = p->d_bt;
            return;
        }
        TreeTw& tree = s.kind == STEP_TREE ? s.ta.tw : s.pa.tree;
        tree.direct = at(s.tab.tree_direct), tree.lo = at(s.tab.tree_lo), tree.hi = at(s.tab.tree_hi);
        if (s.kind == STEP_R2C_POST || s.kind == STEP_C2R_PRE) s.ra.tw_lo = at(s.tab.lo), s.ra.tw_hi = at(s.tab.hi);
        else s.pa.tw_r = at(s.tab.r), s.pa.tw_lo = at(s.tab.lo), s.pa.tw_hi = at(s.tab.hi);
        if (s.lds > 65536) (void)hipFuncSetAttribute(s.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s.lds);
    };
    for (Step& s : p->steps) resolve(s);
    for (Step& s : p->tree_only) resolve(s);
    for (Step& s : p->filter_steps) resolve(s);
    // tuning knob (tools/probe_place.py): hipExtMallocWithFlags flags for the
    // ping-pong workspace, e.g. 4 = hipDeviceMallocContiguous
    const int w_flags = env_int("PIFFT_W_MALLOC_FLAGS", 0);
    if (p->bytes_w)
        HIPCHK(w_flags ? hipExtMallocWithFlags(&p->buf[BUF_W], p->bytes_w, (unsigned)w_flags)
                       : hipMalloc(&p->buf[BUF_W], p->bytes_w));
    if (p->bytes_ta) HIPCHK(hipMalloc(&p->buf[BUF_TA], p->bytes_ta));
    if (p->bytes_z) HIPCHK(hipMalloc(&p->buf[BUF_Z], p->bytes_z));
    if (p->bytes_y) HIPCHK(hipMalloc(&p->buf[BUF_Y], p->bytes_y));
    HIPCHK(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
    p->ev.resize(2 * p->steps.size());
    for (auto& e : p->ev) HIPCHK(hipEventCreateWithFlags(&e, kTimingEventFlags));
    for (auto& e : p->sev) HIPCHK(hipEventCreateWithFlags(&e, kTimingEventFlags));
    return 0;
}

// PIFFT_INVERSE: IDFT(x) = swap(DFT(swap(x))), swap(a + bi) = b + ai, for the
// whole linear transform (tree, local FFT, any output order).  The plan is the
// forward plan build_plan made; the one launch that reads the caller's input
// becomes its twin swapping what it loads, the one launch that writes the
// caller's output its twin swapping what it stores (one launch: both).  No
// launch, byte or table more; the result equals swap(forward(swap(x))) bit
// for bit.  Step::pk keeps the forward instance the twin derives from.
int make_inverse(pifft_plan* p) {
    if (p->steps.empty()) return fail("empty plan");
    const size_t last = p->steps.size() - 1;
    if (p->steps[0].src != BUF_IN || p->steps[last].dst != BUF_OUT) return fail("inverse plan: unexpected buffer chain");
    for (size_t i = 1; i <= last; i++)
        if (p->steps[i].src == BUF_IN) return fail("inverse plan: launch %zu reads the input again", i);
    for (size_t i = 0; i <= last; i++) {
        const int sw = (i == 0 ? 1 : 0) | (i == last ? 2 : 0);
        if (!sw) continue;
        Step& s = p->steps[i];
        if (s.kind == STEP_PASS || s.kind == STEP_TREE_PASS) {
            const PassKernel& k = *s.pk;
            const TwinKernel* t = find_twin(k, sw);
            if (!t)
                return fail("no inverse twin (swap %d) of pass kernel prec=%d R=%d C=%d mode=%d nts=%d lp=%d vpt=%d", sw,
                            k.prec, k.R, k.C, k.mode, k.nts, k.lp, k.vpt);
            s.fn = t->fn;
        } else {
            const void* t = find_aux_twin(s.fn, sw);
            if (!t) return fail("no inverse twin (swap %d) of the %s kernel of launch %zu", sw,
                                s.kind == STEP_TREE ? "tree" : "interleave", i);
            s.fn = t;
        }
    }
    return 0;
}

// one chain of launches for the shape p holds: choose (pifft_planner.h), lay
// out the tables at the end of tb's blob, assemble the launches (an inverse
// plan: with its twins).  No device, no allocation; a matrix plan runs it
// twice over one builder (build_matrix)
int plan_chain(pifft_plan* p, TableBuilder& tb) {
    PlanChoice ch;
    if (choose_plan(*p, ch)) return -1;
    const TableLayout tl = layout_tables(*p, ch, tb);
    p->tw_bytes = tb.size() ? tb.size() : 256;
    return (assemble_steps(p, ch, tl) || (p->inverse && make_inverse(p))) ? -1 : 0;
}
// the chain, a real plan's added launch, then, unless dry (pifft_plan_dry_run:
// no device, no allocation), materialise.
// real_n: the real length of a real plan (its added launch), else 0
int build_plan(pifft_plan* p, bool dry, uint64_t real_n = 0) {
    TableBuilder tb(p->esz);
    tb.size_only = dry;
    if (plan_chain(p, tb)) return -1;
    if (real_n) add_real_step(p, tb, real_n, p->inverse);
    return dry ? 0 : materialise(p, tb);
}

// the checks every plan shares; real: a real plan of n reals (create_real),
// which splits its n/2-point transform
int check_args(pifft_plan** out, uint64_t n, uint32_t workers, uint32_t first, uint32_t count, uint32_t batch, int prec,
               bool real) {
    if (!out) return fail("plan pointer is NULL");
    *out = nullptr;
    if (real && (n < 4 || !is_pow2(n))) return fail("Invalid input size (a real plan needs 2^i reals, i > 1)");
    if (n < 2 || !is_pow2(n)) return fail("Invalid input size (should be 2^i for i>0)");
    if (workers == 0 || !is_pow2(workers)) return fail("Invalid number of procs (should be 2^i for i>0)");
    if (real && workers > n / 2) return fail("More processors than inputs! (a real plan splits its n/2-point transform)");
    if (workers > n) return fail("More processors than inputs!");
    if (count == 0 || !is_pow2(count) || first % count != 0 || (uint64_t)first + count > workers)
        return fail("invalid worker range [%u, %u) of %u", first, first + count, workers);
    if (batch == 0) return fail("batch must be >= 1");
    if (prec != PIFFT_F32 && prec != PIFFT_F64) return fail("prec must be PIFFT_F32 or PIFFT_F64");
    return 0;
}

// n: the complex transform's length; real_n: see build_plan
int create_checked(pifft_plan** out, uint64_t n, uint32_t workers, uint32_t first, uint32_t count, uint32_t batch,
                   int prec, int device, int flags, bool dry, uint64_t real_n = 0) {
    if (!dry) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail("no HIP device available");
        if (device < 0 || device >= ndev) return fail("device %d out of range (%d devices)", device, ndev);
    }
    const int order = flags & ~(PIFFT_SEPARATE_TREE | PIFFT_INVERSE);
    pifft_plan* p = new pifft_plan;
    static_cast<PlanShape&>(*p) = plan_shape(n, workers, first, count, batch, prec, order == PIFFT_OUT_NATURAL,
                                             order == PIFFT_OUT_BITREV, (flags & PIFFT_SEPARATE_TREE) != 0);
    p->device = dry ? -1 : device;
    p->flags = flags;
    p->inverse = (flags & PIFFT_INVERSE) != 0;
    DeviceGuard g(p->device);
    if (build_plan(p, dry, real_n)) {
        std::string keep = g_err;
        release(p);
        g_err = keep;
        return -1;
    }
    *out = p;
    return 0;
}

int create(pifft_plan** out, uint64_t n, uint32_t workers, uint32_t first, uint32_t count,
           uint32_t batch, int prec, int device, int flags, bool dry = false) {
    if (check_args(out, n, workers, first, count, batch, prec, false)) return -1;
    const int order = flags & ~(PIFFT_SEPARATE_TREE | PIFFT_INVERSE);
    if (order != PIFFT_OUT_NATURAL && order != PIFFT_OUT_SLICES && order != PIFFT_OUT_BITREV)
        return fail("unknown flags %d", flags);
    // (flags name an order for a worker range: the value is as unknown for a
    // partial range -- PIFFT_INVERSE alone, say, which implies natural order --
    // as an undefined bit is, and the message says which rule it broke)
    if (order == PIFFT_OUT_NATURAL && count != workers)
        return fail("unknown flags %d for workers [%u, %u) of %u: natural-order output needs all workers on one plan "
                    "(use PIFFT_OUT_SLICES)", flags, first, first + count, workers);
    return create_checked(out, n, workers, first, count, batch, prec, device, flags, dry);
}

// Real-input plans (pifft_plan_create_real; kernels and formulas in
// pifft_real.h).  The N reals are the H = N/2 complex values z[n] = x[2n] +
// i x[2n+1] as they lie in memory, so the plan is the complex plan build_plan
// makes for (H, P, all workers, natural order) -- untouched, whatever
// choose_plan picks for that shape -- plus one streaming launch (add_real_step):
//   R2C: [inner forward chain: d_in -> Z] [k_r2c_post: Z -> d_out]
//   C2R: [k_c2r_pre: d_in -> Z] [inner inverse chain (make_inverse): Z -> d_out]
// Z (BUF_Z, batch x H values) is plan-owned: the inner chain of an R2C plan
// uses it wherever the complex plan uses the caller's output (its last store
// and, in multi-pass plans, a ping-pong stage), that of a C2R plan where the
// complex plan reads the caller's input; d_in is never written.  Bins k and
// H - k belong to different workers (residues r and -r mod P), so a real plan
// always holds all P workers.
int create_real(pifft_plan** out, uint64_t n, uint32_t workers, uint32_t batch, int prec, int device, int direction,
                bool dry = false) {
    if (check_args(out, n, workers, 0, workers, batch, prec, true)) return -1;
    if (direction != PIFFT_REAL_FORWARD && direction != PIFFT_REAL_INVERSE)
        return fail("direction must be PIFFT_REAL_FORWARD or PIFFT_REAL_INVERSE");
    const bool c2r = direction == PIFFT_REAL_INVERSE;
    return create_checked(out, n / 2, workers, 0, workers, batch, prec, device,
                          PIFFT_OUT_NATURAL | (c2r ? PIFFT_INVERSE : 0), dry, n);
}

// a chain's launches joined to plan p with its caller-side buffers renamed
// (matrix and chirp plans: two chains planned by plan_chain over one builder)
void splice(pifft_plan* p, const pifft_plan& q, int in, int out) {
    for (Step s : q.steps) {
        s.src = s.src == BUF_IN ? in : s.src == BUF_OUT ? out : s.src;
        s.dst = s.dst == BUF_OUT ? out : s.dst;
        p->steps.push_back(s);
    }
    for (int i = 0; i < q.npasses; i++) {
        p->radix[p->npasses] = q.radix[i];
        p->lines[p->npasses] = q.lines[i];
        p->vpt[p->npasses++] = q.vpt[i];
    }
    p->wil |= q.wil;
    p->ilv |= q.ilv;
}

// Matrix plans (pifft_plan_create_matrix; the kernel in pifft_matrix.h): batch
// arrays of n0 x n1 values.  The plan is the two complex plans plan_chain makes
// for the rows, (n1, one worker, batch n0), and the columns, (n0, one worker,
// batch n1) -- natural order, untouched, PIFFT_INVERSE each on its own -- with
// k_transpose launches between them, over Z (BUF_Z, batch n0 n1 values):
//   natural:        [rows: d_in -> Z] [T: Z -> d_out] [columns: d_out -> Z] [T: Z -> d_out]
//   transposed out: [rows: d_in -> d_out] [T: d_out -> Z] [columns: Z -> d_out]
// A chain keeps its own ping-pong: where the complex plan uses the caller's
// output it uses the buffer named above (remap, as add_real_step), and W as
// ever.  The chains never run concurrently: one W of the larger size.  Both
// chains' tables go into one blob (one TableBuilder: the second chain's offsets
// come out rebased), so materialise resolves the spliced steps as any plan's.
int build_matrix(pifft_plan* p, bool dry) {
    const bool tout = (p->flags & PIFFT_MATRIX_TRANSPOSED_OUT) != 0;
    TableBuilder tb(p->esz);
    tb.size_only = dry;
    pifft_plan chain[2];  // rows, columns: planned here, never materialised (they own nothing)
    const uint64_t len[2] = {p->n1, p->n0};
    for (int c = 0; c < 2; c++) {
        pifft_plan& q = chain[c];
        static_cast<PlanShape&>(q) =
            plan_shape(len[c], 1, 0, 1, (uint32_t)(p->batch * len[1 - c]), p->prec, true, false, false);
        q.device = -1;
        q.flags = p->flags & PIFFT_INVERSE;
        q.inverse = p->inverse;
        if (plan_chain(&q, tb)) return -1;
    }
    p->tw_bytes = tb.size();
    if (chain[0].npasses + chain[1].npasses > 8)
        return fail("matrix plan: %d + %d passes exceed the 8 a plan describes", chain[0].npasses, chain[1].npasses);
    const uint64_t total = (uint64_t)p->batch * p->n0 * p->n1;
    p->bytes_z = (size_t)total * p->esz;
    p->bytes_w = std::max(chain[0].bytes_w, chain[1].bytes_w);
    auto transpose = [&](uint64_t rows, uint64_t cols, int src, int dst) {
        Step s;
        s.kind = STEP_TRANSPOSE;
        s.fn = transpose_fn(p->prec);
        s.xa = p->prec == PIFFT_F64 ? transpose_args<double>(rows, cols, p->batch)
                                    : transpose_args<float>(rows, cols, p->batch);
        s.src = src;
        s.dst = dst;
        s.block = dim3(256);
        s.grid = dim3(stride_grid(s.xa.tiles * 256));  // one workgroup per tile, up to the cap
        s.bytes = 2 * total * p->esz;
        p->steps.push_back(s);
    };
    if (tout) {
        splice(p, chain[0], BUF_IN, BUF_OUT);
        transpose(p->n0, p->n1, BUF_OUT, BUF_Z);
        splice(p, chain[1], BUF_Z, BUF_OUT);
    } else {
        splice(p, chain[0], BUF_IN, BUF_Z);
        transpose(p->n0, p->n1, BUF_Z, BUF_OUT);
        splice(p, chain[1], BUF_OUT, BUF_Z);
        transpose(p->n1, p->n0, BUF_Z, BUF_OUT);
    }
    return dry ? 0 : materialise(p, tb);
}

int create_matrix(pifft_plan** out, uint64_t n0, uint64_t n1, uint32_t batch, int prec, int device, int flags,
                  bool dry = false) {
    if (!out) return fail("plan pointer is NULL");
    *out = nullptr;
    if (n0 < 2 || !is_pow2(n0) || n1 < 2 || !is_pow2(n1))
        return fail("Invalid matrix size (n0 and n1 should be 2^i for i>0)");
    if (batch == 0) return fail("batch must be >= 1");
    if (prec != PIFFT_F32 && prec != PIFFT_F64) return fail("prec must be PIFFT_F32 or PIFFT_F64");
    if (flags & ~(PIFFT_INVERSE | PIFFT_MATRIX_TRANSPOSED_OUT))
        return fail("unknown flags %d (a matrix plan takes PIFFT_INVERSE and PIFFT_MATRIX_TRANSPOSED_OUT)", flags);
    // (n0, n1 < 2^32 from here on: batch n0 n1 < 2^64)
    if (std::max(n0, n1) > 0xffffffffull / batch)
        return fail("matrix plan too large: batch * max(n0, n1) must fit the row transforms' 32-bit batch");
    if (!dry) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail("no HIP device available");
        if (device < 0 || device >= ndev) return fail("device %d out of range (%d devices)", device, ndev);
    }
    pifft_plan* p = new pifft_plan;
    static_cast<PlanShape&>(*p) = plan_shape(n0 * n1, 1, 0, 1, batch, prec, true, false, false);
    p->matrix = true;
    p->n0 = n0;
    p->n1 = n1;
    p->device = dry ? -1 : device;
    p->flags = flags;
    p->inverse = (flags & PIFFT_INVERSE) != 0;
    DeviceGuard g(p->device);
    if (build_matrix(p, dry)) {
        std::string keep = g_err;
        release(p);
        g_err = keep;
        return -1;
    }
    *out = p;
    return 0;
}

// Chirp plans (pifft_plan_create_chirp; kernels and formulas in pifft_chirp.h):
// batch rows of N values, N no power of two.  The plan is the two complex
// plans plan_chain makes for (M, one worker, natural order, batch), M =
// chirp_length(N) -- untouched; the second with PIFFT_INVERSE -- around a
// pointwise product, between two streaming launches, over Z (BUF_Z) and Y
// (BUF_Y), batch x M values each:
//   [k_chirp_pre: d_in -> Z] [forward chain: Z -> Y] [k_spectrum_mul: Y in place]
//   [inverse chain: Y -> Z] [k_chirp_post: Z -> d_out]
// A chain keeps its own ping-pong (splice, as build_matrix) and W as ever; the
// chains never run concurrently: one W of the larger size.  Both chains'
// tables and the two-level table of w_2N go into one blob.  The plan's own
// PIFFT_INVERSE is the swapping twins of the first and the last launch; the
// chains between are the same in both directions.
int chirp_spectrum(pifft_plan* p);  // (below: it runs a plan)
int build_chirp(pifft_plan* p, bool dry) {
    const uint64_t N = p->chirp_n, M = p->n;
    TableBuilder tb(p->esz);
    tb.size_only = dry;
    pifft_plan chain[2];  // forward, inverse: planned here, never materialised (they own nothing)
    for (int c = 0; c < 2; c++) {
        pifft_plan& q = chain[c];
        static_cast<PlanShape&>(q) = plan_shape(M, 1, 0, 1, p->batch, p->prec, true, false, false);
        q.device = -1;
        q.flags = c ? PIFFT_INVERSE : 0;
        q.inverse = c == 1;
        if (plan_chain(&q, tb)) return -1;
    }
    const TwoLevel tw = two_level_any(tb, 2 * N);
    tb.align();
    p->tw_bytes = tb.size();
    if (chain[0].npasses + chain[1].npasses > 8)
        return fail("chirp plan: %d + %d passes exceed the 8 a plan describes", chain[0].npasses, chain[1].npasses);
    p->bytes_z = p->bytes_y = (size_t)p->batch * M * p->esz;
    p->bytes_bt = (size_t)M * p->esz;
    p->bytes_w = std::max(chain[0].bytes_w, chain[1].bytes_w);
    auto stream = [&](int step, int kind, int sw, int src, int dst, uint64_t elems) {
        Step s;
        s.kind = step;
        s.fn = chirp_fn(kind, p->prec, sw);
        const uint64_t units = p->prec == PIFFT_F64 ? chirp_units<double>(kind, N, M) : chirp_units<float>(kind, N, M);
        s.block = dim3(256);
        s.grid = dim3(stride_grid((uint64_t)p->batch * units));
        s.ca = p->prec == PIFFT_F64 ? chirp_args<double>(kind, N, p->batch, (uint64_t)s.grid.x * 256)
                                    : chirp_args<float>(kind, N, p->batch, (uint64_t)s.grid.x * 256);
        s.ca.tw_h = tw.h;
        s.tab.lo = tw.lo;
        s.tab.hi = tw.hi;
        s.src = src;
        s.dst = dst;
        s.bytes = elems * p->esz;
        p->steps.push_back(s);
    };
    stream(STEP_CHIRP_PRE, CHIRP_PRE, p->inverse ? 1 : 0, BUF_IN, BUF_Z, (uint64_t)p->batch * (N + M));
    splice(p, chain[0], BUF_Z, BUF_Y);
    stream(STEP_SPECTRUM_MUL, CHIRP_MUL, 0, BUF_Y, BUF_Y, (uint64_t)p->batch * 2 * M + M);
    splice(p, chain[1], BUF_Y, BUF_Z);
    stream(STEP_CHIRP_POST, CHIRP_POST, p->inverse ? 2 : 0, BUF_Z, BUF_OUT, (uint64_t)p->batch * 2 * N);
    return dry ? 0 : (materialise(p, tb) || chirp_spectrum(p)) ? -1 : 0;
}

int create_chirp(pifft_plan** out, uint64_t n, uint32_t batch, int prec, int device, int flags, bool dry = false) {
    if (!out) return fail("plan pointer is NULL");
    *out = nullptr;
    if (n >= 2 && is_pow2(n))
        return fail("Invalid input size (a chirp plan takes an n that is no power of two: use pifft_plan_create for 2^i)");
    if (n < 3 || n > (1ull << 27)) return fail("Invalid input size (a chirp plan needs 3 <= n <= 2^27)");
    if (batch == 0) return fail("batch must be >= 1");
    if (prec != PIFFT_F32 && prec != PIFFT_F64) return fail("prec must be PIFFT_F32 or PIFFT_F64");
    if (flags & ~PIFFT_INVERSE) return fail("unknown flags %d (a chirp plan takes PIFFT_INVERSE)", flags);
    if (!dry) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail("no HIP device available");
        if (device < 0 || device >= ndev) return fail("device %d out of range (%d devices)", device, ndev);
    }
    pifft_plan* p = new pifft_plan;
    static_cast<PlanShape&>(*p) = plan_shape(chirp_length(n), 1, 0, 1, batch, prec, true, false, false);
    p->chirp_n = n;
    p->device = dry ? -1 : device;
    p->flags = flags;
    p->inverse = (flags & PIFFT_INVERSE) != 0;
    DeviceGuard g(p->device);
    if (build_chirp(p, dry)) {
        std::string keep = g_err;
        release(p);
        g_err = keep;
        return -1;
    }
    *out = p;
    return 0;
}

// Convolution plans (pifft_plan_create_conv; kernels and formulas in
// pifft_conv.h): batch rows of n reals times one filter of taps reals.  With
// M = conv_length(n, taps) (cyclic: n) and H = M/2 the plan is the two complex
// plans plan_chain makes for (H, one worker, natural order, batch) -- untouched;
// the second with PIFFT_INVERSE, exactly the chains of the real plans of M --
// around the fused pair kernel, over Z (BUF_Z) and Y (BUF_Y), batch x H values:
//   linear: [k_conv_pad: d_in -> Z] [forward chain: Z -> Y] [k_conv_pair: Y in place]
//           [inverse chain: Y -> Z] [k_conv_crop: Z -> d_out]
//   cyclic: [forward chain: d_in -> Y] [k_conv_pair: Y in place] [inverse chain: Y -> d_out]
// A chain keeps its own ping-pong (splice, as build_matrix) and W as ever.
// pifft_conv_set_filter's launches (filter_steps) are planned here too:
//   [k_conv_filter: d_h -> Z row 0] [forward chain at batch 1: Z -> Y row 0] [k_r2c_post: Y -> G]
// the chain by plan_chain for (H, one worker, batch 1), whose launches may
// differ from those for `batch`.  The three chains never run concurrently: one
// W of the largest size.  All their tables and the two-level table of w_M go
// into one blob.  A cyclic plan's Z is the one row set_filter needs.
int build_conv(pifft_plan* p, bool dry) {
    const uint64_t H = p->n, M = p->conv_m;
    const bool cyclic = (p->flags & PIFFT_CONV_CYCLIC) != 0;
    TableBuilder tb(p->esz);
    tb.size_only = dry;
    pifft_plan chain[3];  // forward, inverse, forward at batch 1: planned here, never materialised
    for (int c = 0; c < 3; c++) {
        pifft_plan& q = chain[c];
        static_cast<PlanShape&>(q) = plan_shape(H, 1, 0, 1, c == 2 ? 1 : p->batch, p->prec, true, false, false);
        q.device = -1;
        q.flags = c == 1 ? PIFFT_INVERSE : 0;
        q.inverse = c == 1;
        if (plan_chain(&q, tb)) return -1;
    }
    const TwoLevel tw = two_level(tb, M);
    tb.align();
    p->tw_bytes = tb.size();
    if (chain[0].npasses + chain[1].npasses > 8)
        return fail("convolution plan: %d + %d passes exceed the 8 a plan describes", chain[0].npasses,
                    chain[1].npasses);
    p->bytes_z = (size_t)(cyclic ? 1 : p->batch) * H * p->esz;
    p->bytes_y = (size_t)p->batch * H * p->esz;
    p->bytes_g = (size_t)(H + 1) * p->esz;
    p->bytes_w = std::max(std::max(chain[0].bytes_w, chain[1].bytes_w), chain[2].bytes_w);
    const size_t rsz = p->esz / 2;  // bytes of a real
    auto stream = [&](std::vector<Step>& to, int step, int kind, uint64_t len, uint32_t batch, int src, int dst,
                      uint64_t bytes) {
        Step s;
        s.kind = step;
        s.fn = conv_fn(kind, p->prec);
        const uint64_t units = p->prec == PIFFT_F64 ? conv_units<double>(kind, len, H) : conv_units<float>(kind, len, H);
        s.block = dim3(256);
        s.grid = dim3(stride_grid((uint64_t)batch * units));
        s.va = p->prec == PIFFT_F64 ? conv_args<double>(kind, len, H, batch, (uint64_t)s.grid.x * 256)
                                    : conv_args<float>(kind, len, H, batch, (uint64_t)s.grid.x * 256);
        s.va.tw_h = tw.h;
        s.va.rev = (step == STEP_CONV_FILTER && (p->flags & PIFFT_CONV_CORRELATE)) ? 1u : 0u;
        s.tab.lo = tw.lo;
        s.tab.hi = tw.hi;
        s.src = src;
        s.dst = dst;
        s.bytes = bytes;
        to.push_back(s);
    };
    if (!cyclic)
        stream(p->steps, STEP_CONV_PAD, CONV_PAD, p->conv_n, p->batch, BUF_IN, BUF_Z,
               (uint64_t)p->batch * (p->conv_n + M) * rsz);
    splice(p, chain[0], cyclic ? BUF_IN : BUF_Z, BUF_Y);
    stream(p->steps, STEP_CONV_PAIR, CONV_PAIR, 0, p->batch, BUF_Y, BUF_Y, ((uint64_t)p->batch * 2 * H + H + 1) * p->esz);
    splice(p, chain[1], BUF_Y, cyclic ? BUF_OUT : BUF_Z);
    if (!cyclic)
        stream(p->steps, STEP_CONV_CROP, CONV_CROP, p->conv_len, p->batch, BUF_Z, BUF_OUT,
               (uint64_t)p->batch * (M + p->conv_len) * rsz);
    // pifft_conv_set_filter: its d_h stands where an execution's d_in stands
    stream(p->filter_steps, STEP_CONV_FILTER, CONV_FILTER, p->conv_taps, 1, BUF_IN, BUF_Z, (p->conv_taps + M) * rsz);
    for (Step s : chain[2].steps) {
        s.src = s.src == BUF_IN ? BUF_Z : s.src == BUF_OUT ? BUF_Y : s.src;
        s.dst = s.dst == BUF_OUT ? BUF_Y : s.dst;
        p->filter_steps.push_back(s);
    }
    Step r;
    r.kind = STEP_R2C_POST;
    r.fn = aux_fn(PIFFT_AUX_R2C, p->prec);
    r.tab.lo = tw.lo;
    r.tab.hi = tw.hi;
    r.ra.tw_h = tw.h;
    r.ra.batch = 1;
    r.ra.h = H;
    r.ra.units = p->prec == PIFFT_F64 ? real_units<double>(H) : real_units<float>(H);
    r.block = dim3(256);
    r.grid = dim3(stride_grid(r.ra.units));
    r.ra.step_rows = ((uint64_t)r.grid.x * 256) / r.ra.units;
    r.ra.step_units = ((uint64_t)r.grid.x * 256) % r.ra.units;
    r.bytes = (2 * H + 1) * p->esz;
    r.src = BUF_Y;
    r.dst = BUF_G;
    p->filter_steps.push_back(r);
    return dry ? 0 : materialise(p, tb);
}

int create_conv(pifft_plan** out, uint64_t n, uint64_t taps, uint32_t batch, int prec, int device, int flags,
                bool dry = false) {
    if (!out) return fail("plan pointer is NULL");
    *out = nullptr;
    if (n == 0 || taps == 0) return fail("Invalid input size (a convolution plan needs n >= 1 and taps >= 1)");
    if (batch == 0) return fail("batch must be >= 1");
    if (prec != PIFFT_F32 && prec != PIFFT_F64) return fail("prec must be PIFFT_F32 or PIFFT_F64");
    if (flags & ~(PIFFT_CONV_CORRELATE | PIFFT_CONV_CYCLIC))
        return fail("unknown flags %d (a convolution plan takes PIFFT_CONV_CORRELATE and PIFFT_CONV_CYCLIC)", flags);
    const bool cyclic = (flags & PIFFT_CONV_CYCLIC) != 0;
    const uint64_t cap = 1ull << 28;
    if (cyclic) {
        if (n < 4 || !is_pow2(n)) return fail("Invalid input size (a cyclic convolution plan needs n = 2^i, i > 1)");
        if (n > cap) return fail("convolution plan too large: a cyclic plan needs n <= 2^28");
        if (taps > n) return fail("Invalid filter size (a cyclic convolution plan needs taps <= n)");
    } else if (n > cap || taps > cap || n + taps - 1 > cap) {
        return fail("convolution plan too large: n + taps - 1 must not exceed 2^28");
    }
    if (!dry) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail("no HIP device available");
        if (device < 0 || device >= ndev) return fail("device %d out of range (%d devices)", device, ndev);
    }
    const uint64_t M = cyclic ? n : conv_length(n, taps);
    pifft_plan* p = new pifft_plan;
    static_cast<PlanShape&>(*p) = plan_shape(M / 2, 1, 0, 1, batch, prec, true, false, false);
    p->conv = true;
    p->conv_n = n;
    p->conv_taps = taps;
    p->conv_len = cyclic ? n : n + taps - 1;
    p->conv_m = M;
    p->device = dry ? -1 : device;
    p->flags = flags;
    DeviceGuard g(p->device);
    if (build_conv(p, dry)) {
        std::string keep = g_err;
        release(p);
        g_err = keep;
        return -1;
    }
    *out = p;
    return 0;
}

const char* kRealOnly = "real plans (pifft_plan_create_real) run through pifft_execute_device, "
                        "pifft_execute_device_timed, pifft_profile_* and pifft_launch_loop only";
const char* kMatrixOnly = "matrix plans (pifft_plan_create_matrix) run through pifft_execute_device, "
                          "pifft_execute_device_timed, pifft_profile_* and pifft_launch_loop only";
const char* kChirpOnly = "chirp plans (pifft_plan_create_chirp) run through pifft_execute_device, "
                         "pifft_execute_device_timed, pifft_profile_* and pifft_launch_loop only";
// why a host-boundary / multi-plan / tree / tuning entry point refuses plan p, or NULL
const char* kConvOnly = "convolution plans (pifft_plan_create_conv) run through pifft_execute_device, "
                        "pifft_execute_device_timed, pifft_profile_* and pifft_launch_loop only";
const char* device_only(const pifft_plan* p) {
    return p->real ? kRealOnly : p->matrix ? kMatrixOnly : p->chirp_n ? kChirpOnly : p->conv ? kConvOnly : nullptr;
}

// One launch.  With events (e0, e1): hipExtLaunchKernel binds them to the
// kernel's own dispatch (its start and end timestamps, what rocprofv3 reports
// as the kernel's duration) -- no marker packet between launches.  Marker
// events (hipEventRecord before every launch) cost ~4 us of GPU time each and
// made the per-launch means of the 10-50 us configs longer than their steps
// (round-2 verdict); kernel-bound events add nothing to the stream.
int launch_step(pifft_plan* p, const Step& s, const void* d_in, void* d_out, hipStream_t st,
                hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr) {
    void* base[NBUF] = {const_cast<void*>(d_in), d_out,         p->buf[BUF_W], p->buf[BUF_TA],
                        p->buf[BUF_Z],           p->buf[BUF_Y], p->buf[BUF_G]};
    const char* src = (const char*)base[s.src] + s.src_off * p->esz;
    char* dst = (char*)base[s.dst] + s.dst_off * p->esz;
    auto go = [&](void** args, size_t lds) {
        return (e0 || e1) ? hipExtLaunchKernel(s.fn, s.grid, s.block, args, lds, st, e0, e1, 0)
                          : hipLaunchKernel(s.fn, s.grid, s.block, args, lds, st);
    };
    hipError_t e = hipSuccess;
    switch (s.kind) {
        case STEP_PASS:
        case STEP_TREE_PASS: {
            PassArgs a = s.pa;
            a.in = src;
            a.out = dst;
#ifdef PIFFT_WG_CLOCK
            a.wg_clock = p->dbg_clk;
#endif
            void* args[] = {&a};
            e = go(args, s.lds);
            break;
        }
        case STEP_TREE: {
            TreeArgs a = s.ta;
            a.in = src;
            a.out = dst;
            void* args[] = {&a};
            e = go(args, s.lds);
            break;
        }
        case STEP_INTERLEAVE: {
            const void* in = src;
            void* o = dst;
            uint64_t total = s.il_total;
            uint32_t ln = s.il_log_n, lpp = s.il_log_p;
            void* args[] = {&in, &o, &total, &ln, &lpp};
            e = go(args, 0);
            break;
        }
        case STEP_R2C_POST:
        case STEP_C2R_PRE: {
            RealArgs a = s.ra;
            a.in = src;
            a.out = dst;
            void* args[] = {&a};
            e = go(args, 0);
            break;
        }
        case STEP_TRANSPOSE: {
            TransposeArgs a = s.xa;
            a.in = src;
            a.out = dst;
            void* args[] = {&a};
            e = go(args, 0);
            break;
        }
        case STEP_CHIRP_PRE:
        case STEP_SPECTRUM_MUL:
        case STEP_CHIRP_POST: {
            ChirpArgs a = s.ca;
            a.in = src;
            a.out = dst;
            void* args[] = {&a};
            e = go(args, 0);
            break;
        }
        case STEP_CONV_PAD:
        case STEP_CONV_PAIR:
        case STEP_CONV_CROP:
        case STEP_CONV_FILTER: {
            ConvArgs a = s.va;
            a.in = src;
            a.out = dst;
            void* args[] = {&a};
            e = go(args, 0);
            break;
        }
        default:
            return fail("bad step kind %d", s.kind);
    }
    if (e != hipSuccess) return fail("kernel launch failed: %s", hipGetErrorString(e));
    return 0;
}

// every launch of the plan; ev (or NULL): 2 events per launch, its start and stop
int launch_steps(pifft_plan* p, const void* d_in, void* d_out, hipStream_t st, hipEvent_t* ev) {
    for (size_t i = 0; i < p->steps.size(); i++)
        if (launch_step(p, p->steps[i], d_in, d_out, st, ev ? ev[2 * i] : nullptr, ev ? ev[2 * i + 1] : nullptr))
            return -1;
    return 0;
}

// A chirp plan's Bt = DFT_M(b) / M, fixed at creation and the same for both
// precisions up to its one final rounding: b is filled on the device in fp64
// (k_chirp_fill, from an fp64 two-level table of w_2N), transformed by a
// temporary fp64 plan of (M, one worker, batch 1), scaled by the exact 1/M and
// rounded once to the plan's precision (k_chirp_bt).  No host sincos per
// element, no host FFT.  Synchronous; everything but Bt is freed on return.
int chirp_spectrum(pifft_plan* p) {
    const uint64_t N = p->chirp_n, M = p->n;
    TableBuilder tb(16);
    const TwoLevel tw = two_level_any(tb, 2 * N);
    pifft_plan* t = nullptr;
    void *d_tab = nullptr, *d_b = nullptr, *d_B = nullptr;
    auto run = [&]() -> int {
        if (create(&t, M, 1, 0, 1, 1, PIFFT_F64, p->device, PIFFT_OUT_NATURAL)) return -1;
        HIPCHK(hipMalloc(&d_tab, tb.blob.size()));
        HIPCHK(hipMalloc(&d_b, (size_t)M * 16));
        HIPCHK(hipMalloc(&d_B, (size_t)M * 16));
        HIPCHK(hipMemcpy(d_tab, tb.blob.data(), tb.blob.size(), hipMemcpyHostToDevice));
        const dim3 grid(stride_grid(M)), block(256);
        ChirpArgs a = chirp_args<double>(CHIRP_FILL, N, 1, (uint64_t)grid.x * 256);
        a.out = d_b;
        a.tw_lo = (const char*)d_tab + tw.lo;
        a.tw_hi = (const char*)d_tab + tw.hi;
        a.tw_h = tw.h;
        void* fill_args[] = {&a};
        HIPCHK(hipLaunchKernel(chirp_fn(CHIRP_FILL, 64, 0), grid, block, fill_args, 0, p->stream));
        if (launch_steps(t, d_b, d_B, p->stream, nullptr)) return -1;
        double inv_m = 1.0 / (double)M;
        uint64_t m = M;
        void* bt_args[] = {&d_B, &p->d_bt, &inv_m, &m};
        HIPCHK(hipLaunchKernel(chirp_fn(CHIRP_BT, p->prec, 0), grid, block, bt_args, 0, p->stream));
        HIPCHK(hipStreamSynchronize(p->stream));
        return 0;
    };
    const int rc = run();
    const std::string keep = g_err;
    if (rc) (void)hipStreamSynchronize(p->stream);
    if (d_tab) (void)hipFree(d_tab);
    if (d_b) (void)hipFree(d_b);
    if (d_B) (void)hipFree(d_B);
    release(t);
    g_err = keep;
    return rc;
}

// per-launch durations of one recorded execution (ev as launch_steps)
int read_launch_ms(size_t ns, hipEvent_t* ev, std::vector<float>& ms) {
    ms.assign(ns, 0.0f);
    if (!ns) return 0;
    HIPCHK(hipEventSynchronize(ev[2 * ns - 1]));
    for (size_t i = 0; i < ns; i++) HIPCHK(hipEventElapsedTime(&ms[i], ev[2 * i], ev[2 * i + 1]));
    return 0;
}

int check_buffers(const pifft_plan* p, const void* d_in, void* d_out) {
    if (!p) return fail("plan is NULL");
    if (!d_in || !d_out) return fail("NULL device buffer");
    if (d_in == d_out) return fail("in-place execution is not supported (d_in == d_out)");
    // k_transpose moves fp32 values in 16-B pairs (pifft_matrix.h): hipMalloc's alignment is enough
    if (p->matrix && (((uintptr_t)d_in | (uintptr_t)d_out) & 15))
        return fail("matrix plans need 16-byte aligned device buffers");
    if (p->conv && !p->conv_ready)
        return fail("convolution plan: no filter set (call pifft_conv_set_filter before executing)");
    return 0;
}

uint64_t out_elems(const pifft_plan* p) { return (uint64_t)p->batch * p->nq * p->m; }

// run every step with kernel-bound events, wait, per-launch durations
int run_timed(pifft_plan* p, const void* d_in, void* d_out, hipStream_t st, std::vector<float>& ms) {
    if (launch_steps(p, d_in, d_out, st, p->ev.data())) return -1;
    return read_launch_ms(p->steps.size(), p->ev.data(), ms);
}

bool stage1_step(const Step& s) { return s.kind == STEP_TREE || s.kind == STEP_TREE_PASS; }

void stage_split(const pifft_plan* p, const std::vector<float>& ms, double* s1, double* s2) {
    double a = 0, b = 0;
    for (size_t i = 0; i < ms.size(); i++) (stage1_step(p->steps[i]) ? a : b) += ms[i];
    if (s1) *s1 = a;
    if (s2) *s2 = b;
}

// One execution timed like the reference's two stage timers (tm_funnel,
// tm_tube: wall clock around each whole stage, CPU.c:414-481): a marker
// event before the stage's first launch and after its last, so the gaps and
// launch latency between kernels count.  (The stage-1 launches -- the tree,
// or the tree fused into the first pass -- lead every plan.)
// An empty stage (P = 1: no tree, as the reference's funnel loop that never
// runs; M = 1: no local FFT) gets no marker of its own and reads 0.
size_t stage1_launches(const pifft_plan* p) {
    size_t n1 = 0;
    while (n1 < p->steps.size() && stage1_step(p->steps[n1])) n1++;
    return n1;
}
int launch_stage_marked(pifft_plan* p, const void* d_in, void* d_out) {
    const size_t n1 = stage1_launches(p), ns = p->steps.size();
    HIPCHK(hipEventRecord(p->sev[0], p->stream));
    for (size_t i = 0; i < ns; i++) {
        if (i == n1 && n1 > 0) HIPCHK(hipEventRecord(p->sev[1], p->stream));
        if (launch_step(p, p->steps[i], d_in, d_out, p->stream)) return -1;
    }
    HIPCHK(hipEventRecord(p->sev[2], p->stream));
    return 0;
}
int read_stage_marked(pifft_plan* p, double* s1, double* s2) {
    const size_t n1 = stage1_launches(p), ns = p->steps.size();
    float a = 0.0f, b = 0.0f;
    HIPCHK(hipEventSynchronize(p->sev[2]));
    if (n1 == 0)
        HIPCHK(hipEventElapsedTime(&b, p->sev[0], p->sev[2]));
    else if (n1 == ns)
        HIPCHK(hipEventElapsedTime(&a, p->sev[0], p->sev[2]));
    else {
        HIPCHK(hipEventElapsedTime(&a, p->sev[0], p->sev[1]));
        HIPCHK(hipEventElapsedTime(&b, p->sev[1], p->sev[2]));
    }
    *s1 = a;
    *s2 = b;
    return 0;
}

// device result of a plan holding only some workers (slice-major) -> their
// natural-order host positions (natural-order and bit-reversed plans copy
// straight into host_out, pifft_execute_group)
void scatter_to_host(const pifft_plan* p, const char* res, char* host_out) {
    const size_t esz = p->esz;
    const uint64_t M = p->m;
    // a plan holding only some workers: its bins go to their stride-P
    // natural-order positions (other positions untouched, CPU.c:496-499).
    // host_out is a plain C buffer (a double _Complex / float _Complex array is
    // only 8- / 4-byte aligned): element-sized memcpy, which the compiler
    // lowers to plain moves without assuming cx<T>'s 16- / 8-byte alignment
    for (uint32_t bt = 0; bt < p->batch; bt++) {
        for (uint32_t q = p->q0; q < p->q0 + p->nq; q++) {
            const uint64_t r = bitrev(q, p->lp);
            const char* s = res + ((uint64_t)bt * p->nq * M + (uint64_t)(q - p->q0) * M) * esz;
            char* d = host_out + ((uint64_t)bt * p->n + r) * esz;
            const uint64_t dstride = (uint64_t)p->P * esz;
            if (esz == 16)
                for (uint64_t k = 0; k < M; k++) memcpy(d + k * dstride, s + k * 16, 16);
            else
                for (uint64_t k = 0; k < M; k++) memcpy(d + k * dstride, s + k * 8, 8);
        }
    }
}

int ensure_host_staging(pifft_plan* p) {
    if (!p->d_hin) HIPCHK(hipMalloc(&p->d_hin, (size_t)p->batch * p->n * p->esz));
    if (!p->d_hout) HIPCHK(hipMalloc(&p->d_hout, (size_t)out_elems(p) * p->esz));
    return 0;
}

int launch_interleave(const void* d_slices, void* d_out, uint64_t n, uint32_t workers, uint32_t batch, int prec,
                      hipStream_t st) {
    if (prec != PIFFT_F64 && prec != PIFFT_F32) return fail("bad precision");
    uint64_t total = (uint64_t)batch * n;
    const int lp = ilog2u(workers);
    uint32_t ln = (uint32_t)ilog2u(n), lpp = (uint32_t)lp;
    const void* in = d_slices;
    void* o = d_out;
    void* args[] = {&in, &o, &total, &ln, &lpp};
    HIPCHK(hipLaunchKernel(interleave_fn(prec, lp, n), dim3(stride_grid(interleave_threads(total, lp, prec, n))),
                           dim3(256), args, 0, st));
    return 0;
}

// The plans' worker ranges cover [0, P) exactly once, every plan slice-major
// (PIFFT_OUT_SLICES) with the same n, P, batch and precision.
int check_cover(pifft_plan* const* plans, int np, bool quiet) {
    if (!plans || np <= 0) return quiet ? -1 : fail("no plans");
    std::vector<int> order;
    for (int i = 0; i < np; i++) {
        const pifft_plan* p = plans[i];
        if (!p) return quiet ? -1 : fail("plan %d is NULL", i);
        if (p->n != plans[0]->n || p->P != plans[0]->P || p->batch != plans[0]->batch || p->prec != plans[0]->prec)
            return quiet ? -1 : fail("plans of a gather must share n, workers, batch and precision");
        if (p->inverse != plans[0]->inverse)
            return quiet ? -1 : fail("plans of a gather must share the direction (PIFFT_INVERSE on all or none)");
        if (p->natural || p->bitrev)
            return quiet ? -1 : fail("plan %d: a gather needs slice-major plans (PIFFT_OUT_SLICES)", i);
        order.push_back(i);
    }
    std::sort(order.begin(), order.end(), [&](int a, int b) { return plans[a]->q0 < plans[b]->q0; });
    uint64_t next = 0;
    for (int i : order) {
        if (plans[i]->q0 != next) break;
        next += plans[i]->nq;
    }
    if (next != plans[0]->P)
        return quiet ? -1 : fail("the plans' worker ranges must cover workers [0, %u) exactly once", plans[0]->P);
    return 0;
}

// peer access from plan d's device to `src_dev` (xGMI loads/copies without a
// host bounce); a pair that cannot peer still copies, staged by the runtime
int enable_peer(pifft_plan* d, int src_dev) {
    if (fault_at("enable_peer"))
        return fail("hipDeviceEnablePeerAccess(%d -> %d): injected fault (PIFFT_FAULT=enable_peer)", d->device, src_dev);
    if (src_dev == d->device) return 0;
    for (int e : d->peer_on)
        if (e == src_dev) return 0;
    int can = 0;
    HIPCHK(hipDeviceCanAccessPeer(&can, d->device, src_dev));
    if (can) {
        const hipError_t e = hipDeviceEnablePeerAccess(src_dev, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
            return fail("hipDeviceEnablePeerAccess(%d -> %d): %s", d->device, src_dev, hipGetErrorString(e));
        (void)hipGetLastError();  // clear a sticky "already enabled"
    }
    d->peer_on.push_back(src_dev);
    return 0;
}

// The optional final exchange: on every destination j with
// d_natural[j] != NULL, copy each plan's slices into the plan-owned gather
// buffer of j's device (hipMemcpyPeerAsync over xGMI, one copy stream per
// source so the links run concurrently), then interleave them into natural
// order (k_interleave).  Synchronous; *ms = the slowest destination's time.
int gather_group(pifft_plan* const* plans, int np, const void* const* d_slices, void* const* d_natural, double* ms) {
    if (check_cover(plans, np, false)) return -1;
    if (!d_slices || !d_natural) return fail("NULL buffer list");
    for (int i = 0; i < np; i++)
        if (!d_slices[i]) return fail("d_slices[%d] is NULL", i);
    const pifft_plan* p0 = plans[0];
    const uint64_t N = p0->n, M = p0->m;
    const size_t esz = p0->esz;
    // every destination is written (interleave) while other destinations'
    // copy streams may still read the sources: no destination may overlap
    // any source buffer (or another destination)
    auto overlap = [](const void* a, size_t na, const void* b, size_t nb) {
        const char *x = (const char*)a, *y = (const char*)b;
        return x < y + nb && y < x + na;
    };
    const size_t nat_bytes = (size_t)p0->batch * N * esz;
    for (int j = 0; j < np; j++) {
        if (!d_natural[j]) continue;
        for (int i = 0; i < np; i++) {
            const size_t sb = (size_t)out_elems(plans[i]) * esz;
            if (overlap(d_natural[j], nat_bytes, d_slices[i], sb))
                return fail("d_natural[%d] overlaps d_slices[%d]: destinations must be distinct from every source", j, i);
            if (i < j && d_natural[i] && overlap(d_natural[j], nat_bytes, d_natural[i], nat_bytes))
                return fail("d_natural[%d] overlaps d_natural[%d]", j, i);
        }
    }
    // the copy schedule (pifft_gather.h; its multi-device logic is unit-tested on the CPU)
    std::vector<GatherSrc> srcs;
    std::vector<bool> has_dst;
    for (int i = 0; i < np; i++) {
        srcs.push_back({plans[i]->device, plans[i]->q0, plans[i]->nq});
        has_dst.push_back(d_natural[i] != nullptr);
    }
    const GatherSchedule gs = gather_schedule(srcs, has_dst, N, M, p0->batch);
    // one destination's copies + interleave, enqueued (no host wait)
    auto enqueue = [&](int j) -> int {
        pifft_plan* d = plans[j];
        DeviceGuard g(d->device);
        if (!d->d_gather) HIPCHK(hipMalloc(&d->d_gather, (size_t)d->batch * N * esz));
        for (const auto& pr : gs.peer)
            if (pr.first == d->device && enable_peer(d, pr.second)) return -1;
        while ((int)d->gst.size() < gs.streams) {
            hipStream_t st;
            hipEvent_t ev;
            HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
            d->gst.push_back(st);
            HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            d->gdone.push_back(ev);
        }
        for (auto& e : d->gev)
            if (!e) HIPCHK(hipEventCreate(&e));
        HIPCHK(hipEventRecord(d->gev[0], d->stream));
        for (int i = 0; i < gs.streams; i++) HIPCHK(hipStreamWaitEvent(d->gst[i], d->gev[0], 0));
        for (const GatherCopy& c : gs.copies) {
            if (c.dst != j) continue;
            const pifft_plan* s = plans[c.src];
            if (fault_at("peer_copy"))
                return fail("hipMemcpyPeerAsync(%d <- %d): injected fault (PIFFT_FAULT=peer_copy)", d->device,
                            s->device);
            HIPCHK(hipMemcpyPeerAsync((char*)d->d_gather + c.dst_off * esz, d->device,
                                      (const char*)d_slices[c.src] + c.src_off * esz, s->device, c.elems * esz,
                                      d->gst[c.stream]));
        }
        for (int i = 0; i < gs.streams; i++) {
            HIPCHK(hipEventRecord(d->gdone[i], d->gst[i]));
            HIPCHK(hipStreamWaitEvent(d->stream, d->gdone[i], 0));
        }
        if (launch_interleave(d->d_gather, d_natural[j], N, d->P, d->batch, d->prec, d->stream)) return -1;
        HIPCHK(hipEventRecord(d->gev[1], d->stream));
        return 0;
    };
    for (int j = 0; j < np; j++) {
        if (!d_natural[j] || !enqueue(j)) continue;
        // a failure part-way: wait for what was already enqueued (copies
        // still reading the caller's slices, or writing a gather buffer)
        // before returning, so the caller may reuse its buffers and the plans
        // stay usable; the first error's message is kept
        const std::string msg = g_err;
        for (int k = 0; k <= j; k++) {
            if (!d_natural[k]) continue;
            DeviceGuard g(plans[k]->device);
            for (auto st : plans[k]->gst) (void)hipStreamSynchronize(st);
            (void)hipStreamSynchronize(plans[k]->stream);
        }
        (void)hipGetLastError();
        g_err = msg;
        return -1;
    }
    double worst = 0.0;
    for (int j = 0; j < np; j++) {
        if (!d_natural[j]) continue;
        pifft_plan* d = plans[j];
        DeviceGuard g(d->device);
        HIPCHK(hipEventSynchronize(d->gev[1]));
        float t = 0.0f;
        HIPCHK(hipEventElapsedTime(&t, d->gev[0], d->gev[1]));
        worst = std::max(worst, (double)t);
    }
    if (ms) *ms = worst;
    return 0;
}

}  // namespace

// ===========================================================================
// C-ABI
// ===========================================================================
extern "C" {

const char* pifft_last_error(void) { return g_err.c_str(); }

int pifft_abi_version(void) { return PIFFT_ABI_VERSION; }

int pifft_gpu_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        fail("hipGetDeviceCount: %s", hipGetErrorString(e));
        return -1;
    }
    return n;
}

int pifft_plan_create(pifft_plan** plan, uint64_t n, uint32_t workers, uint32_t batch, int prec) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    return create(plan, n, workers, 0, workers, batch, prec, dev, PIFFT_OUT_NATURAL);
}

int pifft_plan_create_slices(pifft_plan** plan, uint64_t n, uint32_t workers, uint32_t first,
                             uint32_t count, uint32_t batch, int prec, int device, int flags) {
    return create(plan, n, workers, first, count, batch, prec, device, flags);
}

void pifft_plan_destroy(pifft_plan* plan) { release(plan); }

int pifft_plan_dry_run(uint64_t n, uint32_t workers, uint32_t first, uint32_t count, uint32_t batch, int prec,
                       int flags, pifft_plan_info* info) {
    if (!info) return fail("info is NULL");
    pifft_plan* p = nullptr;
    if (create(&p, n, workers, first, count, batch, prec, -1, flags, true)) return -1;
    const int rc = pifft_plan_get_info(p, info);
    release(p);
    return rc;
}

int pifft_plan_create_real(pifft_plan** plan, uint64_t n, uint32_t workers, uint32_t batch, int prec, int device,
                           int direction) {
    return create_real(plan, n, workers, batch, prec, device, direction);
}

int pifft_plan_dry_run_real(uint64_t n, uint32_t workers, uint32_t batch, int prec, int direction,
                            pifft_plan_info* info) {
    if (!info) return fail("info is NULL");
    pifft_plan* p = nullptr;
    if (create_real(&p, n, workers, batch, prec, -1, direction, true)) return -1;
    const int rc = pifft_plan_get_info(p, info);
    release(p);
    return rc;
}

int pifft_plan_is_real(const pifft_plan* plan) { return plan ? plan->real : -1; }

int pifft_plan_create_matrix(pifft_plan** plan, uint64_t n0, uint64_t n1, uint32_t batch, int prec, int device,
                             int flags) {
    return create_matrix(plan, n0, n1, batch, prec, device, flags);
}

int pifft_plan_dry_run_matrix(uint64_t n0, uint64_t n1, uint32_t batch, int prec, int flags, pifft_plan_info* info) {
    if (!info) return fail("info is NULL");
    pifft_plan* p = nullptr;
    if (create_matrix(&p, n0, n1, batch, prec, -1, flags, true)) return -1;
    const int rc = pifft_plan_get_info(p, info);
    release(p);
    return rc;
}

int pifft_plan_create_chirp(pifft_plan** plan, uint64_t n, uint32_t batch, int prec, int device, int flags) {
    return create_chirp(plan, n, batch, prec, device, flags);
}

int pifft_plan_dry_run_chirp(uint64_t n, uint32_t batch, int prec, int flags, pifft_plan_info* info) {
    if (!info) return fail("info is NULL");
    pifft_plan* p = nullptr;
    if (create_chirp(&p, n, batch, prec, -1, flags, true)) return -1;
    const int rc = pifft_plan_get_info(p, info);
    release(p);
    return rc;
}

int pifft_plan_is_chirp(const pifft_plan* plan) { return plan ? (plan->chirp_n ? 1 : 0) : -1; }

int pifft_plan_create_conv(pifft_plan** plan, uint64_t n, uint64_t taps, uint32_t batch, int prec, int device,
                           int flags) {
    return create_conv(plan, n, taps, batch, prec, device, flags);
}

int pifft_plan_dry_run_conv(uint64_t n, uint64_t taps, uint32_t batch, int prec, int flags, pifft_plan_info* info) {
    if (!info) return fail("info is NULL");
    pifft_plan* p = nullptr;
    if (create_conv(&p, n, taps, batch, prec, -1, flags, true)) return -1;
    const int rc = pifft_plan_get_info(p, info);
    release(p);
    return rc;
}

int pifft_conv_set_filter(pifft_plan* p, const void* d_h, void* stream) {
    if (!p) return fail("plan is NULL");
    if (!p->conv) return fail("pifft_conv_set_filter: not a convolution plan");
    if (!d_h) return fail("NULL device buffer");
    DeviceGuard g(p->device);
    for (const Step& s : p->filter_steps)
        if (launch_step(p, s, d_h, nullptr, (hipStream_t)stream)) return -1;
    p->conv_ready = true;
    return 0;
}

int pifft_plan_is_conv(const pifft_plan* plan) { return plan ? (plan->conv ? 1 : 0) : -1; }

int pifft_plan_conv_shape(const pifft_plan* plan, uint64_t* n, uint64_t* taps, uint64_t* out_len, uint64_t* m) {
    if (!plan || !n || !taps || !out_len || !m) return fail("NULL argument");
    if (!plan->conv) return fail("pifft_plan_conv_shape: not a convolution plan");
    *n = plan->conv_n;
    *taps = plan->conv_taps;
    *out_len = plan->conv_len;
    *m = plan->conv_m;
    return 0;
}

int pifft_plan_get_dims(const pifft_plan* plan, uint64_t* n0, uint64_t* n1) {
    if (!plan || !n0 || !n1) return fail("NULL argument");
    *n0 = plan->matrix ? plan->n0 : 1;
    *n1 = plan->matrix ? plan->n1 : plan->real ? plan->real_n : plan->chirp_n ? plan->chirp_n
          : plan->conv ? plan->conv_n : plan->n;
    return 0;
}

int pifft_plan_launch_grid(const pifft_plan* plan, int launch, uint32_t* workgroups) {
    if (!plan || !workgroups) return fail("NULL argument");
    if (launch < 0 || launch >= (int)plan->steps.size()) return fail("launch %d out of range", launch);
    const dim3& g = plan->steps[(size_t)launch].grid;
    *workgroups = g.x * g.y * g.z;
    return 0;
}

int pifft_instance_count(void) { return (int)pass_kernels().size(); }

int pifft_instance_desc(int i, int32_t* desc) {
    if (!desc) return fail("desc is NULL");
    if (i < 0 || i >= (int)pass_kernels().size()) return fail("instance %d out of range", i);
    const PassKernel& k = pass_kernels()[(size_t)i];
    const int32_t d[7] = {k.prec, k.R, k.C, k.mode, k.nts, k.lp, k.vpt};
    memcpy(desc, d, sizeof d);
    return 0;
}

int pifft_instance_found(int i) {
    if (i < 0 || i >= (int)pass_kernels().size()) return fail("instance %d out of range", i);
    return found_log()[(size_t)i].load(std::memory_order_relaxed);
}

int pifft_plan_dry_run_instances(uint64_t n, uint32_t workers, uint32_t first, uint32_t count, uint32_t batch,
                                 int prec, int flags, int32_t* ids, int max_ids) {
    if (!ids && max_ids > 0) return fail("ids is NULL");
    pifft_plan* p = nullptr;
    if (create(&p, n, workers, first, count, batch, prec, -1, flags, true)) return -1;
    const int nl = (int)p->steps.size();
    const PassKernel* base = pass_kernels().data();
    for (int i = 0; i < nl && i < max_ids; i++) {
        const PassKernel* k = p->steps[(size_t)i].pk;
        ids[i] = k ? (int32_t)(k - base) : -1;
    }
    release(p);
    return nl;
}

int pifft_aux_count(void) { return kAuxCount; }

int pifft_aux_desc(int i, int32_t* desc) {
    if (!desc) return fail("desc is NULL");
    if (i < 0 || i >= kAuxCount) return fail("auxiliary kernel %d out of range", i);
    const int32_t d[4] = {kAux[i].family, kAux[i].prec, kAux[i].L, kAux[i].sw};
    memcpy(desc, d, sizeof d);
    return 0;
}

}  // extern "C"

namespace {
// the dry-run plan's launches: registry index (-1: a k_pass launch) and grid size in blocks
int describe_aux(pifft_plan* p, int32_t* ids, uint32_t* grids, int max_ids) {
    const int nl = (int)p->steps.size();
    for (int i = 0; i < nl && i < max_ids; i++) {
        if (ids) ids[i] = (int32_t)aux_index(p->steps[(size_t)i].fn);
        if (grids) grids[i] = p->steps[(size_t)i].grid.x;
    }
    release(p);
    return nl;
}
}  // namespace

extern "C" {

int pifft_plan_dry_run_aux(uint64_t n, uint32_t workers, uint32_t first, uint32_t count, uint32_t batch, int prec,
                           int flags, int32_t* ids, uint32_t* grids, int max_ids) {
    pifft_plan* p = nullptr;
    if (create(&p, n, workers, first, count, batch, prec, -1, flags, true)) return -1;
    return describe_aux(p, ids, grids, max_ids);
}

int pifft_plan_dry_run_aux_real(uint64_t n, uint32_t workers, uint32_t batch, int prec, int direction, int32_t* ids,
                                uint32_t* grids, int max_ids) {
    pifft_plan* p = nullptr;
    if (create_real(&p, n, workers, batch, prec, -1, direction, true)) return -1;
    return describe_aux(p, ids, grids, max_ids);
}

int pifft_plan_get_info(const pifft_plan* p, pifft_plan_info* info) {
    if (!p || !info) return fail("NULL argument");
    memset(info, 0, sizeof *info);
    info->n = p->n;
    info->workers = p->P;
    info->first_worker = p->q0;
    info->num_workers = p->nq;
    info->batch = p->batch;
    info->prec = p->prec;
    info->device = p->device;
    info->flags = p->flags;
    info->local_n = p->m;
    info->in_elems = (uint64_t)p->batch * p->n;
    info->out_elems = out_elems(p);
    info->workspace_bytes = p->bytes_w + p->bytes_ta + p->tw_bytes;
    if (p->real) {  // n: the real length; buffers in complex elements of the precision
        const uint64_t H = p->n;
        info->n = p->real_n;
        info->in_elems = (uint64_t)p->batch * (p->real == 1 ? H : H + 1);
        info->out_elems = (uint64_t)p->batch * (p->real == 1 ? H + 1 : H);
        info->workspace_bytes += p->bytes_z + p->rtw_bytes;
    }
    if (p->matrix) {  // n = n0 n1 (the shape's); a row's length; Z on top of the one W and both chains' tables
        info->local_n = p->n1;
        info->workspace_bytes += p->bytes_z;
    }
    if (p->chirp_n) {  // n = N; the chains' length M; Z, Y and Bt on top of the one W and all the tables
        info->n = p->chirp_n;
        info->in_elems = info->out_elems = (uint64_t)p->batch * p->chirp_n;
        info->workspace_bytes += p->bytes_z + p->bytes_y + p->bytes_bt;
    }
    if (p->conv) {  // n = the signal length, in reals as in_elems / out_elems; local_n = H (the shape's); Z, Y and G
        info->n = p->conv_n;
        info->in_elems = (uint64_t)p->batch * p->conv_n;
        info->out_elems = (uint64_t)p->batch * p->conv_len;
        info->workspace_bytes += p->bytes_z + p->bytes_y + p->bytes_g;
    }
    info->layout = (p->wil ? 1 : 0) | (p->ilv ? 2 : 0);
    info->num_launches = (int)p->steps.size();
    info->num_passes = p->npasses;
    info->tree_launches = p->tree_steps;
    for (int i = 0; i < 8; i++) {
        info->radix[i] = p->radix[i];
        info->lines[i] = p->lines[i];
        info->vpt[i] = p->vpt[i];
    }
    std::vector<const void*> fns;
    for (size_t i = 0; i < p->steps.size() && i < PIFFT_MAX_LAUNCH_INFO; i++) {
        info->launch_bytes[i] = p->steps[i].bytes;
        info->launch_kind[i] = p->steps[i].kind;
        size_t f = 0;
        while (f < fns.size() && fns[f] != p->steps[i].fn) f++;
        if (f == fns.size()) fns.push_back(p->steps[i].fn);
        info->launch_fn[i] = (int32_t)f;
        info->launch_mode[i] = p->steps[i].pk ? p->steps[i].pk->mode : 0;
    }
    return 0;
}

int pifft_plan_kernel_name(const pifft_plan* p, int launch, char* buf, size_t len) {
    if (!p || !buf || len == 0) return fail("NULL argument");
    if (launch < 0 || launch >= (int)p->steps.size()) return fail("launch %d out of range", launch);
    DeviceGuard g(p->device);
    const char* mangled = hipKernelNameRefByPtr(p->steps[(size_t)launch].fn, nullptr);
    if (!mangled) return fail("no kernel name for launch %d", launch);
    int st = 0;
    char* dem = abi::__cxa_demangle(mangled, nullptr, nullptr, &st);
    snprintf(buf, len, "%s", (st == 0 && dem) ? dem : mangled);
    free(dem);
    return 0;
}

// the launch an execution of a PIFFT_PROFILE_SAMPLED run times (or -1):
// odd executions time one launch each, round robin, so every timed dispatch
// follows an untimed one (a timed dispatch delays the next one by ~9 us and
// would isolate it)
int sampled_launch(int k, size_t ns) { return (k & 1) ? (int)(((size_t)k >> 1) % ns) : -1; }

int pifft_execute_device(pifft_plan* p, const void* d_in, void* d_out, void* stream) {
    if (check_buffers(p, d_in, d_out)) return -1;
    DeviceGuard g(p->device);
    hipStream_t st = (hipStream_t)stream;  // NULL = the default stream
    const size_t ns = p->steps.size();
    if (p->prof_used >= p->prof_steps) return launch_steps(p, d_in, d_out, st, nullptr);
    const int k = p->prof_used++;
    if (p->prof_mode == PIFFT_PROFILE_ALL) return launch_steps(p, d_in, d_out, st, &p->prof_ev[(size_t)k * 2 * ns]);
    const int li = sampled_launch(k, ns);
    for (size_t i = 0; i < ns; i++) {
        hipEvent_t* e = (int)i == li ? &p->prof_ev[(size_t)k * 2] : nullptr;
        if (launch_step(p, p->steps[i], d_in, d_out, st, e ? e[0] : nullptr, e ? e[1] : nullptr)) return -1;
    }
    return 0;
}

int pifft_launch_loop(pifft_plan* p, const int* launches, int nlaunches, int reps, const void* d_in, void* d_out,
                      void* stream, float* mean_ms) {
    if (check_buffers(p, d_in, d_out)) return -1;
    if (!launches || nlaunches < 1 || reps < 1 || !mean_ms) return fail("bad arguments");
    for (int j = 0; j < nlaunches; j++)
        if (launches[j] < 0 || (size_t)launches[j] >= p->steps.size())
            return fail("launch %d out of range (plan has %zu)", launches[j], p->steps.size());
    DeviceGuard g(p->device);
    hipStream_t st = (hipStream_t)stream;
    auto rounds = [&](int r) -> int {
        for (int k = 0; k < r; k++)
            for (int j = 0; j < nlaunches; j++)
                if (launch_step(p, p->steps[(size_t)launches[j]], d_in, d_out, st)) return -1;
        return 0;
    };
    // the plan's own event pair, as markers around the loop (p->ev holds >= 2)
    if (rounds(2)) return -1;
    HIPCHK(hipEventRecord(p->ev[0], st));
    if (rounds(reps)) return -1;
    HIPCHK(hipEventRecord(p->ev[1], st));
    if (launch_steps(p, d_in, d_out, st, nullptr)) return -1;  // d_out = the plan's result again
    HIPCHK(hipEventSynchronize(p->ev[1]));
    float ms = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, p->ev[0], p->ev[1]));
    HIPCHK(hipStreamSynchronize(st));
    *mean_ms = ms / (float)((size_t)reps * (size_t)nlaunches);
    return 0;
}

#ifdef PIFFT_WG_CLOCK
// Diagnostics build only (-DPIFFT_WG_CLOCK, tools/wg_clock.py; not in
// include/pifft.h): `warm` full executions, then launches 0 .. launch-1 as
// usual and `launch` with every workgroup recording its entry and
// stores-done wall clock, hardware id and per-stage stamps
// (PIFFT_WGC_WORDS words per workgroup, PassArgs::wg_clock) into
// host[0 .. min(PIFFT_WGC_WORDS grid, max_words)).  Returns the workgroup count (or -1);
// *wall_hz = the wall clock's rate.  Synchronous.
int pifft_debug_wg_clock(pifft_plan* p, int launch, const void* d_in, void* d_out, void* stream, int warm,
                         unsigned long long* host, size_t max_words, unsigned long long* wall_hz) {
    if (check_buffers(p, d_in, d_out)) return -1;
    if (launch < 0 || (size_t)launch >= p->steps.size()) return fail("launch %d out of range", launch);
    const Step& s = p->steps[(size_t)launch];
    if (s.kind != STEP_PASS && s.kind != STEP_TREE_PASS) return fail("launch %d is not a pass", launch);
    DeviceGuard g(p->device);
    hipStream_t st = (hipStream_t)stream;
    const size_t nwg = (size_t)s.grid.x * s.grid.y * s.grid.z, words = PIFFT_WGC_WORDS * nwg;
    unsigned long long* clk = nullptr;
    HIPCHK(hipMalloc(&clk, words * sizeof(unsigned long long)));
    HIPCHK(hipMemset(clk, 0, words * sizeof(unsigned long long)));  // (stamps a pass does not reach stay 0)
    int rc = 0;
    for (int k = 0; k < warm && rc == 0; k++) rc = launch_steps(p, d_in, d_out, st, nullptr);
    for (int i = 0; i < launch && rc == 0; i++) rc = launch_step(p, p->steps[(size_t)i], d_in, d_out, st);
    if (rc == 0) {
        p->dbg_clk = clk;
        rc = launch_step(p, s, d_in, d_out, st);
        p->dbg_clk = nullptr;
    }
    if (rc == 0 && hipStreamSynchronize(st) != hipSuccess) rc = fail("hipStreamSynchronize failed");
    if (rc == 0 && hipMemcpy(host, clk, std::min(words, max_words) * sizeof(unsigned long long),
                             hipMemcpyDeviceToHost) != hipSuccess)
        rc = fail("hipMemcpy failed");
    int khz = 0;
    if (rc == 0 && hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, p->device) != hipSuccess)
        rc = fail("no wall clock rate");
    (void)hipFree(clk);
    if (rc) return -1;
    *wall_hz = (unsigned long long)khz * 1000ull;
    return (int)nwg;
}
#endif

int pifft_plan_tune_workspace(pifft_plan* p, const void* d_in, void* d_out, void* stream, int tries,
                              float* best_ms) {
    if (check_buffers(p, d_in, d_out)) return -1;
    if (device_only(p)) return fail("pifft_plan_tune_workspace: %s", device_only(p));
    if (tries < 1) return fail("tries must be >= 1");
    DeviceGuard g(p->device);
    hipStream_t st = (hipStream_t)stream;
    if (!p->buf[BUF_W] || tries == 1) {  // nothing to place
        if (best_ms) *best_ms = 0.0f;
        return 0;
    }
    hipEvent_t e[2];
    HIPCHK(hipEventCreateWithFlags(&e[0], kTimingEventFlags));
    if (hipEventCreateWithFlags(&e[1], kTimingEventFlags) != hipSuccess) {
        (void)hipEventDestroy(e[0]);
        return fail("hipEventCreate failed");
    }
    // mean of 3 executions after one warm-up, with the plan's current workspace
    auto timed = [&](float& ms) -> int {
        if (launch_steps(p, d_in, d_out, st, nullptr)) return -1;
        HIPCHK(hipEventRecord(e[0], st));
        for (int r = 0; r < 3; r++)
            if (launch_steps(p, d_in, d_out, st, nullptr)) return -1;
        HIPCHK(hipEventRecord(e[1], st));
        HIPCHK(hipEventSynchronize(e[1]));
        HIPCHK(hipEventElapsedTime(&ms, e[0], e[1]));
        ms /= 3.0f;
        return 0;
    };
    int rc = 0;
    float best = 0.0f;
    if (timed(best)) rc = -1;
    // every losing workspace stays allocated until the end, so each try lands
    // somewhere new (a freed range would come straight back from hipMalloc)
    std::vector<void*> losers;
    for (int t = 1; t < tries && rc == 0; t++) {
        void* keep = p->buf[BUF_W];
        void* fresh = nullptr;
        // the losers stay allocated until the end: try only while the device
        // keeps room for another workspace and 4 GiB beyond this one (other
        // processes on the GPU, e.g. bench.py's same-device rehearsal ranks,
        // allocate concurrently)
        size_t mfree = 0, mtotal = 0;
        if (hipMemGetInfo(&mfree, &mtotal) != hipSuccess || mfree < 2 * p->bytes_w + (4ull << 30)) {
            (void)hipGetLastError();
            break;
        }
        if (hipMalloc(&fresh, p->bytes_w) != hipSuccess) {
            (void)hipGetLastError();
            break;  // no room for another workspace: keep the best so far
        }
        p->buf[BUF_W] = fresh;
        float ms = 0.0f;
        if (timed(ms)) {
            rc = -1;
            p->buf[BUF_W] = keep;
            losers.push_back(fresh);
        } else if (ms < best) {
            best = ms;
            losers.push_back(keep);
        } else {
            p->buf[BUF_W] = keep;
            losers.push_back(fresh);
        }
    }
    (void)hipStreamSynchronize(st);
    for (void* w : losers) (void)hipFree(w);
    (void)hipEventDestroy(e[0]);
    (void)hipEventDestroy(e[1]);
    if (best_ms) *best_ms = best;
    return rc;
}

int pifft_profile_start(pifft_plan* p, int steps, int mode) {
    if (!p || steps < 0) return fail("bad arguments");
    if (mode != PIFFT_PROFILE_ALL && mode != PIFFT_PROFILE_SAMPLED) return fail("unknown profile mode %d", mode);
    DeviceGuard g(p->device);
    const size_t need = (size_t)steps * 2 * (mode == PIFFT_PROFILE_ALL ? p->steps.size() : 1);
    while (p->prof_ev.size() < need) {
        hipEvent_t e;
        HIPCHK(hipEventCreateWithFlags(&e, kTimingEventFlags));
        p->prof_ev.push_back(e);
    }
    p->prof_steps = steps;
    p->prof_used = 0;
    p->prof_mode = mode;
    return 0;
}

int pifft_profile_read(pifft_plan* p, float* launch_ms_sum, int* launch_samples, int max_launches) {
    if (!p) return fail("plan is NULL");
    DeviceGuard g(p->device);
    const size_t ns = p->steps.size();
    const int used = p->prof_used;
    p->prof_steps = p->prof_used = 0;  // profiling stops, also on an error below
    std::vector<float> sum(ns, 0.0f), ms;
    std::vector<int> cnt(ns, 0);
    for (int k = 0; k < used; k++) {
        // each execution's own events: the executions may have run on different streams
        if (p->prof_mode == PIFFT_PROFILE_ALL) {
            if (read_launch_ms(ns, &p->prof_ev[(size_t)k * 2 * ns], ms)) return -1;
            for (size_t i = 0; i < ns; i++) sum[i] += ms[i], cnt[i]++;
        } else {
            const int li = sampled_launch(k, ns);
            if (li < 0) continue;
            hipEvent_t* e = &p->prof_ev[(size_t)k * 2];
            float t = 0.0f;
            HIPCHK(hipEventSynchronize(e[1]));
            HIPCHK(hipEventElapsedTime(&t, e[0], e[1]));
            sum[(size_t)li] += t;
            cnt[(size_t)li]++;
        }
    }
    for (int i = 0; i < max_launches && i < (int)ns; i++) {
        if (launch_ms_sum) launch_ms_sum[i] = sum[(size_t)i];
        if (launch_samples) launch_samples[i] = cnt[(size_t)i];
    }
    return used;
}

int pifft_execute_device_timed(pifft_plan* p, const void* d_in, void* d_out, void* stream,
                               float* launch_ms, int max_launches) {
    if (check_buffers(p, d_in, d_out)) return -1;
    DeviceGuard g(p->device);
    hipStream_t st = (hipStream_t)stream;  // NULL = the default stream
    std::vector<float> ms;
    if (run_timed(p, d_in, d_out, st, ms)) return -1;
    // (fence-free timing events: the output is complete and visible once the
    // stream itself has drained)
    HIPCHK(hipStreamSynchronize(st));
    if (launch_ms)
        for (int i = 0; i < max_launches && i < (int)ms.size(); i++) launch_ms[i] = ms[i];
    return 0;
}

int pifft_execute(pifft_plan* p, const void* host_in, void* host_out, double* ms1, double* ms2) {
    if (p && device_only(p)) return fail("pifft_execute: %s", device_only(p));
    return pifft_execute_group(&p, 1, host_in, host_out, ms1, ms2);
}

int pifft_execute_group(pifft_plan** plans, int np, const void* host_in, void* host_out,
                        double* ms1, double* ms2) {
    if (!plans || np <= 0) return fail("no plans");
    if (!host_in) return fail("host_in is NULL");
    for (int i = 0; i < np; i++) {
        if (!plans[i]) return fail("plan %d is NULL", i);
        if (device_only(plans[i])) return fail("pifft_execute_group: %s", device_only(plans[i]));
        if (plans[i]->n != plans[0]->n || plans[i]->batch != plans[0]->batch ||
            plans[i]->prec != plans[0]->prec)
            return fail("plans of a group must share n, batch and precision");
        if (plans[i]->inverse != plans[0]->inverse)
            return fail("plans of a group must share the direction (PIFFT_INVERSE on all or none)");
    }
    // stage the input on every device (outside the timed region, like the
    // reference's per-worker memcpy of the whole input, CPU.c:407): one copy
    // over PCIe to the first plan's device, then a broadcast device to device
    // (hipMemcpyPeerAsync over xGMI, all destinations concurrently) instead
    // of one PCIe copy per GPU
    const size_t in_bytes = (size_t)plans[0]->batch * plans[0]->n * plans[0]->esz;
    {
        pifft_plan* p0 = plans[0];
        DeviceGuard g(p0->device);
        if (ensure_host_staging(p0)) return -1;
        HIPCHK(hipMemcpyAsync(p0->d_hin, host_in, in_bytes, hipMemcpyHostToDevice, p0->stream));
        HIPCHK(hipStreamSynchronize(p0->stream));
    }
    // (a failure part-way waits for the broadcast copies already enqueued --
    // they read plans[0]'s staging buffer, which the next call overwrites)
    auto broadcast = [&](int i) -> int {
        pifft_plan* p = plans[i];
        DeviceGuard g(p->device);
        if (ensure_host_staging(p)) return -1;
        if (enable_peer(p, plans[0]->device)) return -1;
        if (fault_at("broadcast"))
            return fail("hipMemcpyPeerAsync(%d <- %d): injected fault (PIFFT_FAULT=broadcast)", p->device,
                        plans[0]->device);
        HIPCHK(hipMemcpyPeerAsync(p->d_hin, p->device, plans[0]->d_hin, plans[0]->device, in_bytes, p->stream));
        return 0;
    };
    for (int i = 1; i < np; i++) {
        if (!broadcast(i)) continue;
        const std::string msg = g_err;
        for (int k = 1; k < i; k++) {
            DeviceGuard g(plans[k]->device);
            (void)hipStreamSynchronize(plans[k]->stream);
        }
        (void)hipGetLastError();
        g_err = msg;
        return -1;
    }
    for (int i = 1; i < np; i++) {
        DeviceGuard g(plans[i]->device);
        HIPCHK(hipStreamSynchronize(plans[i]->stream));
    }
    // launch all GPUs, then wait for all (stage markers: wall time per stage)
    for (int i = 0; i < np; i++) {
        pifft_plan* p = plans[i];
        DeviceGuard g(p->device);
        if (launch_stage_marked(p, p->d_hin, p->d_hout)) return -1;
    }
    double t1 = 0, t2 = 0;
    for (int i = 0; i < np; i++) {
        pifft_plan* p = plans[i];
        DeviceGuard g(p->device);
        double a, b;
        if (read_stage_marked(p, &a, &b)) return -1;
        // the timing events skip the system-scope fence: the stream itself is
        // waited for before anything reads the result on the host
        HIPCHK(hipStreamSynchronize(p->stream));
        if (a + b > t1 + t2) {  // the slowest GPU sets the job's time
            t1 = a;
            t2 = b;
        }
    }
    if (ms1) *ms1 = t1;
    if (ms2) *ms2 = t2;
    if (host_out) {
        if (np > 1 && check_cover(plans, np, true) == 0) {
            // the whole transform over several plans: gather on the first
            // plan's device (pifft_allgather) into a result buffer held for
            // this call only -- not the input staging copy, which
            // pifft_execute_group_kernel_times re-runs the plans on, and not
            // a persistent one (it would add N to the first device's
            // footprint for the plan's life) -- and copy back once
            pifft_plan* p = plans[0];
            const size_t nat_bytes = (size_t)p->batch * p->n * p->esz;
            void* d_nat = nullptr;
            {
                DeviceGuard g(p->device);
                HIPCHK(hipMalloc(&d_nat, nat_bytes));
            }
            std::vector<const void*> sl(np);
            std::vector<void*> nat(np, nullptr);
            for (int i = 0; i < np; i++) sl[i] = plans[i]->d_hout;
            nat[0] = d_nat;
            int rc = gather_group(plans, np, sl.data(), nat.data(), nullptr);
            DeviceGuard g(p->device);
            if (rc == 0) {
                const hipError_t e = hipMemcpy(host_out, d_nat, nat_bytes, hipMemcpyDeviceToHost);
                if (e != hipSuccess) rc = fail("hipMemcpy of the gathered result: %s", hipGetErrorString(e));
            }
            (void)hipFree(d_nat);  // (synchronizes: no gather copy still writes it)
            return rc;
        }
        for (int i = 0; i < np; i++) {
            pifft_plan* p = plans[i];
            DeviceGuard g(p->device);
            // natural order, and the reference's scratch order (whole segments),
            // land in host_out as they are: straight device-to-host copies (no
            // host-side staging copy: that single-threaded 4 GiB memcpy was half
            // of a 2^28 fp64 call, profiles/r02_host_boundary.log)
            if (p->natural) {
                HIPCHK(hipMemcpy(host_out, p->d_hout, (size_t)p->batch * p->n * p->esz, hipMemcpyDeviceToHost));
                continue;
            }
            if (p->bitrev) {
                const uint64_t M = p->m;
                for (uint32_t bt = 0; bt < p->batch; bt++)
                    HIPCHK(hipMemcpy((char*)host_out + ((uint64_t)bt * p->n + (uint64_t)p->q0 * M) * p->esz,
                                     (const char*)p->d_hout + (uint64_t)bt * p->nq * M * p->esz,
                                     (size_t)p->nq * M * p->esz, hipMemcpyDeviceToHost));
                continue;
            }
            const size_t bytes = (size_t)out_elems(p) * p->esz;
            p->host_tmp.resize(bytes);
            HIPCHK(hipMemcpy(p->host_tmp.data(), p->d_hout, bytes, hipMemcpyDeviceToHost));
            scatter_to_host(p, p->host_tmp.data(), (char*)host_out);
        }
    }
    return 0;
}

int pifft_execute_group_kernel_times(pifft_plan** plans, int np, double* ms1, double* ms2) {
    if (!plans || np <= 0) return fail("no plans");
    for (int i = 0; i < np; i++) {
        if (!plans[i]) return fail("plan %d is NULL", i);
        if (device_only(plans[i])) return fail("pifft_execute_group_kernel_times: %s", device_only(plans[i]));
        if (!plans[i]->d_hin || !plans[i]->d_hout) return fail("plan %d: no staged input (call pifft_execute_group first)", i);
    }
    for (int i = 0; i < np; i++) {
        pifft_plan* p = plans[i];
        DeviceGuard g(p->device);
        if (launch_steps(p, p->d_hin, p->d_hout, p->stream, p->ev.data())) return -1;
    }
    double t1 = 0, t2 = 0;
    for (int i = 0; i < np; i++) {
        pifft_plan* p = plans[i];
        DeviceGuard g(p->device);
        std::vector<float> ms;
        if (read_launch_ms(p->steps.size(), p->ev.data(), ms)) return -1;
        HIPCHK(hipStreamSynchronize(p->stream));
        double a, b;
        stage_split(p, ms, &a, &b);
        if (a + b > t1 + t2) {
            t1 = a;
            t2 = b;
        }
    }
    if (ms1) *ms1 = t1;
    if (ms2) *ms2 = t2;
    return 0;
}

int pifft_generate_device(void* d_x, uint64_t count, uint64_t n, uint64_t seed, uint64_t first,
                          int prec, void* stream) {
    if (!d_x) return fail("NULL buffer");
    if (prec != PIFFT_F32 && prec != PIFFT_F64) return fail("bad precision");
    if (count == 0) return 0;
    double scale = sqrt((double)n);
    void* args[] = {&d_x, &count, &scale, &seed, &first};
    HIPCHK(hipLaunchKernel(aux_fn(PIFFT_AUX_GENERATE, prec), dim3(stride_grid(count)), dim3(256), args, 0,
                           (hipStream_t)stream));
    return 0;
}

int pifft_interleave_device(const void* d_slices, void* d_out, uint64_t n, uint32_t workers,
                            uint32_t batch, int prec, void* stream) {
    if (!d_slices || !d_out || d_slices == d_out) return fail("bad buffers");
    if (n < 2 || !is_pow2(n) || !workers || !is_pow2(workers) || workers > n) return fail("bad n/workers");
    return launch_interleave(d_slices, d_out, n, workers, batch, prec, (hipStream_t)stream);
}

int pifft_allgather(pifft_plan* const* plans, int nplans, const void* const* d_slices, void* const* d_natural,
                    double* ms) {
    for (int i = 0; plans && i < nplans; i++)
        if (plans[i] && device_only(plans[i])) return fail("pifft_allgather: %s", device_only(plans[i]));
    return gather_group(plans, nplans, d_slices, d_natural, ms);
}

int pifft_tree_device(pifft_plan* p, const void* d_in, void* d_seg, void* stream) {
    if (check_buffers(p, d_in, d_seg)) return -1;
    if (device_only(p)) return fail("pifft_tree_device: %s", device_only(p));
    if (p->inverse) return fail("pifft_tree_device: forward plans only (the reference's tree)");
    DeviceGuard g(p->device);
    hipStream_t st = (hipStream_t)stream;  // NULL = the default stream
    if (p->tree_only.empty()) {  // P == 1: the segment is the input
        HIPCHK(hipMemcpyAsync(d_seg, d_in, (size_t)p->batch * p->n * p->esz, hipMemcpyDeviceToDevice, st));
        return 0;
    }
    for (const Step& s : p->tree_only)
        if (launch_step(p, s, d_in, d_seg, st)) return -1;
    return 0;
}

}  // extern "C"
