// The convolution plans' per-thread code (csrc/pifft_conv.h) on the host: every
// thread of a grid-stride launch is run in turn over heap buffers of exactly
// the sizes a plan passes, so a host sanitizer sees every index the kernels
// would form (its red zones sit on both sides of every buffer).
//
//   conv stream <n> <taps> <batch> <32|64> <threads, 0: the library's> <misalign>
//       k_conv_pad, k_conv_crop and k_conv_filter (forward and back to front)
//       against plain loops; every output value stored, the pad zeros included.
//       misalign shifts the caller-side buffers by that many reals (guarded
//       values before them), so rows start at every residue of 16 B.
//       {"bad": values that differ in bits, "unwritten": .., "guard": ..}
//   conv pair <H> <batch> <32|64> <threads, 0: the library's>
//       k_conv_pair in place against real_unit<0> (k_r2c_post), a plain complex
//       product and real_unit<1> (k_c2r_pre) run one after the other over
//       buffers of their own: bit for bit.  {"bad": .., "unwritten": ..}
//   conv formula <n> <taps> <32|64> <0 convolve | 1 correlate>
//       filter, a naive O(H^2) DFT and the R2C fix-up for G; pad, a naive DFT,
//       pair, a naive inverse and crop -- against the direct long-double sum.
//       {"err": rel-L2 in units of eps, "m": M}
#include "../../cs87project-msolano2_amd/csrc/pifft_chirp.h"
#include "../../cs87project-msolano2_amd/csrc/pifft_conv.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace pifft;
typedef long double ld;

static const ld kPi = 3.141592653589793238462643383279502884L;

static void* alloc16(size_t bytes) {  // exactly `bytes`, 16-B aligned
    void* p = nullptr;
    if (posix_memalign(&p, 16, bytes ? bytes : 1)) exit(3);
    return p;
}
static uint64_t rng = 0x9E3779B97F4A7C15ull;
static uint64_t draw64() {
    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
    return rng;
}
static double draw() { return (double)(draw64() >> 11) * 0x1.0p-53 * 2.0 - 1.0; }

// the planner's two_level(tb, M), in precision T
template <typename T>
struct Table {
    cx<T>*lo, *hi;
    uint32_t h;
    explicit Table(uint64_t M) {
        int logm = 0;
        while ((1ull << logm) < M) logm++;
        h = (uint32_t)((logm + 1) / 2);
        const uint64_t nlo = 1ull << h, nhi = (M >> h) ? (M >> h) : 1;
        lo = (cx<T>*)alloc16(nlo * sizeof(cx<T>));
        hi = (cx<T>*)alloc16(nhi * sizeof(cx<T>));
        for (uint64_t e = 0; e < nlo; e++) lo[e] = root(e % M, M);
        for (uint64_t e = 0; e < nhi; e++) hi[e] = root((e << h) % M, M);
    }
    ~Table() {
        free(lo);
        free(hi);
    }
    static cx<T> root(uint64_t x, uint64_t M) {
        const ld ang = 2 * kPi * ((ld)x / (ld)M);
        return {(T)(double)cosl(ang), (T)(double)(-sinl(ang))};  // (TableBuilder::put: through double)
    }
};

template <typename V>
static bool same(V a, V b) {
    return memcmp(&a, &b, sizeof a) == 0;
}

// the launch's thread count: as build_conv sizes it, or `thr` threads in all --
// fewer than the work items, so that the threads make second and later trips
static uint64_t threads_of(uint64_t total, uint64_t thr) {
    if (thr) return thr;
    const uint64_t blocks = (total + 255) / 256, cap = 262144;
    return (blocks < cap ? (blocks ? blocks : 1) : cap) * 256;
}

template <int KIND, typename T>
static void launch(uint64_t len, uint64_t H, uint32_t batch, uint64_t cap, const Table<T>* t, const void* in, void* out,
                   const void* g, uint32_t rev = 0) {
    const uint64_t threads = threads_of((uint64_t)batch * conv_units<T>(KIND, len, H), cap);
    ConvArgs a = conv_args<T>(KIND, len, H, batch, threads);
    if (t) a.tw_lo = t->lo, a.tw_hi = t->hi, a.tw_h = t->h;
    a.in = in;
    a.out = out;
    a.g = g;
    a.rev = rev;
    for (uint64_t gid = 0; gid < threads; gid++) conv_thread<KIND, T>(a, gid);
}

template <typename T>
static int run_stream(uint64_t n, uint64_t taps, uint32_t batch, uint64_t cap, uint64_t mis) {
    const uint64_t L = n + taps - 1, M = conv_length(n, taps), H = M / 2;
    const T unset = (T)-12345.0;
    uint64_t bad = 0, unwritten = 0, guard = 0;
    // the caller's rows: batch * n reals exactly (+ mis guarded reals in front)
    T* x0 = (T*)alloc16((batch * n + mis) * sizeof(T));
    T* x = x0 + mis;
    for (uint64_t i = 0; i < batch * n; i++) x[i] = (T)draw();
    T* z = (T*)alloc16(batch * M * sizeof(T));
    // --- pad ---
    for (uint64_t i = 0; i < batch * M; i++) z[i] = unset;
    launch<CONV_PAD, T>(n, H, batch, cap, nullptr, x, z, nullptr);
    for (uint32_t b = 0; b < batch; b++)
        for (uint64_t j = 0; j < M; j++) {
            const T got = z[b * M + j];
            unwritten += same(got, unset);
            bad += !same(got, j < n ? x[b * n + j] : (T)0);
        }
    // --- crop: Z rows of fresh values -> rows of L ---
    for (uint64_t i = 0; i < batch * M; i++) z[i] = (T)draw();
    T* y0 = (T*)alloc16((batch * L + mis) * sizeof(T));
    T* y = y0 + mis;
    for (uint64_t i = 0; i < batch * L + mis; i++) y0[i] = unset;
    launch<CONV_CROP, T>(L, H, batch, cap, nullptr, z, y, nullptr);
    for (uint64_t i = 0; i < mis; i++) guard += !same(y0[i], unset);
    for (uint32_t b = 0; b < batch; b++)
        for (uint64_t j = 0; j < L; j++) {
            const T got = y[b * L + j];
            unwritten += same(got, unset);
            bad += !same(got, z[b * M + j]);
        }
    // --- filter: taps reals exactly, forward and back to front, into row 0 of Z ---
    T* h0 = (T*)alloc16((taps + mis) * sizeof(T));
    T* h = h0 + mis;
    for (uint64_t i = 0; i < taps; i++) h[i] = (T)draw();
    const T scale = (T)(1.0 / (double)M);
    for (uint32_t rev = 0; rev < 2; rev++) {
        std::vector<T> before(z, z + batch * M);
        for (uint64_t j = 0; j < M; j++) z[j] = unset;
        launch<CONV_FILTER, T>(taps, H, 1, cap, nullptr, h, z, nullptr, rev);
        for (uint64_t j = 0; j < M; j++) {
            unwritten += same(z[j], unset);
            bad += !same(z[j], j < taps ? (T)(h[rev ? taps - 1 - j : j] * scale) : (T)0);
        }
        for (uint64_t i = M; i < batch * M; i++) guard += !same(z[i], before[i]);  // (the other rows untouched)
    }
    printf("{\"bad\": %llu, \"unwritten\": %llu, \"guard\": %llu}\n", (unsigned long long)bad,
           (unsigned long long)unwritten, (unsigned long long)guard);
    free(x0);
    free(z);
    free(y0);
    free(h0);
    return 0;
}

// k_r2c_post / k_c2r_pre over their own buffers, every thread of the launch in turn
template <int DIR, typename T>
static void real_launch(uint64_t H, uint32_t batch, uint64_t cap, const Table<T>& t, const void* in, void* out) {
    RealArgs a{};
    a.in = in;
    a.out = out;
    a.tw_lo = t.lo, a.tw_hi = t.hi, a.tw_h = t.h;
    a.batch = batch;
    a.h = H;
    a.units = real_units<T>(H);
    const uint64_t threads = threads_of((uint64_t)batch * a.units, cap);
    a.step_rows = threads / a.units;
    a.step_units = threads % a.units;
    for (uint64_t gid = 0; gid < threads; gid++) real_thread<DIR, T>(a, gid);
}

template <typename T>
static int run_pair(uint64_t H, uint32_t batch, uint64_t cap) {
    Table<T> t(2 * H);
    const T unset = (T)-12345.0;
    const cx<T> U{unset, unset};
    uint64_t bad = 0, unwritten = 0;
    cx<T>* y = (cx<T>*)alloc16(batch * H * sizeof(cx<T>));
    cx<T>* g = (cx<T>*)alloc16((H + 1) * sizeof(cx<T>));
    for (uint64_t i = 0; i < batch * H; i++) y[i] = {(T)draw(), (T)draw()};
    for (uint64_t i = 0; i <= H; i++) g[i] = {(T)draw(), (T)draw()};
    g[0].im = g[H].im = (T)0;  // (as k_r2c_post leaves them)
    // the three launches, one after the other
    cx<T>* X = (cx<T>*)alloc16(batch * (H + 1) * sizeof(cx<T>));
    cx<T>* want = (cx<T>*)alloc16(batch * H * sizeof(cx<T>));
    for (uint64_t i = 0; i < batch * (H + 1); i++) X[i] = U;
    for (uint64_t i = 0; i < batch * H; i++) want[i] = U;
    real_launch<0, T>(H, batch, cap, t, y, X);
    for (uint32_t b = 0; b < batch; b++)
        for (uint64_t k = 0; k <= H; k++) {
            unwritten += same(X[b * (H + 1) + k], U);
            X[b * (H + 1) + k] = chirp_mul(X[b * (H + 1) + k], g[k]);
        }
    real_launch<1, T>(H, batch, cap, t, X, want);
    // the fused launch, in place
    launch<CONV_PAIR, T>(0, H, batch, cap, &t, nullptr, y, g);
    for (uint64_t i = 0; i < batch * H; i++) {
        unwritten += same(want[i], U);
        bad += !same(y[i], want[i]);
    }
    printf("{\"bad\": %llu, \"unwritten\": %llu}\n", (unsigned long long)bad, (unsigned long long)unwritten);
    free(y);
    free(g);
    free(X);
    free(want);
    return 0;
}

// out[k] = sum_j in[j] e^{sign 2 pi i jk/H}, exact up to its one rounding to T
template <typename T>
static void naive_dft(cx<T>* v, uint64_t H, int sign) {
    std::vector<cx<T>> in(v, v + H);
    for (uint64_t k = 0; k < H; k++) {
        ld re = 0, im = 0;
        for (uint64_t j = 0; j < H; j++) {
            const ld ang = 2 * kPi * ((ld)((j * k) % H) / (ld)H), c = cosl(ang), s = sign * sinl(ang);
            re += (ld)in[j].re * c - (ld)in[j].im * s;
            im += (ld)in[j].re * s + (ld)in[j].im * c;
        }
        v[k] = {(T)re, (T)im};
    }
}

template <typename T>
static int run_formula(uint64_t n, uint64_t taps, int correlate) {
    const uint64_t L = n + taps - 1, M = conv_length(n, taps), H = M / 2;
    Table<T> t(M);
    T* x = (T*)alloc16(n * sizeof(T));
    T* h = (T*)alloc16(taps * sizeof(T));
    for (uint64_t i = 0; i < n; i++) x[i] = (T)draw();
    for (uint64_t i = 0; i < taps; i++) h[i] = (T)draw();
    cx<T>* z = (cx<T>*)alloc16(H * sizeof(cx<T>));
    cx<T>* g = (cx<T>*)alloc16((H + 1) * sizeof(cx<T>));
    T* y = (T*)alloc16(L * sizeof(T));
    // G as pifft_conv_set_filter fixes it
    launch<CONV_FILTER, T>(taps, H, 1, 262144, nullptr, h, z, nullptr, (uint32_t)correlate);
    naive_dft(z, H, -1);
    real_launch<0, T>(H, 1, 262144, t, z, g);
    // an execution
    launch<CONV_PAD, T>(n, H, 1, 262144, nullptr, x, z, nullptr);
    naive_dft(z, H, -1);
    launch<CONV_PAIR, T>(0, H, 1, 262144, &t, nullptr, z, g);
    naive_dft(z, H, +1);
    launch<CONV_CROP, T>(L, H, 1, 262144, nullptr, z, y, nullptr);
    ld num = 0, den = 0;
    for (uint64_t j = 0; j < L; j++) {
        ld s = 0;
        for (uint64_t i = 0; i < taps; i++)
            if (j >= i && j - i < n) s += (ld)x[j - i] * (ld)h[correlate ? taps - 1 - i : i];
        num += ((ld)y[j] - s) * ((ld)y[j] - s);
        den += s * s;
    }
    const ld eps = sizeof(T) == 4 ? 0x1.0p-23L : 0x1.0p-52L;
    printf("{\"err\": %.4Lf, \"m\": %llu}\n", sqrtl(num / den) / eps, (unsigned long long)M);
    free(x);
    free(h);
    free(z);
    free(g);
    free(y);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    if (!strcmp(argv[1], "stream") && argc == 8) {
        const uint64_t n = strtoull(argv[2], nullptr, 10), taps = strtoull(argv[3], nullptr, 10);
        const uint32_t batch = (uint32_t)atoi(argv[4]);
        const int prec = atoi(argv[5]);
        const uint64_t cap = strtoull(argv[6], nullptr, 10), mis = strtoull(argv[7], nullptr, 10);
        if (n < 1 || taps < 1 || batch < 1 || n + taps > (1 << 16) || mis > 3) return 2;
        return prec == 64 ? run_stream<double>(n, taps, batch, cap, mis) : run_stream<float>(n, taps, batch, cap, mis);
    }
    if (!strcmp(argv[1], "pair") && argc == 6) {
        const uint64_t H = strtoull(argv[2], nullptr, 10);
        const uint32_t batch = (uint32_t)atoi(argv[3]);
        const uint64_t cap = strtoull(argv[5], nullptr, 10);
        if (H < 2 || H > (1 << 16) || (H & (H - 1)) || batch < 1) return 2;
        return atoi(argv[4]) == 64 ? run_pair<double>(H, batch, cap) : run_pair<float>(H, batch, cap);
    }
    if (!strcmp(argv[1], "formula") && argc == 6) {
        const uint64_t n = strtoull(argv[2], nullptr, 10), taps = strtoull(argv[3], nullptr, 10);
        if (n < 1 || taps < 1 || n + taps - 1 > 64) return 2;
        return atoi(argv[4]) == 64 ? run_formula<double>(n, taps, atoi(argv[5]))
                                   : run_formula<float>(n, taps, atoi(argv[5]));
    }
    return 2;
}
