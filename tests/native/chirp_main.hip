// The chirp plans' per-thread code (csrc/pifft_chirp.h) on the host: every
// thread of a grid-stride launch is run in turn over heap buffers of exactly
// the sizes a plan passes, so a host sanitizer sees every index the kernels
// would form (its red zones sit on both sides of every buffer).
//
//   chirp kernels <N> <batch> <32|64> <grid cap, 0: the library's> <misalign>
//       k_chirp_pre (SW 0, 1), k_spectrum_mul and k_chirp_post (SW 0, 2) against
//       the same arithmetic done value by value with r = j^2 mod 2N taken in
//       unsigned __int128; every output value stored, the pad zeros included.
//       misalign = 1 shifts the caller-side buffers by one complex value (one
//       guarded value before them), so the rows 16-B aligned in a plan's buffers
//       are the misaligned ones here.
//       {"bad": values that differ in bits, "unwritten": .., "guard": ..}
//   chirp sqmod <N> <samples, 0: every j < N>
//       chirp_sq_mod and chirp_sq_next against unsigned __int128.  {"bad": ..}
//   chirp tw <N> <32|64>
//       the two-level w_2N^r against long double e^{-i pi r/N}, every r < 2N (2^20
//       sampled r above that many).  {"err": the largest |difference| in units of eps}
//   chirp formula <N> <32|64> <0 forward | 1 swapped>
//       pre, a naive O(M^2) DFT, mul, a naive inverse and post -- Bt from
//       chirp_fill_one, a naive fp64-rounded DFT and chirp_bt_one -- against the
//       direct DFT.  {"err": rel-L2 in units of eps}
#include "../../cs87project-msolano2_amd/csrc/pifft_chirp.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace pifft;
typedef long double ld;
typedef unsigned __int128 u128;

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

// the planner's two_level_any(tb, 2N), in precision T
template <typename T>
struct Table {
    cx<T>*lo, *hi;
    uint32_t h;
    explicit Table(uint64_t N) {
        const uint64_t L = 2 * N;
        int logl = 0;
        while ((1ull << logl) < L) logl++;
        h = (uint32_t)((logl + 1) / 2);
        const uint64_t nlo = 1ull << h, nhi = (L + nlo - 1) >> h;
        lo = (cx<T>*)alloc16(nlo * sizeof(cx<T>));
        hi = (cx<T>*)alloc16(nhi * sizeof(cx<T>));
        for (uint64_t e = 0; e < nlo; e++) lo[e] = root(e % L, L);
        for (uint64_t e = 0; e < nhi; e++) hi[e] = root((e << h) % L, L);
    }
    ~Table() {
        free(lo);
        free(hi);
    }
    static cx<T> root(uint64_t x, uint64_t L) {
        const ld ang = 2 * kPi * ((ld)x / (ld)L);
        return {(T)(double)cosl(ang), (T)(double)(-sinl(ang))};  // (TableBuilder::put: through double)
    }
};

static uint64_t sq_mod_ref(uint64_t j, uint64_t n2) { return (uint64_t)(((u128)j * (u128)j) % (u128)n2); }

template <typename T>
static bool same(cx<T> a, cx<T> b) {
    return memcmp(&a, &b, sizeof a) == 0;
}

template <typename T>
static void attach(ChirpArgs& a, const Table<T>& t) {
    a.tw_lo = t.lo;
    a.tw_hi = t.hi;
    a.tw_h = t.h;
}

// the launch's thread count, as build_chirp sizes it
static uint64_t threads_of(uint64_t total, uint64_t cap) {
    const uint64_t blocks = (total + 255) / 256;
    return (blocks < cap ? (blocks ? blocks : 1) : cap) * 256;
}

template <int KIND, typename T, int SW>
static void launch(uint64_t N, uint32_t batch, uint64_t cap, const Table<T>& t, const void* in, void* out,
                   const void* bt) {
    const uint64_t M = chirp_length(N);
    const uint64_t threads = threads_of((uint64_t)batch * chirp_units<T>(KIND, N, M), cap);
    ChirpArgs a = chirp_args<T>(KIND, N, batch, threads);
    attach(a, t);
    a.in = in;
    a.out = out;
    a.bt = bt;
    for (uint64_t gid = 0; gid < threads; gid++) chirp_thread<KIND, T, SW>(a, gid);
}

template <typename T>
static int run_kernels(uint64_t N, uint32_t batch, uint64_t cap, int mis) {
    const uint64_t M = chirp_length(N), n2 = 2 * N;
    if (!cap) cap = 262144;
    Table<T> t(N);
    const T unset = (T)-12345.0;
    const cx<T> U{unset, unset};
    uint64_t bad = 0, unwritten = 0, guard = 0;
    auto w_of = [&](uint64_t j) { return real_tw(t.lo, t.hi, t.h, sq_mod_ref(j, n2)); };
    // the caller's rows: batch * N values exactly (+ mis guarded values in front)
    cx<T>* x0 = (cx<T>*)alloc16((batch * N + mis) * sizeof(cx<T>));
    cx<T>* x = x0 + mis;
    for (uint64_t i = 0; i < batch * N; i++) x[i] = {(T)draw(), (T)draw()};
    cx<T>* z = (cx<T>*)alloc16(batch * M * sizeof(cx<T>));
    cx<T>* bt = (cx<T>*)alloc16(M * sizeof(cx<T>));
    for (uint64_t i = 0; i < M; i++) bt[i] = {(T)draw(), (T)draw()};
    cx<T>* o0 = (cx<T>*)alloc16((batch * N + mis) * sizeof(cx<T>));
    cx<T>* o = o0 + mis;
    for (int sw = 0; sw < 2; sw++) {
        // --- pre ---
        for (uint64_t i = 0; i < batch * M; i++) z[i] = U;
        if (sw) launch<CHIRP_PRE, T, 1>(N, batch, cap, t, x, z, nullptr);
        else launch<CHIRP_PRE, T, 0>(N, batch, cap, t, x, z, nullptr);
        for (uint32_t b = 0; b < batch; b++)
            for (uint64_t j = 0; j < M; j++) {
                const cx<T> got = z[b * M + j];
                unwritten += same(got, U);
                const cx<T> want = j < N ? chirp_mul(sw ? chirp_swap(x[b * N + j]) : x[b * N + j], w_of(j))
                                         : cx<T>{(T)0, (T)0};
                bad += !same(got, want);
            }
        // --- mul, in place over the pre's output ---
        std::vector<cx<T>> before(z, z + batch * M);
        launch<CHIRP_MUL, T, 0>(N, batch, cap, t, nullptr, z, bt);
        for (uint32_t b = 0; b < batch; b++)
            for (uint64_t k = 0; k < M; k++) bad += !same(z[b * M + k], chirp_mul(before[b * M + k], bt[k]));
        // --- post ---
        for (uint64_t i = 0; i < batch * N + mis; i++) o0[i] = U;
        if (sw) launch<CHIRP_POST, T, 2>(N, batch, cap, t, z, o, nullptr);
        else launch<CHIRP_POST, T, 0>(N, batch, cap, t, z, o, nullptr);
        for (int i = 0; i < mis; i++) guard += !same(o0[i], U);
        for (uint32_t b = 0; b < batch; b++)
            for (uint64_t k = 0; k < N; k++) {
                const cx<T> got = o[b * N + k];
                unwritten += same(got, U);
                const cx<T> y = chirp_mul(z[b * M + k], w_of(k));
                bad += !same(got, sw ? chirp_swap(y) : y);
            }
    }
    printf("{\"bad\": %llu, \"unwritten\": %llu, \"guard\": %llu}\n", (unsigned long long)bad,
           (unsigned long long)unwritten, (unsigned long long)guard);
    free(x0);
    free(z);
    free(bt);
    free(o0);
    return 0;
}

static int run_sqmod(uint64_t N, uint64_t samples) {
    const uint64_t n2 = 2 * N;
    const double inv = 1.0 / (double)n2;
    uint64_t bad = 0;
    auto one = [&](uint64_t j) {
        const uint64_t r = chirp_sq_mod(j, n2, inv);
        bad += r != sq_mod_ref(j, n2);
        if (j + 1 < N) bad += chirp_sq_next(r, j, n2) != sq_mod_ref(j + 1, n2);
    };
    if (!samples)
        for (uint64_t j = 0; j < N; j++) one(j);
    else {
        one(0), one(N - 1), one(N - 2), one(N / 2);
        for (uint64_t i = 0; i < samples; i++) one(draw64() % N);
    }
    printf("{\"bad\": %llu}\n", (unsigned long long)bad);
    return 0;
}

template <typename T>
static int run_tw(uint64_t N) {
    Table<T> t(N);
    const uint64_t n2 = 2 * N;
    const ld eps = sizeof(T) == 4 ? 0x1.0p-23L : 0x1.0p-52L;
    ld worst = 0;
    auto one = [&](uint64_t r) {
        const cx<T> w = real_tw(t.lo, t.hi, t.h, r);
        const ld ang = kPi * ((ld)r / (ld)N), dr = (ld)w.re - cosl(ang), di = (ld)w.im + sinl(ang);
        const ld e = sqrtl(dr * dr + di * di);
        if (e > worst) worst = e;
    };
    if (n2 <= (1ull << 20))
        for (uint64_t r = 0; r < n2; r++) one(r);
    else {
        one(0), one(n2 - 1);
        for (int i = 0; i < (1 << 20); i++) one(draw64() % n2);
    }
    printf("{\"err\": %.4Lf}\n", worst / eps);
    return 0;
}

template <typename V>
static void naive_dft(const std::vector<V>& in, std::vector<V>& out, int sign) {
    const uint64_t M = in.size();
    out.resize(M);
    for (uint64_t k = 0; k < M; k++) {
        ld re = 0, im = 0;
        for (uint64_t j = 0; j < M; j++) {
            const ld ang = 2 * kPi * ((ld)((j * k) % M) / (ld)M), c = cosl(ang), s = sign * sinl(ang);
            re += (ld)in[j].re * c - (ld)in[j].im * s;
            im += (ld)in[j].re * s + (ld)in[j].im * c;
        }
        out[k] = {(decltype(out[k].re))re, (decltype(out[k].re))im};
    }
}

template <typename T>
static int run_formula(uint64_t N, int swapped) {
    const uint64_t M = chirp_length(N);
    Table<T> t(N);
    Table<double> td(N);
    // Bt as the library fixes it: b in fp64, DFT_M, / M, one rounding to T
    ChirpArgs f = chirp_args<double>(CHIRP_FILL, N, 1, 256);
    attach(f, td);
    std::vector<cx<double>> b(M), B;
    for (uint64_t j = 0; j < M; j++) b[j] = chirp_fill_one(f, j);
    naive_dft(b, B, -1);
    cx<T>* bt = (cx<T>*)alloc16(M * sizeof(cx<T>));
    for (uint64_t k = 0; k < M; k++) bt[k] = chirp_bt_one<T>(B[k], 1.0 / (double)M);
    cx<T>* x = (cx<T>*)alloc16(N * sizeof(cx<T>));
    for (uint64_t i = 0; i < N; i++) x[i] = {(T)draw(), (T)draw()};
    cx<T>* z = (cx<T>*)alloc16(M * sizeof(cx<T>));
    cx<T>* o = (cx<T>*)alloc16(N * sizeof(cx<T>));
    if (swapped) launch<CHIRP_PRE, T, 1>(N, 1, 262144, t, x, z, nullptr);
    else launch<CHIRP_PRE, T, 0>(N, 1, 262144, t, x, z, nullptr);
    std::vector<cx<T>> a(z, z + M), A;
    naive_dft(a, A, -1);
    memcpy(z, A.data(), M * sizeof(cx<T>));
    launch<CHIRP_MUL, T, 0>(N, 1, 262144, t, nullptr, z, bt);
    std::vector<cx<T>> y(z, z + M), c;
    naive_dft(y, c, +1);
    memcpy(z, c.data(), M * sizeof(cx<T>));
    if (swapped) launch<CHIRP_POST, T, 2>(N, 1, 262144, t, z, o, nullptr);
    else launch<CHIRP_POST, T, 0>(N, 1, 262144, t, z, o, nullptr);
    // the direct DFT of x; swapped: swap(DFT(swap(x))), the unnormalised inverse
    ld num = 0, den = 0;
    for (uint64_t k = 0; k < N; k++) {
        ld re = 0, im = 0;
        for (uint64_t j = 0; j < N; j++) {
            const ld ang = 2 * kPi * ((ld)((j * k) % N) / (ld)N), cs = cosl(ang), sn = (swapped ? 1 : -1) * sinl(ang);
            re += (ld)x[j].re * cs - (ld)x[j].im * sn;
            im += (ld)x[j].re * sn + (ld)x[j].im * cs;
        }
        num += ((ld)o[k].re - re) * ((ld)o[k].re - re) + ((ld)o[k].im - im) * ((ld)o[k].im - im);
        den += re * re + im * im;
    }
    const ld eps = sizeof(T) == 4 ? 0x1.0p-23L : 0x1.0p-52L;
    printf("{\"err\": %.4Lf}\n", sqrtl(num / den) / eps);
    free(bt);
    free(x);
    free(z);
    free(o);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const uint64_t N = strtoull(argv[2], nullptr, 10);
    if (N < 3 || N > (1ull << 27) || !(N & (N - 1))) return 2;
    if (!strcmp(argv[1], "kernels") && argc == 7) {
        const uint32_t batch = (uint32_t)atoi(argv[3]);
        const uint64_t cap = strtoull(argv[5], nullptr, 10);
        const int mis = atoi(argv[6]);
        if (batch < 1 || N > (1 << 16) || (mis != 0 && mis != 1)) return 2;
        return atoi(argv[4]) == 64 ? run_kernels<double>(N, batch, cap, mis) : run_kernels<float>(N, batch, cap, mis);
    }
    if (!strcmp(argv[1], "sqmod") && argc == 4) return run_sqmod(N, strtoull(argv[3], nullptr, 10));
    if (!strcmp(argv[1], "tw") && argc == 4) return atoi(argv[3]) == 64 ? run_tw<double>(N) : run_tw<float>(N);
    if (!strcmp(argv[1], "formula") && argc == 5 && N <= 64)
        return atoi(argv[3]) == 64 ? run_formula<double>(N, atoi(argv[4])) : run_formula<float>(N, atoi(argv[4]));
    return 2;
}
