// cs87project-msolano2_amd/csrc/pifft_chirp.h
//
// Arbitrary-length 1-D transforms (pifft_plan_create_chirp): the streaming
// kernels of Bluestein's chirp-z algorithm around two power-of-two chains.
// Included by pifft.hip only; the k_pass translation units do not see this
// header.
//
// For N not a power of two, w[j] = e^{-i pi j^2/N} and jk = (j^2 + k^2 - (k-j)^2)/2:
//   X[k] = sum_j x[j] e^{-2 pi i jk/N} = w[k] sum_j (x[j] w[j]) conj(w[k-j]),
// a linear convolution, done as a cyclic one of length M, the smallest power of
// two >= 2N - 1:
//   a[j] = x[j] w[j], j < N; 0 for N <= j < M                   (k_chirp_pre)
//   b[j] = conj w[j], j < N; b[M-j] = conj w[j], 1 <= j < N; else 0  (k_chirp_fill)
//   Bt   = DFT_M(b) / M, once per plan, in fp64, rounded once     (k_chirp_bt)
//   c    = IDFT_M(DFT_M(a) Bt), the inverse unnormalised        (k_spectrum_mul)
//   X[k] = w[k] c[k], k < N                                     (k_chirp_post)
//
// w[j] depends on r = j^2 mod 2N only: w[j] = w_2N^r, w_2N = e^{-i pi/N}.  r is
// exact integer arithmetic (chirp_sq_mod): j^2 < 2^54 fits 64 bits; the
// quotient j^2 / 2N < 2^26 is estimated by one fp64 product with 1/(2N) --
// within 2^-24 of the true quotient, so its floor is off by at most one -- and
// the remainder j^2 - q 2N, taken in 64-bit integers, is put right by one
// conditional step.  No 64-bit division in the kernels.  Of two adjacent
// values the second takes r + 2j + 1, reduced once.
// w_2N^r is the plan's two-level table, hi[r >> h] lo[r & mask] (real_tw,
// 2^h ~ sqrt 2N entries each, L2 resident at every size): no sincos, no
// fast-math, and like every kernel here built with -ffp-contract=off.  r is
// pseudo-random in j, so a wave's lookups are gathers of 64 different lines per
// level: measured, they and not the arithmetic of r are what keeps k_chirp_pre
// and k_chirp_post from a copy's rate.
//
// All three plan kernels stream.  Z and Y rows (stride M, a power of two >= 8)
// are 16-B aligned: 16-B accesses throughout.  The caller's rows (stride N) need
// only the alignment of their complex type: fp64 moves one 16-B value per lane,
// fp32 two adjacent values -- one 16-B access where the address is 16-B aligned,
// two 8-B accesses where it is not (real_ld2 / real_st2; an odd N puts every
// other fp32 row at 8 mod 16) -- and the last value of an odd row alone: no
// byte outside a row's N values is read or written.  k_chirp_pre writes the
// zeros of [N, M) of every row on every execution: the inverse chain leaves its
// result in Z, so the pad is dirty after each run.
//
// PIFFT_INVERSE: IDFT(x) = swap(DFT(swap(x))).  k_chirp_pre<T, 1> swaps re/im of
// what it loads from d_in, k_chirp_post<T, 2> what it stores to d_out; all
// between is the forward plan.
//
// The per-thread code is __host__ __device__ so the index arithmetic can be
// run under a host sanitizer (tests/native/chirp_main.hip).
#pragma once

#include "pifft_real.h"

namespace pifft {

struct ChirpArgs {
    const void* in;
    void* out;
    const void* tw_lo;  // two-level w_2N (two_level_any)
    const void* tw_hi;
    const void* bt;     // k_spectrum_mul: Bt, M values
    uint32_t tw_h;
    uint32_t batch;
    uint64_t n, m;      // N; M = chirp_length(N)
    double inv_2n;      // 1 / (2N), rounded once
    uint64_t units;     // work items per row: chirp_units<T>(kind, N, M)
    uint64_t step_rows, step_units;  // the launch's thread count / units, % units
};

enum { CHIRP_PRE = 0, CHIRP_MUL = 1, CHIRP_POST = 2, CHIRP_FILL = 3, CHIRP_BT = 4 };

// the smallest power of two >= 2N - 1
PIFFT_HD uint64_t chirp_length(uint64_t n) {
    uint64_t m = 1;
    while (m < 2 * n - 1) m <<= 1;
    return m;
}

// values a thread takes per work item
template <typename T>
constexpr uint64_t chirp_vec() {
    return sizeof(T) == 4 ? 2 : 1;
}
// work items per row: pre and mul walk the M values of a Z / Y row, post the N results
template <typename T>
PIFFT_HD uint64_t chirp_units(int kind, uint64_t n, uint64_t m) {
    return kind == CHIRP_POST ? (n + chirp_vec<T>() - 1) / chirp_vec<T>() : m / chirp_vec<T>();
}

// j^2 mod 2N, exactly (j < N <= 2^27)
PIFFT_HD uint64_t chirp_sq_mod(uint64_t j, uint64_t n2, double inv_2n) {
    const uint64_t jj = j * j;
    const uint64_t q = (uint64_t)((double)jj * inv_2n);
    const int64_t r = (int64_t)(jj - q * n2);
    return (uint64_t)(r < 0 ? r + (int64_t)n2 : r >= (int64_t)n2 ? r - (int64_t)n2 : r);
}
// (j + 1)^2 mod 2N from r = j^2 mod 2N
PIFFT_HD uint64_t chirp_sq_next(uint64_t r, uint64_t j, uint64_t n2) {
    const uint64_t s = r + 2 * j + 1;  // (2j + 1 < 2N)
    return s >= n2 ? s - n2 : s;
}

template <typename T>
PIFFT_HD cx<T> chirp_mul(cx<T> x, cx<T> w) {
    return {x.re * w.re - x.im * w.im, x.re * w.im + x.im * w.re};
}
template <typename T>
PIFFT_HD cx<T> chirp_swap(cx<T> x) {
    return {x.im, x.re};
}

// two adjacent values at a 16-B aligned address (Z, Y and Bt rows)
template <typename T>
PIFFT_HD void chirp_ld16(const cx<T>* p, cx<T>& a, cx<T>& b) {
    const real_f4 v = *reinterpret_cast<const real_f4*>(p);
    a = {v.x, v.y};
    b = {v.z, v.w};
}
template <typename T>
PIFFT_HD void chirp_st16(cx<T>* p, cx<T> a, cx<T> b) {
    real_f4 v;
    v.x = a.re, v.y = a.im, v.z = b.re, v.w = b.im;
    *reinterpret_cast<real_f4*>(p) = v;
}

// k_chirp_pre, work item u of row `row`: Z[row M + j] = x[row N + j] w[j], j < N; 0, N <= j < M
template <typename T, int SW>
PIFFT_HD void chirp_pre_unit(const ChirpArgs& a, uint64_t row, uint64_t u) {
    const uint64_t N = a.n;
    const cx<T>* __restrict__ xi = (const cx<T>*)a.in + row * N;
    cx<T>* __restrict__ zo = (cx<T>*)a.out + row * a.m;
    const cx<T>* lo = (const cx<T>*)a.tw_lo;
    const cx<T>* hi = (const cx<T>*)a.tw_hi;
    const cx<T> zero{(T)0, (T)0};
    if constexpr (chirp_vec<T>() == 1) {
        cx<T> y = zero;
        if (u < N) {
            const cx<T> x = xi[u];
            y = chirp_mul(SW & 1 ? chirp_swap(x) : x, real_tw(lo, hi, a.tw_h, chirp_sq_mod(u, 2 * N, a.inv_2n)));
        }
        zo[u] = y;
    } else {
        const uint64_t j0 = 2 * u;
        cx<T> y0 = zero, y1 = zero;
        if (j0 < N) {
            const bool two = j0 + 1 < N;  // (else the last value of an odd row, alone)
            cx<T> x0, x1 = zero;
            if (two) real_ld2(xi + j0, x0, x1);
            else x0 = xi[j0];
            const uint64_t r0 = chirp_sq_mod(j0, 2 * N, a.inv_2n);
            y0 = chirp_mul(SW & 1 ? chirp_swap(x0) : x0, real_tw(lo, hi, a.tw_h, r0));
            if (two)
                y1 = chirp_mul(SW & 1 ? chirp_swap(x1) : x1, real_tw(lo, hi, a.tw_h, chirp_sq_next(r0, j0, 2 * N)));
        }
        chirp_st16(zo + j0, y0, y1);
    }
}

// k_spectrum_mul, work item u of row `row`: Y[row M + k] *= Bt[k], in place
template <typename T>
PIFFT_HD void chirp_mul_unit(const ChirpArgs& a, uint64_t row, uint64_t u) {
    cx<T>* __restrict__ y = (cx<T>*)a.out + row * a.m;
    const cx<T>* __restrict__ bt = (const cx<T>*)a.bt;
    if constexpr (chirp_vec<T>() == 1) {
        y[u] = chirp_mul(y[u], bt[u]);
    } else {
        cx<T> y0, y1, b0, b1;
        chirp_ld16(y + 2 * u, y0, y1);
        chirp_ld16(bt + 2 * u, b0, b1);
        chirp_st16(y + 2 * u, chirp_mul(y0, b0), chirp_mul(y1, b1));
    }
}

// k_chirp_post, work item u of row `row`: X[row N + k] = w[k] Z[row M + k], k < N
template <typename T, int SW>
PIFFT_HD void chirp_post_unit(const ChirpArgs& a, uint64_t row, uint64_t u) {
    const uint64_t N = a.n;
    const cx<T>* __restrict__ zi = (const cx<T>*)a.in + row * a.m;
    cx<T>* __restrict__ xo = (cx<T>*)a.out + row * N;
    const cx<T>* lo = (const cx<T>*)a.tw_lo;
    const cx<T>* hi = (const cx<T>*)a.tw_hi;
    if constexpr (chirp_vec<T>() == 1) {
        const cx<T> y = chirp_mul(zi[u], real_tw(lo, hi, a.tw_h, chirp_sq_mod(u, 2 * N, a.inv_2n)));
        xo[u] = SW & 2 ? chirp_swap(y) : y;
    } else {
        const uint64_t k0 = 2 * u;
        const uint64_t r0 = chirp_sq_mod(k0, 2 * N, a.inv_2n);
        if (k0 + 1 < N) {
            cx<T> c0, c1;
            chirp_ld16(zi + k0, c0, c1);
            const cx<T> y0 = chirp_mul(c0, real_tw(lo, hi, a.tw_h, r0));
            const cx<T> y1 = chirp_mul(c1, real_tw(lo, hi, a.tw_h, chirp_sq_next(r0, k0, 2 * N)));
            real_st2(xo + k0, SW & 2 ? chirp_swap(y0) : y0, SW & 2 ? chirp_swap(y1) : y1);
        } else {  // the last value of an odd row, alone
            const cx<T> y0 = chirp_mul(zi[k0], real_tw(lo, hi, a.tw_h, r0));
            xo[k0] = SW & 2 ? chirp_swap(y0) : y0;
        }
    }
}

// every work item of thread gid0 (< 2^32) of the grid-stride launch (as real_thread)
template <int KIND, typename T, int SW>
PIFFT_HD void chirp_thread(const ChirpArgs& a, uint64_t gid0) {
    uint64_t row = 0, u = gid0;
    if ((a.units >> 32) == 0) {  // (else gid0 < units: row 0)
        const uint32_t q = (uint32_t)gid0 / (uint32_t)a.units;
        row = q;
        u = gid0 - (uint64_t)q * a.units;
    }
    while (row < a.batch) {
        if constexpr (KIND == CHIRP_PRE) chirp_pre_unit<T, SW>(a, row, u);
        else if constexpr (KIND == CHIRP_MUL) chirp_mul_unit<T>(a, row, u);
        else chirp_post_unit<T, SW>(a, row, u);
        u += a.step_units;
        row += a.step_rows;
        if (u >= a.units) {
            u -= a.units;
            row++;
        }
    }
}

// the launch's arguments but the pointers and the table, for `threads` work-items in all
template <typename T>
PIFFT_HD ChirpArgs chirp_args(int kind, uint64_t n, uint32_t batch, uint64_t threads) {
    ChirpArgs a{};
    a.n = n;
    a.m = chirp_length(n);
    a.batch = batch;
    a.inv_2n = 1.0 / (double)(2 * n);
    a.units = chirp_units<T>(kind, n, a.m);
    a.step_rows = threads / a.units;
    a.step_units = threads % a.units;
    return a;
}

// plan creation only, fp64: b[j], j < M, from the fp64 two-level table of w_2N
PIFFT_HD cx<double> chirp_fill_one(const ChirpArgs& a, uint64_t j) {
    const uint64_t N = a.n, d = j < N ? j : a.m - j;  // (M - N + 1 > N - 1: the two runs do not meet)
    if (d >= N) return {0.0, 0.0};
    const cx<double> w =
        real_tw((const cx<double>*)a.tw_lo, (const cx<double>*)a.tw_hi, a.tw_h, chirp_sq_mod(d, 2 * N, a.inv_2n));
    return {w.re, -w.im};
}
// plan creation only: Bt[k] = B[k] / M (exact: M is a power of two), rounded once to T
template <typename T>
PIFFT_HD cx<T> chirp_bt_one(cx<double> B, double inv_m) {
    return {(T)(B.re * inv_m), (T)(B.im * inv_m)};
}

template <typename T, int SW>
__global__ __launch_bounds__(256) void k_chirp_pre(ChirpArgs a) {
    chirp_thread<CHIRP_PRE, T, SW>(a, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
}
template <typename T>
__global__ __launch_bounds__(256) void k_spectrum_mul(ChirpArgs a) {
    chirp_thread<CHIRP_MUL, T, 0>(a, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
}
template <typename T, int SW>
__global__ __launch_bounds__(256) void k_chirp_post(ChirpArgs a) {
    chirp_thread<CHIRP_POST, T, SW>(a, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
}
// (a template, instantiated for double only, so that a host-only build that
// launches nothing needs no device code)
template <typename T>
__global__ __launch_bounds__(256) void k_chirp_fill(ChirpArgs a) {
    static_assert(sizeof(T) == 8, "b is filled in fp64");
    cx<T>* b = (cx<T>*)a.out;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < a.m; j += (uint64_t)gridDim.x * blockDim.x)
        b[j] = chirp_fill_one(a, j);
}
template <typename T>
__global__ __launch_bounds__(256) void k_chirp_bt(const cx<double>* __restrict__ B, cx<T>* __restrict__ bt,
                                                  double inv_m, uint64_t m) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < m; k += (uint64_t)gridDim.x * blockDim.x)
        bt[k] = chirp_bt_one<T>(B[k], inv_m);
}

// The chirp plans' kernels: a table of their own, as the matrix plans' (the
// kAux registry of pifft.hip lists the 1-D and real plans' auxiliary kernels only).
struct ChirpKernel {
    int kind, prec, sw;  // CHIRP_*; 32 / 64; 0, or the swap of an inverse plan's kernel (1 loads, 2 stores)
    const void* fn;
};
inline const void* chirp_fn(int kind, int prec, int sw) {
    static const ChirpKernel kChirp[] = {
        {CHIRP_PRE, 32, 0, (const void*)&k_chirp_pre<float, 0>},
        {CHIRP_PRE, 32, 1, (const void*)&k_chirp_pre<float, 1>},
        {CHIRP_PRE, 64, 0, (const void*)&k_chirp_pre<double, 0>},
        {CHIRP_PRE, 64, 1, (const void*)&k_chirp_pre<double, 1>},
        {CHIRP_MUL, 32, 0, (const void*)&k_spectrum_mul<float>},
        {CHIRP_MUL, 64, 0, (const void*)&k_spectrum_mul<double>},
        {CHIRP_POST, 32, 0, (const void*)&k_chirp_post<float, 0>},
        {CHIRP_POST, 32, 2, (const void*)&k_chirp_post<float, 2>},
        {CHIRP_POST, 64, 0, (const void*)&k_chirp_post<double, 0>},
        {CHIRP_POST, 64, 2, (const void*)&k_chirp_post<double, 2>},
        {CHIRP_FILL, 64, 0, (const void*)&k_chirp_fill<double>},
        {CHIRP_BT, 32, 0, (const void*)&k_chirp_bt<float>},
        {CHIRP_BT, 64, 0, (const void*)&k_chirp_bt<double>},
    };
    for (const ChirpKernel& k : kChirp)
        if (k.kind == kind && k.prec == prec && k.sw == sw) return k.fn;
    return nullptr;
}

}  // namespace pifft
