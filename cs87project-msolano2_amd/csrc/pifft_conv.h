// cs87project-msolano2_amd/csrc/pifft_conv.h
//
// Real FFT convolution plans (pifft_plan_create_conv): the streaming kernels
// around the two H-point chains of a real transform of M = 2H reals.  Included
// by pifft.hip only; the k_pass translation units do not see this header.
//
// batch rows of n reals x, one filter of taps reals h shared by all rows,
// L = n + taps - 1, M the smallest power of two >= max(L, 4), H = M/2:
//   z    = x, zeros up to M, read as H complex values             (k_conv_pad)
//   Y    = DFT_H(z)                                               (forward chain)
//   X[k], X[H-k] = real_pair<0>(Y[k], Y[H-k], w^k)                \
//   P[k] = X[k] G[k],  P[H-k] = X[H-k] G[H-k]                      > k_conv_pair, in place
//   Y'[k], Y'[H-k] = real_pair<1>(P[k], P[H-k], w^k)              /
//   z'   = IDFT_H(Y'), unnormalised                               (inverse chain)
//   y[j] = z' read as reals, j < L                                (k_conv_crop)
// G = R2C_M(h / M), H + 1 values, fixed by pifft_conv_set_filter: the filter
// padded to M reals -- back to front for a correlation -- and scaled by the
// exact 1/M (k_conv_filter), the forward chain at batch 1, k_r2c_post.  R2C
// then C2R returns M times its input (pifft_real.h), so that one 1/M leaves y
// the convolution itself.  A cyclic plan (M = n) has no pad and no crop.
//
// k_conv_pair is k_r2c_post, a pointwise product and k_c2r_pre on the pair
// (k, H-k) in registers: the functions of pifft_real.h and chirp_mul of
// pifft_chirp.h in their own operation order, so the result equals the three
// launches' bit for bit (no contraction: -ffp-contract=off).  Bin 0 follows
// real_one's k == 0 branches -- X[0] and X[H] are real, G[0] and G[H] have
// imaginary part +0, so the product is the real one -- and bin H/2 pairs with
// itself: one product, written once.  Access shape and grid-stride walk are
// real_unit's and real_thread's: fp64 one 16-B value per lane and run, fp32
// two adjacent pairs per lane, the ascending runs of Y and G 16-B accesses
// (the descending ones start at an odd element: two 8-B accesses), a row's
// first and last work items pair by pair.
//
// k_conv_pad and k_conv_crop move 16 B of the Z row per lane (4 floats, 2
// doubles), always one 16-B access there (Z rows are M reals, M >= 4).  The
// caller's rows (stride n in, L out) need only the alignment of T, and an odd
// n or L puts them at every 4-B (fp64: 8-B) residue: one 16-B access where
// the address is 16-B aligned, 8-B and 4-B ones where it is not, and the
// ragged end of a row element by element -- no byte outside a row's n or L
// values is read or written.  k_conv_pad writes the zeros of [n, M) of every
// row on every execution: the inverse chain leaves its result in Z.
//
// The per-thread code is __host__ __device__ so the index arithmetic can be
// run under a host sanitizer (tests/native/conv_main.hip).
#pragma once

// chirp_mul comes from pifft_chirp.h, which the includer brings in before this
// header (pifft.hip does; tests/test_chirp_plan.py holds that pifft.hip alone
// includes it)
#include "pifft_real.h"

namespace pifft {

struct ConvArgs {
    const void* in;
    void* out;
    const void* tw_lo;  // k_conv_pair: two-level w_M (TableBuilder two_level)
    const void* tw_hi;
    const void* g;      // k_conv_pair: G, H + 1 values
    uint32_t tw_h;
    uint32_t batch;
    uint64_t len;       // reals per row on the caller's side: n (pad), L (crop), taps (filter)
    uint64_t h;         // H = M/2, complex values per row of Z and Y
    uint64_t units;     // work items per row: conv_units<T>(kind, len, H)
    uint64_t step_rows, step_units;  // the launch's thread count / units, % units
    uint32_t rev;       // k_conv_filter: the filter read back to front
    double scale;       // k_conv_filter: 1 / M
};

enum { CONV_PAD = 0, CONV_PAIR = 1, CONV_CROP = 2, CONV_FILTER = 3 };

// the smallest power of two >= max(n + taps - 1, 4)
PIFFT_HD uint64_t conv_length(uint64_t n, uint64_t taps) {
    uint64_t m = 4;
    while (m < n + taps - 1) m <<= 1;
    return m;
}

// reals a thread moves per work item of pad and crop: 16 B
template <typename T>
constexpr uint64_t conv_vec() {
    return 16 / sizeof(T);
}
// work items per row: pad and filter walk the M reals of a Z row, crop the L results, pair as real_units
template <typename T>
PIFFT_HD uint64_t conv_units(int kind, uint64_t len, uint64_t h) {
    return kind == CONV_PAIR ? real_units<T>(h)
           : kind == CONV_CROP ? (len + conv_vec<T>() - 1) / conv_vec<T>()
                               : 2 * h / conv_vec<T>();
}

typedef float conv_f2 __attribute__((ext_vector_type(2)));
typedef double conv_d2 __attribute__((ext_vector_type(2)));

// conv_vec reals at a 16-B aligned address (Z rows)
template <typename T>
PIFFT_HD void conv_ld16(const T* p, T* v) {
    if constexpr (sizeof(T) == 4) {
        const real_f4 q = *reinterpret_cast<const real_f4*>(p);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
        const conv_d2 q = *reinterpret_cast<const conv_d2*>(p);
        v[0] = q.x, v[1] = q.y;
    }
}
template <typename T>
PIFFT_HD void conv_st16(T* p, const T* v) {
    if constexpr (sizeof(T) == 4) {
        real_f4 q;
        q.x = v[0], q.y = v[1], q.z = v[2], q.w = v[3];
        *reinterpret_cast<real_f4*>(p) = q;
    } else {
        conv_d2 q;
        q.x = v[0], q.y = v[1];
        *reinterpret_cast<conv_d2*>(p) = q;
    }
}
// conv_vec reals of a caller's row, p aligned as T only: the widest accesses its address allows
template <typename T>
PIFFT_HD void conv_ldv(const T* p, T* v) {
    const uintptr_t a = (uintptr_t)p & 15;
    if (a == 0) {
        conv_ld16(p, v);
    } else if constexpr (sizeof(T) == 8) {
        v[0] = p[0], v[1] = p[1];
    } else if ((a & 7) == 0) {
        const conv_f2 q0 = *reinterpret_cast<const conv_f2*>(p), q1 = *reinterpret_cast<const conv_f2*>(p + 2);
        v[0] = q0.x, v[1] = q0.y, v[2] = q1.x, v[3] = q1.y;
    } else {  // 4 mod 8: p + 1 is 8-B aligned
        const conv_f2 q = *reinterpret_cast<const conv_f2*>(p + 1);
        v[0] = p[0], v[1] = q.x, v[2] = q.y, v[3] = p[3];
    }
}
template <typename T>
PIFFT_HD void conv_stv(T* p, const T* v) {
    const uintptr_t a = (uintptr_t)p & 15;
    if (a == 0) {
        conv_st16(p, v);
    } else if constexpr (sizeof(T) == 8) {
        p[0] = v[0], p[1] = v[1];
    } else if ((a & 7) == 0) {
        conv_f2 q0, q1;
        q0.x = v[0], q0.y = v[1], q1.x = v[2], q1.y = v[3];
        *reinterpret_cast<conv_f2*>(p) = q0;
        *reinterpret_cast<conv_f2*>(p + 2) = q1;
    } else {
        conv_f2 q;
        q.x = v[1], q.y = v[2];
        p[0] = v[0];
        *reinterpret_cast<conv_f2*>(p + 1) = q;
        p[3] = v[3];
    }
}

// k_conv_pad, work item u of row `row`: Z[row M + j] = x[row n + j], j < n; 0, n <= j < M
template <typename T>
PIFFT_HD void conv_pad_unit(const ConvArgs& a, uint64_t row, uint64_t u) {
    constexpr uint64_t V = conv_vec<T>();
    const uint64_t n = a.len, j0 = V * u;
    const T* __restrict__ x = (const T*)a.in + row * n;
    T* __restrict__ z = (T*)a.out + row * 2 * a.h;
    T v[V];
    for (uint64_t i = 0; i < V; i++) v[i] = (T)0;
    if (j0 + V <= n) {
        conv_ldv(x + j0, v);
    } else {  // the ragged end of the row, then zeros
        for (uint64_t i = 0; i < V; i++)
            if (j0 + i < n) v[i] = x[j0 + i];
    }
    conv_st16(z + j0, v);
}

// k_conv_crop, work item u of row `row`: y[row L + j] = Z[row M + j], j < L
template <typename T>
PIFFT_HD void conv_crop_unit(const ConvArgs& a, uint64_t row, uint64_t u) {
    constexpr uint64_t V = conv_vec<T>();
    const uint64_t L = a.len, j0 = V * u;
    const T* __restrict__ z = (const T*)a.in + row * 2 * a.h;
    T* __restrict__ y = (T*)a.out + row * L;
    T v[V];
    conv_ld16(z + j0, v);  // (j0 < L <= M, M a multiple of V: inside the Z row)
    if (j0 + V <= L) {
        conv_stv(y + j0, v);
    } else {
        for (uint64_t i = 0; i < V; i++)
            if (j0 + i < L) y[j0 + i] = v[i];
    }
}

// k_conv_filter, work item u of the one row: Z[j] = h[j] / M (rev: h[taps - 1 - j]), j < taps; 0 up to M
template <typename T>
PIFFT_HD void conv_filter_unit(const ConvArgs& a, uint64_t u) {
    constexpr uint64_t V = conv_vec<T>();
    const uint64_t taps = a.len, j0 = V * u;
    const T* __restrict__ h = (const T*)a.in;
    const T s = (T)a.scale;  // (a power of two: exact)
    T v[V];
    for (uint64_t i = 0; i < V; i++) {
        const uint64_t j = j0 + i;
        v[i] = j < taps ? h[a.rev ? taps - 1 - j : j] * s : (T)0;
    }
    conv_st16((T*)a.out + j0, v);
}

// the three steps of one pair in registers; self: k == H - k, one product
template <typename T>
PIFFT_HD void conv_pair_math(cx<T> A, cx<T> B, cx<T> w, cx<T> gk, cx<T> gm, bool self, cx<T>& rk, cx<T>& rm) {
    cx<T> xk, xm;
    real_pair<0>(A, B, w, xk, xm);
    const cx<T> pk = chirp_mul(xk, gk);
    const cx<T> pm = self ? pk : chirp_mul(xm, gm);
    real_pair<1>(pk, pm, w, rk, rm);
}

// one pair (k, H-k), 0 <= k <= H/2, of the row at y, in place
template <typename T>
PIFFT_HD void conv_pair_one(const ConvArgs& a, cx<T>* __restrict__ y, uint64_t k) {
    const uint64_t H = a.h;
    const cx<T>* __restrict__ g = (const cx<T>*)a.g;
    if (k == 0) {  // (real_one's k == 0 branches around the real products)
        const cx<T> z0 = y[0];
        const T x0 = z0.re + z0.im, xh = z0.re - z0.im;
        const T p0 = x0 * g[0].re, ph = xh * g[H].re;
        y[0] = {p0 + ph, p0 - ph};
        return;
    }
    const uint64_t m = H - k;
    const cx<T> A = y[k];
    const cx<T> B = m != k ? y[m] : A;
    const cx<T> w = real_tw((const cx<T>*)a.tw_lo, (const cx<T>*)a.tw_hi, a.tw_h, k);
    cx<T> rk, rm;
    conv_pair_math(A, B, w, g[k], g[m], m == k, rk, rm);
    y[k] = rk;
    if (m != k) y[m] = rm;  // (bin H/2 pairs with itself: written once)
}

// k_conv_pair, work item u of row `row` (as real_unit)
template <typename T>
PIFFT_HD void conv_pair_unit(const ConvArgs& a, uint64_t row, uint64_t u) {
    const uint64_t H = a.h;
    cx<T>* __restrict__ y = (cx<T>*)a.out + row * H;
    if constexpr (real_vec<T>() == 1) {
        conv_pair_one<T>(a, y, u);
    } else {
        const uint64_t k0 = 2 * u, k1 = k0 + 1;
        if (k0 == 0 || k1 >= H - k1) {  // the row's first and last items: pair by pair
            conv_pair_one<T>(a, y, k0);
            if (k1 <= H / 2) conv_pair_one<T>(a, y, k1);
            return;
        }
        // 2 <= k0 < k1 < H/2: the ascending run (k0, k1), the descending one (H-k1, H-k0)
        const uint64_t m1 = H - k1;
        const cx<T>* __restrict__ g = (const cx<T>*)a.g;
        cx<T> A0, A1, B1, B0, ga0, ga1, gb1, gb0;
        real_ld2(y + k0, A0, A1);
        real_ld2(y + m1, B1, B0);
        real_ld2(g + k0, ga0, ga1);
        real_ld2(g + m1, gb1, gb0);
        const cx<T>* lo = (const cx<T>*)a.tw_lo;
        const cx<T>* hi = (const cx<T>*)a.tw_hi;
        const cx<T> w0 = real_tw(lo, hi, a.tw_h, k0), w1 = real_tw(lo, hi, a.tw_h, k1);
        cx<T> r0, s0, r1, s1;
        conv_pair_math(A0, B0, w0, ga0, gb0, false, r0, s0);
        conv_pair_math(A1, B1, w1, ga1, gb1, false, r1, s1);
        real_st2(y + k0, r0, r1);
        real_st2(y + m1, s1, s0);
    }
}

// every work item of thread gid0 (< 2^32) of the grid-stride launch (as real_thread)
template <int KIND, typename T>
PIFFT_HD void conv_thread(const ConvArgs& a, uint64_t gid0) {
    uint64_t row = 0, u = gid0;
    if ((a.units >> 32) == 0) {  // (else gid0 < units: row 0)
        const uint32_t q = (uint32_t)gid0 / (uint32_t)a.units;
        row = q;
        u = gid0 - (uint64_t)q * a.units;
    }
    while (row < a.batch) {
        if constexpr (KIND == CONV_PAD) conv_pad_unit<T>(a, row, u);
        else if constexpr (KIND == CONV_PAIR) conv_pair_unit<T>(a, row, u);
        else if constexpr (KIND == CONV_CROP) conv_crop_unit<T>(a, row, u);
        else conv_filter_unit<T>(a, u);
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
PIFFT_HD ConvArgs conv_args(int kind, uint64_t len, uint64_t h, uint32_t batch, uint64_t threads) {
    ConvArgs a{};
    a.len = len;
    a.h = h;
    a.batch = batch;
    a.units = conv_units<T>(kind, len, h);
    a.step_rows = threads / a.units;
    a.step_units = threads % a.units;
    a.scale = 1.0 / (double)(2 * h);
    return a;
}

template <typename T>
__global__ __launch_bounds__(256) void k_conv_pad(ConvArgs a) {
    conv_thread<CONV_PAD, T>(a, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
}
template <typename T>
__global__ __launch_bounds__(256) void k_conv_pair(ConvArgs a) {
    conv_thread<CONV_PAIR, T>(a, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
}
template <typename T>
__global__ __launch_bounds__(256) void k_conv_crop(ConvArgs a) {
    conv_thread<CONV_CROP, T>(a, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
}
template <typename T>
__global__ __launch_bounds__(256) void k_conv_filter(ConvArgs a) {
    conv_thread<CONV_FILTER, T>(a, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
}

// The convolution plans' kernels: a table of their own, as the matrix and the
// chirp plans' (the kAux registry of pifft.hip lists the 1-D and real plans'
// auxiliary kernels only).
struct ConvKernel {
    int kind, prec;  // CONV_*; 32 / 64
    const void* fn;
};
inline const void* conv_fn(int kind, int prec) {
    static const ConvKernel kConv[] = {
        {CONV_PAD, 32, (const void*)&k_conv_pad<float>},       {CONV_PAD, 64, (const void*)&k_conv_pad<double>},
        {CONV_PAIR, 32, (const void*)&k_conv_pair<float>},     {CONV_PAIR, 64, (const void*)&k_conv_pair<double>},
        {CONV_CROP, 32, (const void*)&k_conv_crop<float>},     {CONV_CROP, 64, (const void*)&k_conv_crop<double>},
        {CONV_FILTER, 32, (const void*)&k_conv_filter<float>}, {CONV_FILTER, 64, (const void*)&k_conv_filter<double>},
    };
    for (const ConvKernel& k : kConv)
        if (k.kind == kind && k.prec == prec) return k.fn;
    return nullptr;
}

}  // namespace pifft
