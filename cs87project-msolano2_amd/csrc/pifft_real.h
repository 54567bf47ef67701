// cs87project-msolano2_amd/csrc/pifft_real.h
//
// Real-input transforms (pifft_plan_create_real): the two streaming fix-up
// kernels around an N/2-point complex plan.  Included by pifft.hip only; the
// k_pass translation units do not see this header.
//
// N reals x are H = N/2 complex values z[n] = x[2n] + i x[2n+1] as they lie
// in memory.  With Z = DFT_H(z), w = e^{-2 pi i/N} and, for 1 <= k <= H/2,
//   A = Z[k], B = Z[H-k], E = (A + conj B)/2, O = -i (A - conj B)/2, T = w^k O:
//   X[k] = E + T,  X[H-k] = conj(E - T);   X[0] = Zr + Zi, X[H] = Zr - Zi of Z[0]
// (k_r2c_post: Z, batch stride H -> X, batch stride H + 1).  The other way,
//   S = X[k] + conj X[H-k], D = X[k] - conj X[H-k], T = i conj(w^k) D:
//   Z'[k] = S + T,  Z'[H-k] = conj(S - T);   Z'[0] = (X0 + XH) + i (X0 - XH)
// (k_c2r_pre: X -> Z' = 2 Z, so IDFT_H(Z') read as reals is N x).  Bin H/2 is
// paired with itself and written once.
//
// Both kernels stream: a thread reads the two values of a pair (k, H-k) once
// and writes both results; a wave's lanes cover one ascending and one
// descending contiguous run.  fp64 moves one 16-B value per lane and run; fp32
// takes two adjacent pairs per lane, each run as one 16-B access where its
// address is 16-B aligned and as two 8-B accesses where it is not: the H + 1
// stride puts every odd fp32 batch row of X at 8 mod 16, and the descending
// run starts at an odd element, so within a row exactly one of X's two runs is
// aligned, and of Z's the ascending one.
//
// w^k, k <= N/4, is the plan's two-level table of w_N (hi[k >> h] lo[k & mask],
// 2^h ~ sqrt N entries each, cache resident at every size): no sincos, no
// fast-math, and like every kernel here built with -ffp-contract=off.
//
// The per-thread code is __host__ __device__ so the index arithmetic can be
// run under a host sanitizer (tests/native/real_fixup_main.hip).
#pragma once

#include "pifft_kernels.h"

namespace pifft {

#define PIFFT_HD __host__ __device__ __forceinline__

struct RealArgs {
    const void* in;
    void* out;
    const void* tw_lo;  // two-level w_N (TableBuilder two_level)
    const void* tw_hi;
    uint32_t tw_h;
    uint32_t batch;
    uint64_t h;       // H = N/2, complex values per transform of Z
    uint64_t units;   // work items per transform: real_units<T>(H)
    uint64_t step_rows, step_units;  // the launch's thread count / units, % units
};

// pairs a thread takes per work item
template <typename T>
constexpr int real_vec() {
    return sizeof(T) == 4 ? 2 : 1;
}
// work items per transform: pairs k = 0 .. H/2 in groups of real_vec
template <typename T>
constexpr uint64_t real_units(uint64_t h) {
    return (h / 2) / (uint64_t)real_vec<T>() + 1;
}

template <typename T>
PIFFT_HD cx<T> real_tw(const cx<T>* __restrict__ lo, const cx<T>* __restrict__ hi, uint32_t h, uint64_t k) {
    const cx<T> a = lo[k & ((1ull << h) - 1)];
    const cx<T> b = hi[k >> h];
    return {b.re * a.re - b.im * a.im, b.re * a.im + b.im * a.re};
}

// DIR 0: (A, B) = (Z[k], Z[H-k]) -> (X[k], X[H-k]);  DIR 1: (X[k], X[H-k]) -> (Z'[k], Z'[H-k])
template <int DIR, typename T>
PIFFT_HD void real_pair(cx<T> A, cx<T> B, cx<T> w, cx<T>& rk, cx<T>& rm) {
    if constexpr (DIR == 0) {
        const T half = (T)0.5;
        const cx<T> E{(A.re + B.re) * half, (A.im - B.im) * half};
        const cx<T> O{(A.im + B.im) * half, (B.re - A.re) * half};
        const cx<T> t{w.re * O.re - w.im * O.im, w.re * O.im + w.im * O.re};
        rk = {E.re + t.re, E.im + t.im};
        rm = {E.re - t.re, t.im - E.im};
    } else {
        const cx<T> S{A.re + B.re, A.im - B.im};
        const cx<T> D{A.re - B.re, A.im + B.im};
        const cx<T> u{w.re * D.re + w.im * D.im, w.re * D.im - w.im * D.re};  // conj(w) D
        const cx<T> t{-u.im, u.re};
        rk = {S.re + t.re, S.im + t.im};
        rm = {S.re - t.re, t.im - S.im};
    }
}

// two adjacent values: one 16-B access at fp32 where p is 16-B aligned
typedef float real_f4 __attribute__((ext_vector_type(4)));
template <typename T>
PIFFT_HD void real_ld2(const cx<T>* p, cx<T>& a, cx<T>& b) {
    if constexpr (sizeof(T) == 4) {
        if (((uintptr_t)p & 15) == 0) {
            const real_f4 v = *reinterpret_cast<const real_f4*>(p);
            a = {v.x, v.y};
            b = {v.z, v.w};
            return;
        }
    }
    a = p[0];
    b = p[1];
}
template <typename T>
PIFFT_HD void real_st2(cx<T>* p, cx<T> a, cx<T> b) {
    if constexpr (sizeof(T) == 4) {
        if (((uintptr_t)p & 15) == 0) {
            real_f4 v;
            v.x = a.re, v.y = a.im, v.z = b.re, v.w = b.im;
            *reinterpret_cast<real_f4*>(p) = v;
            return;
        }
    }
    p[0] = a;
    p[1] = b;
}

// one pair (k, H-k), 0 <= k <= H/2, of the transform whose rows start at zi / zo
template <int DIR, typename T>
PIFFT_HD void real_one(const RealArgs& a, const cx<T>* __restrict__ zi, cx<T>* __restrict__ zo, uint64_t k) {
    const uint64_t H = a.h;
    if (k == 0) {
        const cx<T> z0 = zi[0];
        if constexpr (DIR == 0) {
            zo[0] = {z0.re + z0.im, (T)0};
            zo[H] = {z0.re - z0.im, (T)0};
        } else {
            const cx<T> zh = zi[H];  // (imaginary parts of X[0], X[H] ignored)
            zo[0] = {z0.re + zh.re, z0.re - zh.re};
        }
        return;
    }
    const uint64_t m = H - k;
    const cx<T> A = zi[k];
    const cx<T> B = m != k ? zi[m] : A;
    const cx<T> w = real_tw((const cx<T>*)a.tw_lo, (const cx<T>*)a.tw_hi, a.tw_h, k);
    cx<T> rk, rm;
    real_pair<DIR>(A, B, w, rk, rm);
    zo[k] = rk;
    if (m != k) zo[m] = rm;  // (bin H/2 pairs with itself: written once)
}

// work item u of transform `row`
template <int DIR, typename T>
PIFFT_HD void real_unit(const RealArgs& a, uint64_t row, uint64_t u) {
    const uint64_t H = a.h;
    const cx<T>* __restrict__ zi = (const cx<T>*)a.in + row * (DIR == 0 ? H : H + 1);
    cx<T>* __restrict__ zo = (cx<T>*)a.out + row * (DIR == 0 ? H + 1 : H);
    if constexpr (real_vec<T>() == 1) {
        real_one<DIR>(a, zi, zo, u);
    } else {
        const uint64_t k0 = 2 * u, k1 = k0 + 1;
        if (k0 == 0 || k1 >= H - k1) {  // the row's first and last items: pair by pair
            real_one<DIR>(a, zi, zo, k0);
            if (k1 <= H / 2) real_one<DIR>(a, zi, zo, k1);
            return;
        }
        // 2 <= k0 < k1 < H/2: the ascending run (k0, k1), the descending one (H-k1, H-k0)
        const uint64_t m1 = H - k1;
        cx<T> A0, A1, B1, B0;
        real_ld2(zi + k0, A0, A1);
        real_ld2(zi + m1, B1, B0);
        const cx<T>* lo = (const cx<T>*)a.tw_lo;
        const cx<T>* hi = (const cx<T>*)a.tw_hi;
        const cx<T> w0 = real_tw(lo, hi, a.tw_h, k0), w1 = real_tw(lo, hi, a.tw_h, k1);
        cx<T> r0, s0, r1, s1;
        real_pair<DIR>(A0, B0, w0, r0, s0);
        real_pair<DIR>(A1, B1, w1, r1, s1);
        real_st2(zo + k0, r0, r1);
        real_st2(zo + m1, s1, s0);
    }
}

// every work item of thread gid0 (< 2^32) of the grid-stride launch
template <int DIR, typename T>
PIFFT_HD void real_thread(const RealArgs& a, uint64_t gid0) {
    uint64_t row = 0, u = gid0;
    if ((a.units >> 32) == 0) {  // (else gid0 < units: row 0)
        const uint32_t q = (uint32_t)gid0 / (uint32_t)a.units;
        row = q;
        u = gid0 - (uint64_t)q * a.units;
    }
    while (row < a.batch) {
        real_unit<DIR, T>(a, row, u);
        u += a.step_units;
        row += a.step_rows;
        if (u >= a.units) {
            u -= a.units;
            row++;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_r2c_post(RealArgs a) {
    real_thread<0, T>(a, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
}
template <typename T>
__global__ __launch_bounds__(256) void k_c2r_pre(RealArgs a) {
    real_thread<1, T>(a, (uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
}

}  // namespace pifft
