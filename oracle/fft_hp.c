/*
 * oracle/fft_hp.c -- TEST INFRASTRUCTURE ONLY: the high-precision yardstick.
 *
 * A textbook radix-2 decimation-in-frequency FFT in C long double (x87 80-bit:
 * 64-bit significand, u = 2^-64), in place on (re, im) pairs.  It measures the
 * error of the oracle (pifft_oracle.c, which rounds like the reference) and of
 * the kernels against the same exact transform; it shares no code, no
 * operation order and no twiddle formula with either.
 *
 * Twiddles: w_N^k = (cosl(a), -sinl(a)), a = 2 pi (k / N), k < N/2, one table;
 * k / N is exact (N a power of two), 2 pi is a long-double literal, so a
 * carries two roundings (<= 2^-63 relative) and every entry is within about
 * 3e-19 of the exact root.
 *
 * DIF level t (block size s = N >> t, h = s/2), for every block at `off`:
 *     a = x[off+b], c = x[off+b+h]
 *     x[off+b]   = a + c
 *     x[off+b+h] = (a - c) w_N^{b 2^t}
 * After all log2 N levels X[k] sits at bitrev(k); `reorder` undoes that.  After
 * only the first log2 P levels (`levels`), x[q N/P .. (q+1) N/P) is worker q's
 * segment behind the pi-FFT's tree stage.
 */
#include "pifft_oracle.h"

#include <math.h>
#include <stdlib.h>

#define HP_TWO_PI 6.283185307179586476925286766559005768L

/* buf: n (re, im) long-double pairs; levels <= log2 n DIF levels are applied
 * (levels > log2 n: all of them); reorder != 0 (all levels only): natural
 * order.  Returns 0, or -1 on a bad size or allocation failure. */
int oracle_fft_hp(long double* buf, uint64_t n, uint32_t levels, int reorder) {
    if (n == 0 || (n & (n - 1))) return -1;
    const uint32_t lg = oracle_ilog2_u64(n);
    if (levels > lg) levels = lg;
    if (reorder && levels != lg) return -1;
    if (n == 1) return 0;
    long double* tw = (long double*)malloc(sizeof(long double) * n);  /* n/2 pairs */
    if (!tw) return -1;
    for (uint64_t k = 0; k < n / 2; k++) {
        const long double a = HP_TWO_PI * ((long double)k / (long double)n);
        tw[2 * k] = cosl(a);
        tw[2 * k + 1] = -sinl(a);
    }
    for (uint32_t t = 0; t < levels; t++) {
        const uint64_t s = n >> t, h = s / 2;
        for (uint64_t off = 0; off < n; off += s) {
            long double* lo = buf + 2 * off;
            long double* hi = lo + 2 * h;
            for (uint64_t b = 0; b < h; b++) {
                const long double ar = lo[2 * b], ai = lo[2 * b + 1];
                const long double cr = hi[2 * b], ci = hi[2 * b + 1];
                const long double wr = tw[2 * (b << t)], wi = tw[2 * (b << t) + 1];
                const long double dr = ar - cr, di = ai - ci;
                lo[2 * b] = ar + cr;
                lo[2 * b + 1] = ai + ci;
                hi[2 * b] = dr * wr - di * wi;
                hi[2 * b + 1] = dr * wi + di * wr;
            }
        }
    }
    free(tw);
    if (reorder) {
        for (uint64_t i = 0; i < n; i++) {
            const uint64_t j = oracle_bit_reverse(i, lg);
            if (j > i) {
                const long double r = buf[2 * i], m = buf[2 * i + 1];
                buf[2 * i] = buf[2 * j];
                buf[2 * i + 1] = buf[2 * j + 1];
                buf[2 * j] = r;
                buf[2 * j + 1] = m;
            }
        }
    }
    return 0;
}
