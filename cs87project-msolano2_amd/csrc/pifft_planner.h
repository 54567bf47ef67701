// cs87project-msolano2_amd/csrc/pifft_planner.h -- the planner's policy: which
// passes, layout, fused tree and tree table a shape gets (choose_plan), as
// plain host C++ with no HIP type or call, so that it runs on a CPU against
// any registry of instances (tests/native/planner_main.cpp).  Every measured
// rule that decides a plan lives here, with the PIFFT_* knobs that steer it;
// pifft.hip lays out the tables, assembles the launches (their own knobs: XCD
// grouping, padded workspace rows, the grid of the grid-stride kernels --
// PIFFT_TREE_GRID_DIV at the tree launches, PIFFT_STRIDE_GRID_MAX, the cap of
// every such grid, 262144 workgroups by default --, ...) and materialises them.
//
// The includer defines find_pass (the registry lookup): pifft.hip over the
// compiled instances, logging every instance found (pifft_instance_found).
#pragma once

#include "pifft_table.h"

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

namespace pifft {

const PassKernel* find_pass(int prec, int R, int C, int mode, int nts = 0, int lp = 0, int vpt = 16);

inline thread_local std::string g_err;

inline int fail(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return -1;
}

// Planner tuning variables (PIFFT_* below) are read only when PIFFT_TUNING=1
// is set: a variable inherited from a shell never changes the product's plan
// (tests/test_planner.py::test_stray_tuning_variables_are_ignored).  Each
// default is the measured winner cited where it is read.
inline bool tuning_on() {
    const char* s = getenv("PIFFT_TUNING");
    return s && s[0] == '1' && s[1] == 0;
}
inline int env_int(const char* name, int dflt) {
    if (!tuning_on()) return dflt;
    const char* s = getenv(name);
    return (s && *s) ? atoi(s) : dflt;
}

inline bool is_pow2(uint64_t x) { return x && !(x & (x - 1)); }
inline int ilog2u(uint64_t x) {
    int l = 0;
    while (x > 1) { x >>= 1; l++; }
    return l;
}

struct PassChoice {
    int R, C, mode, nts;
    int vpt = 16;
};

// Tile = R x C elements per workgroup (C adjacent lines of an R-point sub-FFT).
// Default tile 8192 (fp64) / 16384 (fp32): 128 KiB of data in registers, one
// component (64 KiB) in LDS at a time -> two workgroups per CU; at R = 512 the
// lines give 256-B contiguous row segments (the HBM-efficient width measured
// by tools/probe_bw.hip).
inline int tile_elems(int prec) {
    return env_int(prec == 64 ? "PIFFT_TILE64" : "PIFFT_TILE32", 8192);
}

// The lines per workgroup of a pass, by its role (mode 0: the single pass;
// 1, 2: a strided pass; 3: the fused tree pass).
inline int pick_lines(int prec, int R, uint64_t ntrans_lines_cap, uint64_t total_lines, int mode, int strided_tile = 0) {
    // tuning: the lines themselves, of the single pass or of every strided one
    int C = env_int(mode == 0 ? (prec == 64 ? "PIFFT_SINGLE_C64" : "PIFFT_SINGLE_C32")
                              : (prec == 64 ? "PIFFT_COL_C64" : "PIFFT_COL_C32"), 0);
    // single pass: lines are whole contiguous transforms, no segment-width
    // constraint -> small tiles (measured best: C = 4096/R, i.e. C=1 at 4096)
    int tile = mode == 0   ? env_int(prec == 64 ? "PIFFT_SINGLE_TILE64" : "PIFFT_SINGLE_TILE32", 4096)
               : mode == 1 ? env_int(prec == 64 ? "PIFFT_FIRST_TILE64" : "PIFFT_FIRST_TILE32", tile_elems(prec))
                           : tile_elems(prec);
    if (strided_tile && (mode == 1 || mode == 2)) tile = strided_tile;  // (the packed VPT-32 fp32 tile)
    // fp64 strided passes of R <= 256, not the fused tree pass (mode 3): a
    // 4096-value tile.  At 8192 (R = 256, C = 32, 512 threads) the kernel
    // spills 20 B/lane at its 128-VGPR budget; at C = 16 it runs 256 threads
    // at 138 VGPRs, 3 workgroups per CU.  Measured on MI355X
    // (profiles/r02_smallr_tile.log): 2^22 -7 %, 2^23 -12 %, 2^24 -4 %, the
    // 2^28 worker of 8 -1.5 %; the fused pass itself loses at C = 16 (156
    // VGPRs), so it keeps the 8192 tile
    if (prec == 64 && (mode == 1 || mode == 2) && R <= 256) tile = env_int("PIFFT_SMALLR_TILE64", 4096);
    if (mode == 3) mode = 1;  // the fused first pass: the first-pass tile, mode-1 line rules
    if (C <= 0) C = tile / R;
    if (C < 1) C = 1;
    if (C > 64) C = 64;
    if (R <= 8) C = 64;
    while (C > 1 && (uint64_t)C > ntrans_lines_cap && R > 8) C /= 2;
    // fill the chip: at least ~2 workgroups per CU (small transforms)
    const uint64_t min_wg = (uint64_t)env_int("PIFFT_MIN_WORKGROUPS", 512);
    // strided passes are instantiated for C >= 4 (and fp64 C = 2 at R = 512-2048, PIFFT_STRIDED_CMIN=2)
    const int cmin = mode == 0 ? 1 : env_int("PIFFT_STRIDED_CMIN", 4);
    while (C > cmin && R > 8 && total_lines / (uint64_t)C < min_wg) C /= 2;
    while (C > cmin && !find_pass(prec, R, C, mode)) C /= 2;
    return C;
}

// non-temporal streaming when a pass moves more than the Infinity Cache holds,
// and for 16-64 MiB passes (measured on MI355X, profiles/r02_nt_sweep.log:
// fp64 2^20 P=1 26 -> 24 us, P=8 44 -> 41 us, fp32 4096 x 1024 16 -> 13 us,
// the 2^21-point worker of 8 95 -> 84 us; but 8-16 MiB and 128-256 MiB passes
// lose 5-40 %)
inline int pick_nts(uint64_t pass_bytes) {
    const int force = env_int("PIFFT_NT", -1);
    if (force >= 0) return force ? 1 : 0;
    return (pass_bytes > (256ull << 20) || (pass_bytes > (16ull << 20) && pass_bytes <= (64ull << 20))) ? 1 : 0;
}

// HBM rate of a pass side, by the contiguous bytes per row segment (TB/s).
// Measured on MI355X with tools/probe_bw.hip (strided tile copies) and the
// pass kernels themselves (profiles/r01_tune_*.log); contiguous ~5.6.
inline double seg_rate(double seg_bytes) {
    if (seg_bytes >= 1024) return 5.6;
    if (seg_bytes >= 512) return 5.5;
    if (seg_bytes >= 256) return 5.3;
    if (seg_bytes >= 128) return 4.2;
    if (seg_bytes >= 64) return 2.6;
    return 1.5;
}

// Whole-pass HBM rate (TB/s, both sides) by the pass's position in a plan and
// its strided row-segment width, for HBM-bound plans without a fused tree
// (round 3).  Measured on MI355X (profiles/r03_fp64_radix_order.log,
// r03_fp32_radix_order.log; fp64 2^28 / 2^29, fp32 packed 2^28): a 256-B pass
// runs 5.9 / 5.6 / 5.25 TB/s first / in the middle / last, a 128-B one 5.0 /
// 4.8 / 4.8 -- the last pass's strided stores into the caller's unpadded
// output are slow at either width, so the narrow pass costs least there.
// fp64 2^28: 512-512-1024 4.72 ms vs 1024-512-512 4.82 (same box); fp32 2^28
// 2.47 vs 2.60 ms; fp64 2^29 9.41 vs 9.65 ms.  Same for both precisions.
inline double pass_rate(double seg_bytes, bool first, bool last) {
    if (seg_bytes >= 256) return first ? 5.9 : last ? 5.25 : 5.6;
    if (seg_bytes >= 128) return first ? 5.0 : 4.8;
    return seg_rate(seg_bytes);
}

// fp32 strided passes at 32 values per thread, packed (k_pass VPT 32): a
// 16384-value tile on 512 threads, two workgroups per CU -- the bytes and
// row-segment widths of the fp64 8192-value tile, so fp32 2^28 runs in three
// passes (1024-512-512 at C = 16/32/32) instead of four 128-point ones.
// Measured on MI355X (profiles/r03_fp32_packed_vpt32.log): fp32 2^28 3.36 ->
// 2.67 ms, 2^30 13.7 -> 11.6 ms; 2^26 (512 MiB per side) 0.63 -> 0.65 ms.
// The rule: data beyond 1 GiB per side, no fused tree pass (no packed MODE 3
// instances).  PIFFT_VPT32: -1 this rule, 0 never, 1 whenever instantiated.
inline bool use_vpt32(int prec, uint64_t M, uint64_t ntrans, int heavy_lp) {
    const int force = env_int("PIFFT_VPT32", -1);
    if (prec != 32 || heavy_lp || force == 0) return false;
    return force == 1 || ntrans * M * 8 >= (1ull << 30);
}

// A local FFT being planned: ntrans transforms of M = 2^logm points.
// heavy_lp: the first pass also evaluates the tree (reads P leaves per input,
// P = 2^heavy_lp), so its read side dominates.
struct LocalFft {
    uint64_t M, ntrans;
    int prec, logm, heavy_lp;
    size_t esz;
    int nts;  // pick_nts of the bytes a pass moves
};

inline uint64_t pass_workgroups(const LocalFft& f, const PassChoice& pc) {
    return (f.ntrans * (f.M / (uint64_t)pc.R) + pc.C - 1) / (uint64_t)pc.C;
}

// The lines of a strided pass of radix 2^bits (stile: the packed VPT-32 tile, or 0).
inline int strided_lines(const LocalFft& f, int bits, bool first, int stile) {
    const int role = first ? (f.heavy_lp ? 3 : 1) : 2;
    return pick_lines(f.prec, 1 << bits, f.M >> bits, f.ntrans * (f.M >> bits), role, stile);
}

// M fits one LDS/register-resident pass.
inline int single_pass(const LocalFft& f, std::vector<PassChoice>& out) {
    const int R = (int)f.M;
    const int C = pick_lines(f.prec, R, f.ntrans, f.ntrans, 0);
    if (!find_pass(f.prec, R, C, 0, f.nts)) return fail("no pass kernel for R=%d C=%d", R, C);
    // tuning: 8 values per thread (radix-8 stages, twice the waves per
    // sub-FFT) -- measured slower than 16 at every batch size
    // (profiles/r02_vpt_sweep.log), so only on request and if instantiated
    const int vpt = env_int("PIFFT_SINGLE_VPT", 16);
    const bool instantiated = vpt != 16 && find_pass(f.prec, R, C, 0, f.nts, 0, vpt);
    out.push_back({R, C, 0, f.nts, instantiated ? vpt : 16});
    return 0;
}

// tuning: explicit log2 radices, e.g. PIFFT_RADIX_LOGS=10,10,8 (must sum to log2 M)
// Returns 1 where they applied, 0 where not, -1 where a pass has no instance.
inline int explicit_radices(const LocalFft& f, int stile, std::vector<PassChoice>& out) {
    const char* rl = tuning_on() ? getenv("PIFFT_RADIX_LOGS") : nullptr;
    if (!rl) return 0;
    std::vector<int> logs;
    for (const char* c = rl; *c;) {
        char* end = nullptr;
        const long v = strtol(c, &end, 10);
        if (end == c) break;
        logs.push_back((int)v);
        c = *end ? end + 1 : end;
    }
    int sum = 0;
    for (int l : logs) sum += l;
    if (sum != f.logm || logs.size() <= 1) return 0;
    for (size_t p = 0; p < logs.size(); p++) {
        const int R = 1 << logs[p], mode = p == 0 ? 1 : 2;
        const int C = strided_lines(f, logs[p], p == 0, stile);
        if (!find_pass(f.prec, R, C, mode, f.nts)) return fail("no pass kernel R=%d C=%d", R, C);
        out.push_back({R, C, mode, f.nts});
    }
    return 1;
}

// log2 of pass p's radix where 2^logm splits into k balanced passes
// (order 0: larger radices first, 1: smaller first)
inline int radix_bits(int logm, int k, int order, int p) {
    const int base = logm / k, extra = logm % k;
    return order ? base + (p >= k - extra ? 1 : 0) : base + (p < extra ? 1 : 0);
}

// One candidate, k passes in one order: its passes and its cost by the
// bandwidth model (each pass moves its bytes at the rate of its narrowest
// strided side, C*esz-byte row segments; or, pos, at the position-aware
// rates).  False where a pass has no instance.
// the position rates were measured on passes of >= 128-B segments:
// a candidate with a narrower pass keeps the segment-width model
inline bool price_candidate(const LocalFft& f, int k, int order, int stile, bool pos, std::vector<PassChoice>& cand,
                            double& cost) {
    // (the lines of every pass up to the first without an instance, and, for
    // pos, up to the first narrow one)
    bool ok = true;
    for (int p = 0; p < k && (ok || pos); p++) {
        const int bits = radix_bits(f.logm, k, order, p), mode = p == 0 ? 1 : 2;
        const int C = strided_lines(f, bits, p == 0, stile);
        if (pos) pos = (size_t)C * f.esz >= 128;
        ok = ok && find_pass(f.prec, 1 << bits, C, mode, f.nts);
        if (ok) cand.push_back({1 << bits, C, mode, f.nts});
    }
    if (!ok) return false;
    cost = 0.0;
    for (int p = 0; p < k; p++) {
        const int C = cand[p].C;
        const double rs = seg_rate((double)C * f.esz);                 // strided side
        const double side = (double)f.ntrans * f.M * f.esz * 1e-12;  // TB per side
        const double reads = (p == 0 && f.heavy_lp) ? side * (1 << f.heavy_lp) : side;
        if (pos)
            cost += 2 * side / pass_rate((double)C * f.esz, p == 0, p == k - 1);
        else
            cost += reads / rs + side / (p == 0 ? 5.6 : rs);
    }
    return true;
}

// a fused tree+first pass runs best with the larger radix (R = 512,
// C = 16) first: measured 1-3 % over the model's pick at P = 4, 8.
// Not when that radix leaves the P-fold leaf reads narrower than
// 256-B segments (R = 1024, C = 8 at fp64): then the model picks
// between both orders (config 5, 2^29 per worker: 512-1024-1024
// 19.7 ms vs 256-128-128-128 21.3 ms, profiles/r01_tune_c5.log).
// fp64 only: the fp32 tile gives R = 1024 128-B segments too, but
// the other order there loses the fused kernel (no instance)
inline bool fused_first_pass_wants_larger_radix(const LocalFft& f, int k) {
    const int C0 = strided_lines(f, radix_bits(f.logm, k, 0, 0), true, 0);
    return f.prec != 64 || (size_t)C0 * f.esz >= 256;  // fp32: measured cases only
}

// k Stockham passes with balanced radices, k and the radix order chosen by
// the bandwidth model (price_candidate).
// pos_ok: the position-aware pass rates may price this plan (not for the
// worker-interleaved layout, whose passes move rows of all workers: there the
// narrow pass last measured 1-14 % slower, profiles/r03_pos_model_shapes.log)
inline void modelled_passes(const LocalFft& f, int stile, bool pos_ok, std::vector<PassChoice>& out) {
    const int rmax_log = env_int(f.prec == 64 ? "PIFFT_COL_RMAX_LOG64" : "PIFFT_COL_RMAX_LOG32", 10);
    const int kmin = (f.logm + rmax_log - 1) / rmax_log;
    const int kforce = env_int("PIFFT_PASSES", 0);  // tuning: this many passes
    // data that stays in the 256 MiB Infinity Cache is not bound by HBM row
    // segments: fewest passes there
    const bool resident = 2 * f.ntrans * f.M * f.esz <= (256ull << 20);
    const int kfirst = kforce > 0 ? kforce : kmin, klast = kforce > 0 ? kforce : resident ? kmin : kmin + 1;
    const int force_order = env_int("PIFFT_ORDER", -1);  // tuning: 0 or 1 only
    const bool pos = pos_ok && !resident && !f.heavy_lp && env_int("PIFFT_POS_MODEL", 1);
    double best = 1e300;
    for (int k = kfirst; k <= klast; k++) {
        if (f.logm < 4 * k) break;  // every radix >= 16
        for (int order = 0; order < 2; order++) {  // 0: larger radices first, 1: smaller first
            if (force_order >= 0 && order != force_order) continue;
            if (force_order < 0 && f.heavy_lp > 0 && order == 1 && fused_first_pass_wants_larger_radix(f, k)) continue;
            std::vector<PassChoice> cand;
            double cost;
            if (price_candidate(f, k, order, stile, pos, cand, cost) && cost < best) {
                best = cost;
                out = cand;
            }
        }
    }
}

// The strided passes of a multi-pass local FFT at one tile size.
inline int strided_passes(const LocalFft& f, int stile, bool pos_ok, std::vector<PassChoice>& out) {
    out.clear();
    const int given = explicit_radices(f, stile, out);
    if (given < 0) return -1;
    if (!given) modelled_passes(f, stile, pos_ok, out);
    if (out.empty()) return fail("no pass decomposition for M=2^%d", f.logm);
    return 0;
}

// the packed VPT-32 passes for the 16384-value tile (every strided pass
// must have its instance, else the plan is redone at the 8192 tile)
inline bool pack_vpt32(const LocalFft& f, std::vector<PassChoice>& out) {
    for (auto& pc : out) {
        if (pc.mode != 1 && pc.mode != 2) continue;
        if (!find_pass(f.prec, pc.R, pc.C, pc.mode, pc.nts, 0, 32)) return false;
        pc.vpt = 32;
    }
    return true;
}

// The fused tree pass of a small one-worker slice at 8 values per thread
// (radix-8 stages, twice the waves per workgroup) when it has R <= 512
// points and at most 128 workgroups: a latency-bound launch on a fraction
// of the CUs, whose P leaf loads and tree per value then spread over twice
// the threads.  Measured on MI355X (profiles/r04d_fused_vpt8.log): fp64
// local 2^15-2^18 +4.5-31 % (config 2's slice 14.05 -> 12.66 us), fp32
// +0.6-4 %; R = 1024 -2-3 %, 256 workgroups ties.  PIFFT_FUSED_VPT: the
// values per thread instead (tuning).
inline void small_fused_slice_vpt8(const LocalFft& f, std::vector<PassChoice>& out) {
    if (!f.heavy_lp || out[0].mode != 1) return;
    PassChoice& pc = out[0];
    const int fvpt = env_int("PIFFT_FUSED_VPT", (pc.R <= 512 && pass_workgroups(f, pc) <= 128) ? 8 : 16);
    if (fvpt != pc.vpt && find_pass(f.prec, pc.R, pc.C, 3, pc.nts, f.heavy_lp, fvpt)) pc.vpt = fvpt;
}

// The last strided pass of a small fp64 plan (R <= 512, <= 256
// workgroups) at 8 values per thread too: measured on MI355X
// (profiles/r04k_slice.log, r04k_shapes.log) config 2's one-GPU slice
// 12.7 -> 12.2 us (+3.8 %), fp64 slices of local 2^16-2^19 +1.6-5 %, P = 1
// 2^16-2^18 +5-6 %; 4 values per thread +2.6 % (slice).  PIFFT_LAST_VPT:
// the values per thread instead (tuning, below).
inline void small_fp64_last_pass_vpt8(const LocalFft& f, std::vector<PassChoice>& out) {
    PassChoice& pc = out.back();
    if (f.prec != 64 || out.size() <= 1 || pc.mode != 2 || pc.vpt != 16) return;
    if (pc.R <= 512 && pass_workgroups(f, pc) <= 256 && find_pass(f.prec, pc.R, pc.C, 2, pc.nts, 0, 8)) pc.vpt = 8;
}

// tuning: lines per workgroup (its write side's segment width) and values
// per thread of the last pass
inline void last_pass_override(const LocalFft& f, std::vector<PassChoice>& out) {
    const int last_c = env_int("PIFFT_LAST_C", 0), last_vpt = env_int("PIFFT_LAST_VPT", 0);
    if ((last_c <= 0 && last_vpt <= 0) || out.size() <= 1) return;
    PassChoice& b = out.back();
    const int c = last_c > 0 ? last_c : b.C, v = last_vpt > 0 ? last_vpt : b.vpt;
    if (find_pass(f.prec, b.R, c, b.mode, b.nts, 0, v)) {
        b.C = c;
        b.vpt = v;
    }
}

// Local FFT of length M as passes.  A single LDS/register-resident pass when M
// fits (M <= 2^14); otherwise k Stockham passes with balanced radices, k and
// the radix order chosen by a bandwidth model: each pass moves its bytes at
// the rate of its narrowest strided side (C*esz-byte row segments).
// heavy_first: the first pass also evaluates the tree (reads P leaves per
// input, P = 2^lp), so its read side dominates.
// single_max: the longest one-pass local FFT (log2; default 14, PIFFT_SINGLE_MAX_LOG)
inline int plan_passes(uint64_t M, int prec, uint64_t ntrans, std::vector<PassChoice>& out, int heavy_lp = 0,
                       bool allow_v32 = true, bool pos_ok = true, int single_max = -1) {
    out.clear();
    if (M <= 1) return 0;
    const size_t esz = prec == 64 ? 16 : 8;
    const LocalFft f = {M, ntrans, prec, ilog2u(M), heavy_lp, esz, pick_nts(2 * ntrans * M * esz)};
    if (single_max < 0) single_max = env_int("PIFFT_SINGLE_MAX_LOG", 14);
    if (f.logm <= single_max) return single_pass(f, out);
    const bool v32 = allow_v32 && use_vpt32(prec, M, ntrans, heavy_lp);
    if (strided_passes(f, v32 ? 16384 : 0, pos_ok, out)) return -1;
    if (v32 && !pack_vpt32(f, out) && strided_passes(f, 0, pos_ok, out)) return -1;
    small_fused_slice_vpt8(f, out);
    small_fp64_last_pass_vpt8(f, out);
    last_pass_override(f, out);
    return 0;
}

// What is planned: transform length, workers, the plan's worker range, batch,
// precision and output order (plan_shape derives the rest).
struct PlanShape {
    uint64_t n = 0, m = 0;  // N and the local length M = N / P
    uint32_t P = 1, q0 = 0, nq = 1, batch = 1;
    int prec = 64;
    int lp = 0, log_n = 0, log_m = 0;
    size_t esz = 16;
    bool natural = true;
    bool bitrev = false;         // PIFFT_OUT_BITREV
    bool separate_tree = false;  // PIFFT_SEPARATE_TREE: never fuse the tree into a pass
};

inline PlanShape plan_shape(uint64_t n, uint32_t workers, uint32_t first, uint32_t count, uint32_t batch, int prec,
                            bool natural, bool bitrev, bool separate_tree) {
    PlanShape s;
    s.n = n;
    s.P = workers;
    s.q0 = first;
    s.nq = count;
    s.batch = batch;
    s.prec = prec;
    s.natural = natural;
    s.bitrev = bitrev;
    s.separate_tree = separate_tree;
    s.esz = prec == 64 ? 16 : 8;
    s.lp = ilog2u(workers);
    s.log_n = ilog2u(n);
    s.log_m = s.log_n - s.lp;
    s.m = n >> s.lp;
    return s;
}

// the tree evaluated inside the first pass: by one worker's pass (MODE 3) or
// by the worker-interleaved plan's, for all workers (MODE 11, C lines a tile)
enum { FUSED_NONE = 0, FUSED_ONE_WORKER = 1, FUSED_ALL_WORKERS = 2 };
// the tree's twiddles: the reference-formula table, the two-level w_N, or
// (TREE_TW_WIL_FACTORED) the reference table for the stand-alone tree and the
// two-level one for the worker-interleaved plan's own tree
enum { TREE_TW_NONE = 0, TREE_TW_DIRECT = 1, TREE_TW_FACTORED = 2, TREE_TW_WIL_FACTORED = 3 };

// What choose_plan decides; everything after it is bookkeeping.
struct PlanChoice {
    std::vector<const PassKernel*> passes;  // the instance each pass launches (the fused one first, if any)
    bool wil = false;  // worker-interleaved layout (PassArgs::wil, MODE | 8 passes)
    bool ilv = false;  // the last pass stores natural order itself (PassArgs::ilv_log)
    int fused = FUSED_NONE;
    int tree_tw = TREE_TW_NONE;
};

// What choose_plan's rules hand on to each other.
struct PlanDraft {
    std::vector<PassChoice> passes;
    bool wil = false;          // worker-interleaved layout
    uint32_t fused_lines = 0;  // the all-worker fused first pass's lines per tile, J P (0: no such pass)
};

inline uint64_t local_transforms(const PlanShape& s) { return (uint64_t)s.batch * s.nq; }

// All P <= 16 workers of a natural-order plan on this GPU, with a
// multi-pass local FFT: the worker-interleaved layout (PassArgs::wil).
// The tree's one launch writes z_q[i] at i P + q, every pass reads and
// writes rows holding all workers' values side by side, and the last pass
// stores worker q at slot bitrev(q) -- the natural-order result, without
// an interleave launch or scattered 16-B stores.  PIFFT_WORKER_IL=0: the
// slice-major layout (+ interleave launch or natural-order store).
inline bool wil_ok(const PlanShape& s) {
    return s.natural && s.P > 1 && s.nq == s.P && s.lp <= 4 && env_int("PIFFT_WORKER_IL", 1);
}
// (P = 32 too, one launch only: two threads per position, each evaluating
// the tree pruned to half the workers)
inline bool wil_ok5(const PlanShape& s) {
    return s.natural && s.P > 1 && s.nq == s.P && s.lp == 5 && env_int("PIFFT_WORKER_IL", 1);
}
// One worker per plan: the tree is fused into the first pass, which reads
// the input once.  (Several workers per plan re-reading all P leaves in
// each worker's fused pass measured no consistent win, profiles/
// r02_fuse_all.log; removed in round 4.)
inline bool may_fuse(const PlanShape& s) {
    return s.P > 1 && s.nq == 1 && s.lp <= 4 && !s.separate_tree && env_int("PIFFT_FUSE_TREE", 1);
}
// the worker-interleaved plan may take its tree into its first pass (MODE 11)
inline bool wil_may_fuse(const PlanShape& s) { return !s.separate_tree && env_int("PIFFT_WIL_FUSE", 1); }

// the same radices, every pass a worker-interleaved MODE 2 (| 8) pass at
// the C of a MODE 2 pass whose lines run over all workers
inline bool to_wil(const PlanShape& s, std::vector<PassChoice>& w) {
    bool ok = true;
    for (auto& pc : w) {
        const uint64_t lines = s.m / (uint64_t)pc.R;
        pc.C = pick_lines(s.prec, pc.R, lines << s.lp, local_transforms(s) * lines, 2);
        pc.mode = 2 | 8;
        pc.vpt = 16;
        // tuning: at least this many lines per workgroup (e.g. P, so a
        // row holds every worker's value), if instantiated
        // (default P: 8 workers at C = 8 instead of 4 -- C2 35 -> 32 us,
        // fp32 2^20 P = 8 25 -> 24 us, 2^28 P = 8 unchanged at C = 16;
        // profiles/r03_worker_interleaved.log)
        const int cmin = env_int("PIFFT_WIL_CMIN", (int)s.P);
        if (cmin > pc.C && find_pass(s.prec, pc.R, cmin, pc.mode, pc.nts)) pc.C = cmin;
        ok = ok && find_pass(s.prec, pc.R, pc.C, pc.mode, pc.nts) != nullptr;
        // config-2-sized plans (<= 32 MiB of data): 8 values per thread
        // where instantiated (config 2 29.9 -> 29.0 us, profiles/
        // r04d_wil_vpt8_c2.log); PIFFT_WIL_VPT: instead (tuning)
        const bool small = (uint64_t)s.batch * s.n * s.esz <= (32ull << 20);
        const int wvpt = env_int("PIFFT_WIL_VPT", small ? 8 : 16);
        if (wvpt != pc.vpt && find_pass(s.prec, pc.R, pc.C, pc.mode, pc.nts, 0, wvpt)) pc.vpt = wvpt;
    }
    return ok;
}

// The multi-pass local FFT in the worker-interleaved layout, where every pass has its instance.
inline void worker_interleave(const PlanShape& s, PlanDraft& d) {
    std::vector<PassChoice> w = d.passes;
    if (!to_wil(s, w)) return;
    d.passes = w;
    d.wil = true;
}

// A single transform whose local FFT is one pass (M <= 2^14) would run
// tree + pass + interleave launches.  From M = 2^11 up the
// worker-interleaved plan with every worker's tree fused into its first
// pass (MODE 11 below: the first radix, then an M / R1-point pass) does
// it in two, kept only where that fused plan exists (round 5,
// profiles/r05w_small_wil.log: fp64 2^15 P = 2 22 -> 13 us, 2^16 P = 4
// 23 -> 11, 2^17 P = 8 25 -> 12; fp32 2^17 P = 8 21 -> 9, 2^18 P = 16
// 25 -> 13; 9-30 % at the other sizes).  PIFFT_WIL_SINGLE=0: off.
// And a transform that fits one tile (P M <= 8192 values, from 1024: the
// reference's own GPU sweep, cuda/run-experiments:16) runs every worker's
// tree and its whole M-point FFT in ONE launch: the fused pass at J = 1 (C
// = P lines of R = M points) storing natural order (PIFFT_WIL_ONE_LAUNCH=0:
// off).  Batched, one workgroup per transform: 1.2-2.8x faster than tree +
// pass (profiles/r05bo_batched_one_launch_ab.log; PIFFT_WIL_ONE_BATCH=0: off);
// and batched two-pass plans 11-40 % (r05bt_batched_two_pass_ab.log;
// PIFFT_WIL_SINGLE_BATCH=0: off).
// The two-pass plan from M = 2^11 (fp64 2^14 P = 8 11 -> 10 us, fp32 8 vs
// 11, fp32 2^15 P = 16 12 vs 14: profiles/r05za_small_plan_edges.log).
// (PIFFT_WIL_ONE_MAX: the largest one-launch transform, values -- 16384
// measured slower; the instances exist only where they compile spill-free.
// PIFFT_WIL_SINGLE_MIN_LOG: the two-pass plan's smallest M, log2.  Tuning.)
//
// The one-launch pass of a shape, were it planned: its values per thread (0:
// no instance) and streaming form.
inline PassChoice one_launch_pass(const PlanShape& s) {
    int nts0 = pick_nts(2 * local_transforms(s) * s.m * s.esz);
    // (fp64 P = 2 at M = 4096 spills at 16 values per thread: 8, 1024 threads,
    // batched only -- 64 transforms 21 -> 13 us, one 10 -> 12: profiles/r05v8_*)
    const int vpt0 = find_pass(s.prec, (int)s.m, (int)s.P, 11, 0, s.lp) ? 16 : s.batch >= 64 ? 8 : 0;
    if (nts0 && !find_pass(s.prec, (int)s.m, (int)s.P, 11, nts0, s.lp, vpt0)) nts0 = 0;  // (nt forms not instantiated)
    return {(int)s.m, (int)s.P, 11, nts0, vpt0};
}
// single: the local FFT was planned as one pass; one: one_launch_pass(s)
inline bool one_ok(const PlanShape& s, bool single, const PassChoice& one) {
    const uint64_t pm = (uint64_t)s.P * s.m;
    return (wil_ok(s) || wil_ok5(s)) && single && pm >= 1024 && pm <= (uint64_t)env_int("PIFFT_WIL_ONE_MAX", 8192) &&
           env_int("PIFFT_WIL_ONE_LAUNCH", 1) && find_pass(s.prec, one.R, one.C, 11, one.nts, s.lp, one.vpt);
}
// the one-pass local FFT leaves the slice-major layout: for the one-launch
// plan (one: one_ok), the two-pass fused plan or the P = 16 fallback
inline bool wil_single(const PlanShape& s, bool single, bool one) {
    return (wil_ok(s) || one) && single && env_int("PIFFT_WIL_SINGLE", 1) &&
           (((s.batch == 1 || env_int("PIFFT_WIL_SINGLE_BATCH", 1)) &&
             s.m >= (1ull << env_int("PIFFT_WIL_SINGLE_MIN_LOG", 11))) ||
            (one && (s.batch == 1 || env_int("PIFFT_WIL_ONE_BATCH", 1))));
}

// The one-launch plan: every worker's tree and whole local FFT in the fused pass at J = 1.
inline void one_launch_plan(const PlanShape& s, const PassChoice& one, PlanDraft& d) {
    if (!wil_may_fuse(s)) return;
    d.passes = {one};
    d.wil = true;
    d.fused_lines = s.P;
}

// J by measurement (round 5,
// profiles/r05m_wil_fuse_j.log, the separate tree launch in brackets):
//   fp64, J = 8: config 2 (2^20 P = 8) 26 us (29), 2^20 P = 4 23 (31),
//     P = 2 25 (31), 2^24 P = 8 310 (381), 2^26 P = 4 1.18 ms (1.50),
//     2^28 P = 8 4.98 ms (6.31), P = 16 5.84 (6.13); but P = 16 below
//     256 MiB ties or loses (2^20: 28-45 vs 26 us) -> separate there;
//     J = 16 (256-B leaf rows, first radix 64 at P = 8) loses on the
//     remaining passes it leaves (a 1024 / 2048 pass at 8 lines);
//   fp32: J = 8 up to 32 MiB (2^20 P = 8 20 vs 24 us), J = 16 up to
//     1 GiB (2^24 P = 8 165 vs 208 us); 2^28 P = 8 keeps the separate tree
//     (3.26 vs 3.39-3.51 ms: its remaining passes at 8-B values get
//     128-B rows).
// Two refinements for P <= 8 (round 5, profiles/r05s_*, r05t_*, r05u_*;
// every output checked against the default plan's):
//   - where the 8192-value tile leaves fewer than 256 workgroups (<= 2^20
//     values: 128), the tile is halved and J = 4, so every CU gets one:
//     config 2 26 -> 23 us, fp64 2^20 P = 4 23 -> 21, P = 2 25 -> 23,
//     2^19 P = 8 21 -> 18, 2^18 P = 8 16 -> 14; fp32 2^20 P = 2-8 -1 us;
//   - where J = 8 leaves a remainder the rest of the plan splits in two
//     passes (> 2048 points) and J = 4 leaves one pass: J = 4 (fp64 2^22
//     P = 2 / 4 / 8: 68 / 65 / 64 -> 54 / 51 / 50 us); fp32 at P = 8 from a
//     2048-point remainder on (2^21 27 -> 24 us, 2^22 51 -> 42).  (fp32 at
//     P <= 4 keeps J = 8: its J = 4 remainder passes run at 4 lines, 32-B
//     rows: 2^22 P = 4 50 -> 75 us.)
struct FusedTile {
    int J, tile;  // J line indices x P workers of a tile of this many values (J = 0: no fused pass)
};
inline FusedTile wil_fuse_tile(const PlanShape& s) {
    const uint64_t data = (uint64_t)s.batch * s.n * s.esz;
    const int jdef = s.prec == 64 ? ((s.lp <= 3 || data >= (256ull << 20)) ? 8 : 0)
                                   : (data <= (32ull << 20) ? 8 : data <= (1ull << 30) ? 16 : 0);
    int J = jdef, tile1 = tile_elems(s.prec);
    if (jdef == 8 && s.lp <= 3) {
        const uint64_t rest8 = s.m / (uint64_t)(tile1 / (8 << s.lp)), rest4 = rest8 / 2;
        if ((uint64_t)s.batch * s.n / (uint64_t)tile1 < 256) {
            tile1 /= 2;
            J = 4;
        } else if (rest8 > (s.prec == 64 ? 2048u : 1024u) && rest4 <= 2048 && (s.prec == 64 || s.lp == 3)) {
            J = 4;
        }
    } else if (jdef == 8 && s.lp == 4) {
        // fp32 P = 16: J = 4 where it leaves a remainder of at most 1024
        // points (2^21: 41 -> 26 us; at 2048 its 4-line pass loses, 2^22
        // 52 -> 90, r05u_wil_fuse_remainder.log)
        const uint64_t rest8 = s.m / (uint64_t)(tile1 / (8 << s.lp));
        if (rest8 > 1024 && rest8 / 2 <= 1024) J = 4;
    } else if (jdef == 0 && s.lp == 4 && s.prec == 64 && data >= (32ull << 20) && data <= (64ull << 20)) {
        J = 2;  // fp64 P = 16 at 32-64 MiB: fused at J = 2 (2^21 43 -> 37 us, 2^22 70 -> 65; 2^23 loses)
    }
    return {J, tile1};
}

// The worker-interleaved plan with its tree fused into the first pass
// (MODE 11, k_pass wil_tree_to_lds): a tile of J adjacent line indices x
// all P workers loads each position's P leaves once (J esz-byte leaf
// rows) and evaluates every worker's tree there, so the tree launch (N
// read + N written) and the first pass's re-read of its output are gone.
// The first radix is what that tile leaves (8192 / (J P)), the rest of
// the local FFT is planned as usual.  J: wil_fuse_tile.
// PIFFT_SEPARATE_TREE (CLI -u) or PIFFT_WIL_FUSE=0: the separate tree
// launch; PIFFT_WIL_FUSE_J: J (then the tile stays 8192 unless
// PIFFT_WIL_FUSE_TILE says otherwise), PIFFT_WIL_FUSE_TILE: the tile
// (values), PIFFT_WIL_FUSE_VPT: values per thread (tuning, tests).
inline void fuse_all_workers(const PlanShape& s, PlanDraft& d) {
    if (!wil_may_fuse(s)) return;
    FusedTile t = wil_fuse_tile(s);
    const int jenv = env_int("PIFFT_WIL_FUSE_J", -1);
    if (jenv >= 0) t = {jenv, tile_elems(s.prec)};
    t.tile = env_int("PIFFT_WIL_FUSE_TILE", t.tile);
    const uint64_t ntrans = local_transforms(s);
    const int C1 = t.J > 0 ? t.J << s.lp : 0;
    const int R1 = C1 > 0 ? t.tile / C1 : 0;
    const int vpt1 = env_int("PIFFT_WIL_FUSE_VPT", 16);
    const int nts1 = pick_nts(2 * ntrans * s.m * s.esz);
    std::vector<PassChoice> rest;
    const uint64_t m2 = R1 > 0 ? s.m / (uint64_t)R1 : 0;
    const bool ok = R1 >= 16 && (uint64_t)R1 < s.m && m2 >= (uint64_t)t.J &&
                    find_pass(s.prec, R1, C1, 11, nts1, s.lp, vpt1) &&
                    plan_passes(m2, s.prec, ntrans * (uint64_t)R1, rest, 0, false, false) == 0;
    if (!ok) return;
    // (worker-interleaved passes exist up to R = 2048: a longer single
    // remainder becomes two balanced passes)
    if (rest.size() == 1 && rest[0].R > 2048) {
        const int l = ilog2u(m2);
        rest = {PassChoice{1 << ((l + 1) / 2), 0, 2, rest[0].nts}, PassChoice{1 << (l / 2), 0, 2, rest[0].nts}};
    }
    if (!to_wil(s, rest)) return;
    d.passes.clear();
    d.passes.push_back({R1, C1, 11, nts1, vpt1});
    for (const auto& pc : rest) d.passes.push_back(pc);
    d.wil = true;
    d.fused_lines = (uint32_t)C1;
}

// no fused plan: the single pass -- except P = 16 at fp64 (no fused
// pass below 256 MiB, above), where the worker-interleaved two-pass
// plan after its tree launch still saves the interleave launch (2^16
// 16 -> 15 us, 2^17 21 -> 16, 2^18 30 -> 19; r05w_small_wil.log)
inline void p16_two_pass_plan(const PlanShape& s, PlanDraft& d) {
    std::vector<PassChoice> w;
    if (s.lp != 4 || s.batch != 1 || s.m < 4096) return;
    if (plan_passes(s.m, s.prec, local_transforms(s), w, 0, false, false, ilog2u(s.m) - 1) || w.size() != 2) return;
    if (!to_wil(s, w)) return;
    d.passes = w;
    d.wil = true;
}

// the last pass stores in bit-reversed order: its MODE | 4 twin, at
// the planned C or the widest instantiated one below it
inline int bitrev_last_pass(const PlanShape& s, PlanDraft& d) {
    if (!s.bitrev || d.passes.empty()) return 0;
    PassChoice& l = d.passes.back();
    const int bm = l.mode, cmin = bm == 0 ? 1 : 4;
    if (l.vpt == 8 && !find_pass(s.prec, l.R, l.C, bm | 4, l.nts, 0, 8)) l.vpt = 16;  // (no VPT-8 twin)
    int C = l.C;
    while (C > cmin && !find_pass(s.prec, l.R, C, bm | 4, l.nts, 0, l.vpt)) C /= 2;
    if (!find_pass(s.prec, l.R, C, bm | 4, l.nts, 0, l.vpt))
        return fail("no bit-reversed pass kernel R=%d C=%d mode=%d", l.R, l.C, bm);
    l.C = C;
    l.mode = bm | 4;
    return 0;
}

// All P workers on this plan, natural order, and an output small enough to
// stay in L2 / the Infinity Cache: the last pass stores each worker's bins
// at their natural positions bitrev(q) + P k itself (plain stores; the P
// workers' tiles of a line block back to back on one XCD) instead of a
// slice-major store plus an interleave launch.  Measured on MI355X
// (profiles/r02_ilv_store.log, wall per transform): fp64 2^18-2^22 P=2-16
// 1-22 % faster, fp32 2^20 P=8 7 %, batched single-pass plans (4096 x
// 4096 fp32 P=4, 1024 x 2^12 fp64 P=4) 13-16 %; 2^23 fp64 and 2^22 fp32
// (32 MiB) single transforms up to 5 % slower, few tiles (2^16: 8) 12 %.
// PIFFT_ILV: -1 this rule, 0 never, 1 always (where it applies).
inline bool natural_store(const PlanShape& s, PlanDraft& d) {
    const int force = env_int("PIFFT_ILV", -1);
    const bool ok = s.natural && s.P > 1 && s.nq == s.P && !d.passes.empty() && !d.wil;
    bool on = ok && force == 1;
    if (ok && force < 0) {
        const PassChoice& l = d.passes.back();
        const uint64_t tiles = (local_transforms(s) * (s.m / (uint64_t)l.R) + l.C - 1) / (uint64_t)l.C;
        const uint64_t cap_mib = d.passes.size() == 1 ? (uint64_t)env_int("PIFFT_ILV_SINGLE_MAX_MIB", 128)
                                 : s.prec == 64      ? (uint64_t)env_int("PIFFT_ILV_MAX_MIB64", 64)
                                                      : (uint64_t)env_int("PIFFT_ILV_MAX_MIB32", 16);
        on = tiles >= (uint64_t)env_int("PIFFT_ILV_MIN_TILES", 256) &&
             (uint64_t)s.batch * s.n * s.esz <= (cap_mib << 20);
    }
    if (on) d.passes.back().nts = 0;
    return on;
}

// --- tree tables (w_N) ---
// The worker-interleaved plan's one tree launch (k_tree_wil) feeds its
// passes only -- its output is never observed, and the plan's result
// matches the oracle within tolerance either way -- so from 2^21 values
// up it takes the factored two-level twiddles (one small-table lookup per
// level and thread) instead of the reference-formula table, whose
// N (1 - 1/P) entries it otherwise reads beside the data (C2: 1.44x its
// algorithmic bytes, profiles/r05b_traffic_n2^20_f64_b1_P8_q8.json).
// Measured on MI355X (profiles/r05g_wil_tree.log): fp64 2^21 P = 8
// 46 -> 42 us, 2^22 P = 16 80 -> 70 us; but config 2 itself (fp64 2^20,
// P = 8: 512 workgroups, one round, latency-bound) 29 -> 31 us -- there
// the extra dependent fp64 products sit on the critical path -- and 2^18
// ties.  The stand-alone tree (pifft_tree_device) keeps the reference
// table and stays bitwise.  PIFFT_WIL_TREE_DIRECT=1: the reference table
// at every size (tuning, tests); PIFFT_WIL_TREE_MIN_LOG: the threshold.
inline int tree_table(const PlanShape& s, bool wil) {
    if (s.P <= 1) return TREE_TW_NONE;
    const int direct_max = env_int("PIFFT_TREE_DIRECT_MAX_LOG", 22);
    if (s.log_n > direct_max) return TREE_TW_FACTORED;
    // (and at P = 32, whose one-launch pass evaluates 16 workers' tree
    // per thread: 80 dependent table lookups each, against 5: 2^10
    // 12 -> 8 us, fp32 11 -> 6; P = 16 ties, profiles/r05p32b_*)
    const bool wil_factored = wil && env_int("PIFFT_WIL_TREE_DIRECT", 0) == 0 &&
                   ((uint64_t)s.batch * s.n >= (1ull << env_int("PIFFT_WIL_TREE_MIN_LOG", 21)) || s.lp == 5);
    return wil_factored ? TREE_TW_WIL_FACTORED : TREE_TW_DIRECT;
}

// One worker on this plan, a multi-pass local FFT and log2 P <= 4: fuse the
// tree into the first pass (its P leaves per input instead of a separate
// tree launch that writes, and a pass that re-reads, the N/P segment).
// (Or all workers': the draft's MODE 11 first pass.)  The fused instance, if any.
inline const PassKernel* fused_tree_pass(const PlanShape& s, const PlanDraft& d) {
    const PassKernel* fused = nullptr;
    if (d.passes.empty()) return fused;
    const PassChoice& p0 = d.passes[0];
    if (may_fuse(s) && d.passes.size() > 1) fused = find_pass(s.prec, p0.R, p0.C, 3, p0.nts, s.lp, p0.vpt);
    if (d.fused_lines) fused = find_pass(s.prec, p0.R, p0.C, 11, p0.nts, s.lp, p0.vpt);
    return fused;
}

// --- the instance each pass launches ---
inline int resolve_instances(const PlanShape& s, const PlanDraft& d, const PassKernel* fused,
                             std::vector<const PassKernel*>& out) {
    const std::vector<PassChoice>& passes = d.passes;
    for (size_t i = 0; i < passes.size(); i++) {
        const bool fuse_here = (i == 0 && fused);
        const bool last_pass = i + 1 == passes.size() && passes.size() > 1;
        // tuning: the last pass's streaming form (0 plain, 1 nt both, 2 nt loads, 3 nt stores)
        int nt_override = last_pass && passes[i].mode == 2 ? env_int("PIFFT_LAST_NT", -1) : -1;
        // (and the first pass's, 0 plain / 1 nt both, of a plan without a fused tree; round 6,
        // profiles/r06y3_*: the default stays)
        if (i == 0 && !fuse_here && passes.size() > 1 && passes[i].mode == 1)
            nt_override = env_int("PIFFT_FIRST_NT", -1);
        const PassKernel* k = fuse_here ? fused
                                        : find_pass(s.prec, passes[i].R, passes[i].C, passes[i].mode,
                                                    nt_override >= 0 ? nt_override : passes[i].nts, 0, passes[i].vpt);
        if (!k) return fail("no pass kernel R=%d C=%d", passes[i].R, passes[i].C);
        const uint64_t nlines = local_transforms(s) * (s.m >> ilog2u((uint64_t)k->R));
        const uint64_t wgs = (nlines + (uint64_t)k->C - 1) / (uint64_t)k->C;
        if (wgs * (uint64_t)k->nt >= (1ull << 32)) return fail("transform too large for one launch (%llu work-items)",
                                                             (unsigned long long)(wgs * k->nt));
        out.push_back(k);
    }
    return 0;
}

// The plan of a shape: the local FFT as passes, then each rule in turn.
inline int choose_plan(const PlanShape& s, PlanChoice& ch) {
    PlanDraft d;
    if (plan_passes(s.m, s.prec, local_transforms(s), d.passes, may_fuse(s) ? s.lp : 0, true, !wil_ok(s))) return -1;
    const bool single = d.passes.size() == 1;
    if (wil_ok(s) && d.passes.size() > 1) worker_interleave(s, d);
    const PassChoice one = one_launch_pass(s);
    const bool one_launch = one_ok(s, single, one), small_wil = wil_single(s, single, one_launch);
    if (small_wil && one_launch) one_launch_plan(s, one, d);
    if ((d.wil || small_wil) && !d.fused_lines) fuse_all_workers(s, d);
    if (small_wil && !d.fused_lines) p16_two_pass_plan(s, d);
    if (bitrev_last_pass(s, d)) return -1;
    ch.wil = d.wil;
    ch.ilv = natural_store(s, d);
    ch.tree_tw = tree_table(s, d.wil);
    const PassKernel* fused = fused_tree_pass(s, d);
    ch.fused = !fused ? FUSED_NONE : d.fused_lines ? FUSED_ALL_WORKERS : FUSED_ONE_WORKER;
    return resolve_instances(s, d, fused, ch.passes);
}

}  // namespace pifft
