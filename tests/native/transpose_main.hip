// The matrix plans' transpose (csrc/pifft_matrix.h) on the host: a launch of
// `workgroups` workgroups is emulated phase by phase -- every thread's load
// phase, then every thread's store phase, tile after tile of each workgroup's
// grid-stride loop -- over a plain array standing in for LDS and buffers of
// exactly the sizes a plan passes, so a host sanitizer sees every index the
// kernel would form.
//
//   transpose <rows> <cols> <batch> <32|64> <workgroups>
//
// in[e] = (e + 1, -(e + 1)).  After each tile every output value that is new
// must be the one the transpose puts there and is then marked taken, so a
// later store to it shows; a tile's threads store exactly t_r * t_c values, so
// t_r * t_c new ones mean each was stored once.  The output and the LDS array
// carry 8 guard values on either side.
// Prints {"tiles": tiles of the launch, "unwritten": output values never
// stored, "bad": wrong, repeated or missing stores, "guard": guard values
// overwritten}.
#include "../../cs87project-msolano2_amd/csrc/pifft_matrix.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace pifft;

static void* alloc16(size_t bytes) {  // exactly `bytes`, 16-B aligned
    void* p = nullptr;
    if (posix_memalign(&p, 16, bytes ? bytes : 1)) exit(3);
    return p;
}

template <typename T>
int run(uint64_t rows, uint64_t cols, uint32_t batch, uint64_t wgs) {
    typedef typename tr_vec<T>::type V;
    const uint64_t total = (uint64_t)batch * rows * cols, G = 8;
    const uint32_t nlds = TR_PLANE * tr_sub<T>();
    cx<T>* in = (cx<T>*)alloc16(total * sizeof(cx<T>));
    cx<T>* out0 = (cx<T>*)alloc16((total + 2 * G) * sizeof(cx<T>));
    V* lds0 = (V*)alloc16((nlds + 2 * G) * sizeof(V));
    cx<T>* out = out0 + G;
    V* lds = lds0 + G;
    const cx<T> unset{(T)-1, (T)-1}, taken{(T)-2, (T)-2};
    for (uint64_t e = 0; e < total; e++) in[e] = {(T)(e + 1), -(T)(e + 1)};
    for (uint64_t e = 0; e < total + 2 * G; e++) out0[e] = unset;
    memset(lds0, 0x5a, (nlds + 2 * G) * sizeof(V));
    TransposeArgs a = transpose_args<T>(rows, cols, batch);
    a.in = in;
    a.out = out;
    const uint64_t per_tile = 1ull << (a.log_tr + a.log_tc);
    uint64_t bad = 0;
    for (uint64_t wg = 0; wg < wgs; wg++)
        for (uint64_t tile = wg; tile < a.tiles; tile += wgs) {
            memset(lds, 0x5a, nlds * sizeof(V));  // (a slot read but not written this tile: a wrong value)
            for (uint32_t tid = 0; tid < 256; tid++) tr_load<T>(a, tile, tid, lds);
            for (uint32_t tid = 0; tid < 256; tid++) tr_store<T>(a, tile, tid, lds);
            uint64_t fresh = 0;
            for (uint64_t e = 0; e < total; e++) {
                cx<T>& v = out[e];
                if ((v.re == unset.re && v.im == unset.im) || (v.re == taken.re && v.im == taken.im)) continue;
                const uint64_t b = e / (rows * cols), c = e / rows % cols, r = e % rows;  // out[b][c][r]
                const cx<T> want = in[(b * rows + r) * cols + c];
                bad += !(v.re == want.re && v.im == want.im);
                fresh++;
                v = taken;
            }
            bad += fresh != per_tile;
        }
    uint64_t unwritten = 0, guard = 0;
    for (uint64_t e = 0; e < total; e++) unwritten += !(out[e].re == taken.re && out[e].im == taken.im);
    for (uint64_t i = 0; i < G; i++) {
        guard += !(out0[i].re == unset.re && out0[i].im == unset.im);
        guard += !(out[total + i].re == unset.re && out[total + i].im == unset.im);
    }
    const unsigned char* lb = (const unsigned char*)lds0;
    for (size_t i = 0; i < G * sizeof(V); i++)
        guard += (lb[i] != 0x5a) + (lb[(G + nlds) * sizeof(V) + i] != 0x5a);
    printf("{\"tiles\": %llu, \"unwritten\": %llu, \"bad\": %llu, \"guard\": %llu}\n", (unsigned long long)a.tiles,
           (unsigned long long)unwritten, (unsigned long long)bad, (unsigned long long)guard);
    free(in);
    free(out0);
    free(lds0);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 6) return 2;
    const uint64_t rows = strtoull(argv[1], nullptr, 10), cols = strtoull(argv[2], nullptr, 10);
    const uint32_t batch = (uint32_t)atoi(argv[3]);
    const int prec = atoi(argv[4]);
    const uint64_t wgs = strtoull(argv[5], nullptr, 10);
    auto pow2 = [](uint64_t v) { return v >= 2 && !(v & (v - 1)); };
    if (!pow2(rows) || !pow2(cols) || rows > 8192 || cols > 8192 || batch < 1 || batch > 8 || wgs < 1) return 2;
    if ((uint64_t)batch * rows * cols > (1ull << 20)) return 2;
    return prec == 64 ? run<double>(rows, cols, batch, wgs) : run<float>(rows, cols, batch, wgs);
}
