// The text of the pfslam_search_cov kernels (csrc/pfslam_search_cov.hip.inc, cut out by tests/test_search_cov_kernel_text.py into
// search_cov_kernel_text.inc behind the unchanged text of pfslam_estimate's device functions, of csrc/pfslam_search.hip.inc and of
// csrc/pfslam_search_scan.hip.inc) run on the CPU behind the SIMT shim of tests/search_scan_emu.cpp: one std::thread per GPU thread of a
// workgroup that has barriers or shuffles, the workgroups one after the other.  The call is pfslam_search_scan_cov's: the scan form needs
// no tree.  Every buffer has exactly the size the entry point requests, so that a sanitizer build sees any overrun.  Stand-alone program,
// built with -fsanitize=address,undefined.  TEST INFRASTRUCTURE, not product code.
#include <algorithm>
#include <barrier>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>
#define __device__
#define __host__
#define __forceinline__ inline
#define __global__
#define __launch_bounds__(x)
#define __restrict__
#define __shared__ static
static float *g_dyn_lds;
#define HIP_DYNAMIC_SHARED(type, var) type *var = (type *)g_dyn_lds;
using std::min; using std::max;
struct uint4 { uint32_t x, y, z, w; };
struct float4 { float x, y, z, w; };
struct int2 { int x, y; };
struct float2 { float x, y; };
inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
inline float __uint_as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
inline float __int_as_float(int u) { float f; memcpy(&f, &u, 4); return f; }
inline int __float_as_int(float f) { int u; memcpy(&u, &f, 4); return u; }
inline uint32_t __float_as_uint(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
inline int __ffsll(long long v) { return __builtin_ffsll(v); }
#define __builtin_amdgcn_read_exec() (~0ull)
#define __builtin_amdgcn_ballot_w64(p) ((p) ? 1ull : 0ull)
#define __builtin_amdgcn_readfirstlane(v) (v)
struct Idx { int x; };
static thread_local Idx threadIdx;
static Idx blockIdx;
static std::barrier<> *g_block;
static std::vector<std::unique_ptr<std::barrier<>>> g_wave;
static unsigned long long g_sh[16][64];
inline void __syncthreads() { g_block->arrive_and_wait(); }
template <typename T> inline T __shfl_xor(T v, int off, int) {
    static_assert(sizeof(T) <= 8, "shuffle payload");
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    memcpy(&g_sh[w][l], &v, sizeof(T)); g_wave[w]->arrive_and_wait();
    T r; memcpy(&r, &g_sh[w][l ^ off], sizeof(T)); g_wave[w]->arrive_and_wait();
    return r;
}
inline void atomicAdd(unsigned long long *p, unsigned long long v) { __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
inline int atomicAdd(int *p, int v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
inline unsigned atomicCAS(unsigned *p, unsigned expect, unsigned want) {
    __atomic_compare_exchange_n(p, &expect, want, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
    return expect;
}
inline int atomicMax(int *p, int v) {
    int old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old < v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
}
inline unsigned long long atomicMin(unsigned long long *p, unsigned long long v) {
    unsigned long long old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old > v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
}
#include "register_defines.inc"   // PF_LIDAR_RANGE, PF_SVD_EPSILON, PF_SUM_TILE: the lines of csrc/pfslam_hip.hip
#include "pf_math.h"
#include "kd_device.h"
namespace pf {                    // kd_device.h only declares these outside a device compilation
kd_rsrc_t kd_rsrc(const void *base) { return kd_rsrc_t{base}; }
uint4 kd_load_hot(kd_rsrc_t r, int idx) { return ((const uint4 *)r.base)[idx]; }
int kd_load_i32(kd_rsrc_t r, int idx) { return ((const int *)r.base)[idx]; }
int kd_load_i32_bytes(kd_rsrc_t r, int byte_offset) { return ((const int *)r.base)[byte_offset / 4]; }
uint4 kd_load_hot_at(kd_rsrc_t r, int base, int imm) { return ((const uint4 *)r.base)[(base + imm) / 16]; }
}
#include "search_cov_kernel_text.inc"

template <typename K> void launch_block(int nthreads, K k) {
    std::barrier<> blk(nthreads); g_block = &blk;
    g_wave.clear();
    for (int w = 0; w < (nthreads + 63) / 64; w++) g_wave.emplace_back(new std::barrier<>(64));
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; t++) th.emplace_back([&, t] { threadIdx.x = t; k(); });
    for (auto &x : th) x.join();
}
template <typename T> static std::vector<T> rd(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}
static CovStep cov_step_of(long long n, long long nx, long long ny) { // (csrc/pfslam_search_cov.hip.inc, the host's part)
    const long long t = n / nx;
    return CovStep{(int)(n % nx), (int)(t % ny), (int)(t / ny)};
}
// usage: search_cov_emu IN.bin OUT.bin
//   IN  = int32 {nb, trig, half_x, half_y, half_theta, stride, 0, 0}, float {cx, cy, ct, step_theta, max_dist, res, rx, ry, rt, sigma, 0, 0},
//         ref[nb], scan[nb]
//   OUT = the 12 floats of k_search_result's `out`, int32 {box cells W, H, points, R}, the 16 floats of cov_out, then the score volume,
//         one int32 per candidate
int main(int argc, char **argv) {
    if (argc < 3) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const auto hd = rd<int>(f, 8);
    const auto fl = rd<float>(f, 12);
    const int nb = hd[0], trig = hd[1];
    const auto ref = rd<float>(f, nb);
    const auto scan = rd<float>(f, nb);
    fclose(f);
    // what every entry point derives from its arguments: the library's own search_derive (csrc/pfslam_search.hip.inc), cut out with the kernels
    SearchParams p;
    SearchWhy why;
    const SearchRefusal no = search_derive(fl[5], nb, &fl[0], hd[2], hd[3], hd[4], hd[5], fl[3], fl[4], &p, &why);
    if (no != SEARCH_FITS) return no == SEARCH_QCAP ? 5 : 6;
    const int R = (int)ceilf(pf::fdiv(fl[4], p.res)) + 2;
    const int nx = 2 * p.hx + 1, ny = 2 * p.hy + 1, na = 2 * p.ht + 1;
    const size_t cand = (size_t)nx * ny * na;
    // exact sizes: the sanitizer sees any overrun.  (The field as 32-bit words, as hipMalloc aligns it; its last word may be half used.)
    std::vector<unsigned> field_words(((size_t)p.cap + 2 + 1) / 2, 0xdeaddeadu);
    uint16_t *field = (uint16_t *)field_words.data();
    std::vector<int2> ends((size_t)na * nb, int2{7, 7});
    std::vector<float2> pts((size_t)nb, float2{-7.0f, -7.0f});
    std::vector<int> nin((size_t)na, -7), scores(cand, -7);
    unsigned long long state[3];
    memset(state, 0xff, sizeof(state));
    unsigned long long *key = state;
    int *box = (int *)(state + 1);
    int count = 0;
    std::vector<float> out(PF_SEARCH_OUT, -1.0f);
    for (int b = 0; b < (nb + 255) / 256; b++) {
        blockIdx.x = b;
        for (int t = 0; t < 256; t++) {
            threadIdx.x = t;
            k_scan_points(ref.data(), fl[6], fl[7], fl[8], nb, trig, pts.data(), &count);
        }
    }
    for (int a = 0; a < na; a++) {
        blockIdx.x = a;
        launch_block(256, [&] { k_search_ends(scan.data(), p, trig, ends.data(), nin.data(), box); });
    }
    for (int b = 0; b < (p.cap / 2 + 1 + 255) / 256; b++) {
        blockIdx.x = b;
        for (int t = 0; t < 256; t++) {
            threadIdx.x = t;
            k_scan_fill(p, box, field);
        }
    }
    for (int b = 0; b < (nb + 3) / 4; b++) {
        blockIdx.x = b;
        for (int t = 0; t < 256; t++) {
            threadIdx.x = t;
            k_scan_splat(pts.data(), nb, R, p, box, field);
        }
    }
    const int chunks = (nx * ny + 63) / 64;
    for (int b = 0; b < na * chunks; b++) {
        blockIdx.x = b;
        launch_block(64, [&] { k_search_score(ends.data(), nin.data(), box, field, p, chunks, scores.data(), key); });
    }
    blockIdx.x = 0;
    threadIdx.x = 0;
    k_search_result(key, nin.data(), p, out.data());
    // the reduction, as the entry point launches it
    CovParams q;
    q.hs = pf::fdiv(p.u * 1.442695f, (2.0f * fl[9]) * fl[9]);
    if (!std::isfinite(q.hs) || !(q.hs > 0.0f)) return 7;
    q.cand = (int)cand;
    q.wg = cov_step_of(PF_EST_WAVES * 64, nx, ny);
    q.wave = cov_step_of(64, nx, ny);
    const int nt = (int)((cand + PF_SUM_TILE - 1) / PF_SUM_TILE);
    std::vector<float> part((size_t)12 * nt, -1.0f), cov(PF_COV_OUT, -1.0f);
    if (nt == 1) {
        blockIdx.x = 0;
        launch_block(PF_EST_WAVES * 64, [&] { k_cov_small(scores.data(), key, p, q, part.data(), cov.data()); });
    } else {
        for (int t = 0; t < nt; t++) {
            blockIdx.x = t;
            launch_block(PF_EST_WAVES * 64, [&] { k_cov_moments(scores.data(), key, p, q, part.data(), nt); });
        }
        for (int t = 0; t < nt; t++) {
            blockIdx.x = t;
            launch_block(PF_EST_WAVES * 64, [&] { k_cov_centred(scores.data(), key, p, q, part.data(), part.data() + (size_t)5 * nt, nt); });
        }
        blockIdx.x = 0;
        launch_block(64, [&] { k_cov_final(part.data(), key, q, nt, cov.data()); });
    }
    const SearchBox B = search_box(box, p);
    const int dims[4] = {B.W, B.H, count, R};
    f = fopen(argv[2], "wb");
    fwrite(out.data(), 4, out.size(), f);
    fwrite(dims, 4, 4, f);
    fwrite(cov.data(), 4, cov.size(), f);
    fwrite(scores.data(), 4, scores.size(), f);
    fclose(f);
    return 0;
}
