// The text of the pfslam_search_wide kernels (csrc/pfslam_search_wide.hip.inc, cut out by tests/test_search_wide_kernel_text.py into
// search_wide_kernel_text.inc behind the text of csrc/pfslam_search.hip.inc and csrc/pfslam_register.hip.inc it reuses) run on the CPU behind
// the SIMT shim of tests/search_emu.cpp: one std::thread per GPU thread of a workgroup that has barriers or shuffles, the workgroups of a
// launch one after the other, every buffer at the exact size pfslam_search_wide requests so that a sanitizer build sees any overrun.  The
// host's descent (batches of a quarter of a frontier buffer, depth first) is restated below, statement for statement.
// TEST INFRASTRUCTURE, not product code.
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
#include "register_defines.inc"   // PF_LIDAR_RANGE, PF_SVD_EPSILON: the lines of csrc/pfslam_hip.hip
#include "pf_math.h"
#include "kd_device.h"
namespace pf {                    // kd_device.h only declares these outside a device compilation
kd_rsrc_t kd_rsrc(const void *base) { return kd_rsrc_t{base}; }
uint4 kd_load_hot(kd_rsrc_t r, int idx) { return ((const uint4 *)r.base)[idx]; }
int kd_load_i32(kd_rsrc_t r, int idx) { return ((const int *)r.base)[idx]; }
int kd_load_i32_bytes(kd_rsrc_t r, int byte_offset) { return ((const int *)r.base)[byte_offset / 4]; }
uint4 kd_load_hot_at(kd_rsrc_t r, int base, int imm) { return ((const uint4 *)r.base)[(base + imm) / 16]; }
}
#include "search_wide_kernel_text.inc"

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
// usage: search_wide_emu IN.bin OUT.bin
//   IN  = int32 {n_nodes, planar, nb, trig, half_x, half_y, half_theta, stride, frontier nodes, 0}, float {cx, cy, ct, step_theta, max_dist, res, 0, 0},
//         hot[n] (16 B), z[n], parent[n], w[n], scan[nb]
//   OUT = the 12 floats of k_search_result's `out`, then the eight int64 of `stats`
int main(int argc, char **argv) {
    if (argc < 3) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const auto hd = rd<int>(f, 10);
    const auto fl = rd<float>(f, 8);
    const int n_nodes = hd[0], planar = hd[1], nb = hd[2], trig = hd[3], room = hd[8];
    const auto hot = rd<uint4>(f, n_nodes);
    const auto z = rd<float>(f, n_nodes);
    const auto parent = rd<int>(f, n_nodes);
    const auto w = rd<float>(f, n_nodes);
    const auto scan = rd<float>(f, nb);
    fclose(f);
    if (room < 4) return 7;
    const pf::KdView tree{hot.data(), z.data(), parent.data(), w.data(), planar};
    // what every entry point derives from its arguments: the library's own search_derive (csrc/pfslam_search.hip.inc), cut out with the kernels
    SearchParams p;
    SearchWhy why;
    const SearchRefusal no = search_derive(fl[5], nb, &fl[0], hd[4], hd[5], hd[6], hd[7], fl[3], fl[4], &p, &why);
    if (no != SEARCH_FITS) return no == SEARCH_QCAP ? 5 : 6;
    const long long nx = 2LL * p.hx + 1, ny = 2LL * p.hy + 1, na = 2LL * p.ht + 1;
    int top = 0;
    while (top < PF_WIDE_MAX_LEVEL && (1LL << top) < std::max(nx, ny)) top++;
    const long long n_top = na * (((nx - 1) >> top) + 1) * (((ny - 1) >> top) + 1);
    const size_t level = (size_t)p.cap + 2;
    // exact sizes: the sanitizer sees any overrun
    std::vector<uint16_t> field(level * (size_t)(top + 1), 0xdead);
    std::vector<int2> ends((size_t)na * nb, int2{7, 7});
    std::vector<int> nin((size_t)na, -7), nodes_buf((size_t)room * (size_t)(top + 1), -7), lb((size_t)room, -7);
    unsigned long long state[4];
    memset(state, 0xff, 24);
    unsigned long long *key = state;
    int *box = (int *)(state + 1);
    int *count = (int *)(state + 3);
    std::vector<float> out(PF_SEARCH_OUT, -1.0f);
    for (int a = 0; a < na; a++) {
        blockIdx.x = a;
        launch_block(256, [&] { k_search_ends(scan.data(), p, trig, ends.data(), nin.data(), box); });
    }
    const int cell_blocks = (p.cap + 255) / 256;
    for (int b = 0; b < cell_blocks; b++) { // (no barrier, no shuffle: the threads of a workgroup one after the other)
        blockIdx.x = b;
        for (int t = 0; t < 256; t++) {
            threadIdx.x = t;
            k_search_field(tree, p, box, field.data());
        }
    }
    for (int L = 1; L <= top; L++)
        for (int b = 0; b < cell_blocks; b++) {
            blockIdx.x = b;
            for (int t = 0; t < 256; t++) {
                threadIdx.x = t;
                k_wide_pyramid(box, p, (1 << (L - 1)) * p.stride, field.data() + level * (size_t)(L - 1), field.data() + level * (size_t)L);
            }
        }
    long long have[PF_WIDE_MAX_LEVEL + 1] = {0}, done[PF_WIDE_MAX_LEVEL + 1] = {0};
    long long bounded = 0, scored = 0, batches = 0;
    have[top] = n_top;
    for (int L = top;;) {
        if (done[L] >= have[L]) {
            if (L == top) break;
            L++;
            continue;
        }
        const int n = (int)std::min<long long>(have[L] - done[L], L ? std::max(room / 4, 1) : room);
        int *nodes = nodes_buf.data() + (size_t)room * (size_t)L;
        if (L == top) {
            for (int b = 0; b < (n + 255) / 256; b++) {
                blockIdx.x = b;
                for (int t = 0; t < 256; t++) {
                    threadIdx.x = t;
                    k_wide_top(p, L, done[L], n, nodes);
                }
            }
        } else {
            nodes += done[L];
        }
        done[L] += n;
        batches++;
        (L ? bounded : scored) += n;
        const uint16_t *fL = field.data() + level * (size_t)L;
        for (int b = 0; b < n; b++) {
            blockIdx.x = b;
            if (L) launch_block(64, [&] { k_wide_score<false>(nodes, ends.data(), nin.data(), box, field.data(), fL, p, lb.data(), key); });
            else launch_block(64, [&] { k_wide_score<true>(nodes, ends.data(), nin.data(), box, field.data(), fL, p, lb.data(), key); });
        }
        if (L == 0) continue;
        *count = 0;
        for (int b = 0; b < (n + 255) / 256; b++) {
            blockIdx.x = b;
            launch_block(256, [&] { k_wide_expand(nodes, lb.data(), n, L, p, key, nodes_buf.data() + (size_t)room * (size_t)(L - 1), count); });
        }
        const int kids = *count;
        if (kids < 0 || kids > 4 * n) return 8;
        if (kids) {
            L--;
            have[L] = kids;
            done[L] = 0;
        }
    }
    blockIdx.x = 0;
    threadIdx.x = 0;
    k_search_result(key, nin.data(), p, out.data());
    const SearchBox B = search_box(box, p);
    const long long stats[8] = {state[0] == ~0ull ? -1 : (long long)(state[0] & 0xffffffffull), nx * ny * na, bounded, scored, top, batches, (long long)B.W * B.H, 0};
    f = fopen(argv[2], "wb");
    fwrite(out.data(), 4, out.size(), f);
    fwrite(stats, 8, 8, f);
    fclose(f);
    return 0;
}
