// The text of the pfslam_cast kernels (csrc/pfslam_cast.hip.inc, cut out by tests/test_cast_kernel_text.py into cast_kernel_text.inc) run
// on the CPU behind the SIMT shim of tests/search_emu.cpp: one std::thread per GPU thread of a workgroup that has shuffles (k_cast_box,
// k_cast_count, k_cast_rays), the workgroups one after the other; the threads of k_cast_splat and k_cast_expand, which meet nowhere but in
// atomics, run one after the other too.  Every buffer has exactly the size the entry points request, so that a sanitizer build sees any
// overrun.  Stand-alone program, built with -fsanitize=address,undefined.  TEST INFRASTRUCTURE, not product code.
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
inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
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
inline unsigned long long atomicOr(unsigned long long *p, unsigned long long v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
inline int atomicMax(int *p, int v) {
    int old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old < v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
}
#include "pf_math.h"
#include "kd_device.h"
namespace pf {                    // kd_device.h only declares these outside a device compilation
kd_rsrc_t kd_rsrc(const void *base) { return kd_rsrc_t{base}; }
uint4 kd_load_hot(kd_rsrc_t r, int idx) { return ((const uint4 *)r.base)[idx]; }
int kd_load_i32(kd_rsrc_t r, int idx) { return ((const int *)r.base)[idx]; }
int kd_load_i32_bytes(kd_rsrc_t r, int byte_offset) { return ((const int *)r.base)[byte_offset / 4]; }
uint4 kd_load_hot_at(kd_rsrc_t r, int base, int imm) { return ((const uint4 *)r.base)[(base + imm) / 16]; }
}
#include "cast_kernel_text.inc"

// a grid of 256-thread workgroups whose waves shuffle: 256 threads, started once, take the workgroups one after the other
template <typename K> void launch_waves(int blocks, K k) {
    std::barrier<> blk(256); g_block = &blk;
    g_wave.clear();
    for (int w = 0; w < 4; w++) g_wave.emplace_back(new std::barrier<>(64));
    std::vector<std::thread> th;
    for (int t = 0; t < 256; t++)
        th.emplace_back([&, t] {
            threadIdx.x = t;
            for (int b = 0; b < blocks; b++) {
                if (t == 0) blockIdx.x = b;
                blk.arrive_and_wait();
                k();
                blk.arrive_and_wait();
            }
        });
    for (auto &x : th) x.join();
}
template <typename K> void launch_serial(int blocks, K k) {
    for (int b = 0; b < blocks; b++) {
        blockIdx.x = b;
        for (int t = 0; t < 256; t++) {
            threadIdx.x = t;
            k();
        }
    }
}
template <typename T> static std::vector<T> rd(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}
// usage: cast_emu IN.bin OUT.bin
//   IN  = int32 {nb, trig, m, nodes, inflate, skip_cells, 0, 0}, float {res_x, res_y, max_range, w_min, no_hit, 0, 0, 0},
//         nodes x {x, y, z, w}, m x {x, y, theta}
//   OUT = int64 stats[8] of pfslam_cast, m * nb ranges, m * nb x 2 cells; the same two arrays and an int32 hit count of the plain walk
//         (k_cast_rays<false>); then pfslam_map_raster's W * H bytes
int main(int argc, char **argv) {
    if (argc < 3) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const auto hd = rd<int>(f, 8);
    const auto fl = rd<float>(f, 8);
    const int nb = hd[0], m = hd[2], nn = hd[3];
    const auto nodes = rd<float>(f, (size_t)nn * 4);
    const auto poses = rd<float>(f, (size_t)m * 3);
    fclose(f);
    CastParams p;
    p.res_x = fl[0]; p.res_y = fl[1]; p.max_range = fl[2]; p.w_min = fl[3]; p.no_hit = fl[4];
    p.inflate = hd[4]; p.skip = hd[5]; p.nb = nb; p.trig = hd[1];
    // the map as the handle holds it: the hot records and the weights
    std::vector<uint4> hot((size_t)nn);
    std::vector<float> w((size_t)nn);
    for (int i = 0; i < nn; i++) {
        hot[i] = pf::pack_hot(nodes[4 * i], nodes[4 * i + 1], 0, -1, -1, true);
        w[i] = nodes[4 * i + 3];
    }
    // what cast_build_raster does (csrc/pfslam_cast.hip.inc); exact sizes: the sanitizer sees any overrun
    std::vector<int> st(PF_CAST_STATE, 0);
    for (int k = 0; k < 4; k++) st[k] = -1;
    const int nblk = (nn + 255) / 256;
    launch_waves(nblk, [&] { k_cast_box(hot.data(), w.data(), nn, p, st.data()); });
    CastBox B{0, 0, 0, 0, 0};
    std::vector<unsigned long long> tiles;
    if (st[0] >= 0) {
        const int minx = PF_CAST_BIAS - st[0], maxx = st[1] - PF_CAST_BIAS, miny = PF_CAST_BIAS - st[2], maxy = st[3] - PF_CAST_BIAS;
        B.x0 = minx - p.inflate; B.y0 = miny - p.inflate;
        B.W = maxx - minx + 1 + 2 * p.inflate; B.H = maxy - miny + 1 + 2 * p.inflate;
        B.TH = (B.H + 7) / 8;
        if ((long long)B.W * B.H > (1 << 28)) return 6;
        const size_t ntiles = (size_t)((B.W + 7) / 8) * B.TH;
        tiles.assign(ntiles, 0ull);
        launch_serial(nblk, [&] { k_cast_splat(hot.data(), w.data(), nn, p, B, tiles.data()); });
        launch_waves((int)((ntiles + 255) / 256), [&] { k_cast_count(tiles.data(), (int)ntiles, st.data()); });
    }
    const int rays = m * nb;
    std::vector<float> ranges((size_t)rays, -7.0f);
    std::vector<int> cells((size_t)2 * rays, -7);
    std::vector<float> ranges_plain((size_t)rays, -7.0f);
    std::vector<int> cells_plain((size_t)2 * rays, -7);
    launch_waves((rays + 255) / 256, [&] { k_cast_rays<false>(poses.data(), rays, p, B, tiles.data(), ranges_plain.data(), cells_plain.data(), st.data()); });
    const int hits_plain = st[6];
    st[6] = 0;
    launch_waves((rays + 255) / 256, [&] { k_cast_rays<true>(poses.data(), rays, p, B, tiles.data(), ranges.data(), cells.data(), st.data()); });
    const size_t ncell = (size_t)B.W * B.H;
    std::vector<uint8_t> occ(ncell, 7);
    if (ncell) launch_serial((int)((ncell + 255) / 256), [&] { k_cast_expand(tiles.data(), B, occ.data()); });
    const int64_t stats[8] = {rays, st[6], st[4], st[5], B.x0, B.y0, B.W, B.H};
    f = fopen(argv[2], "wb");
    fwrite(stats, 8, 8, f);
    fwrite(ranges.data(), 4, ranges.size(), f);
    fwrite(cells.data(), 4, cells.size(), f);
    fwrite(ranges_plain.data(), 4, ranges_plain.size(), f);
    fwrite(cells_plain.data(), 4, cells_plain.size(), f);
    fwrite(&hits_plain, 4, 1, f);
    fwrite(occ.data(), 1, occ.size(), f);
    fclose(f);
    return 0;
}
