// The text of the pfslam_cast_score kernel (csrc/pfslam_cast_score.hip.inc) and of the cast kernels it stands on (csrc/pfslam_cast.hip.inc),
// both cut out by tests/test_cast_score_kernel_text.py, run on the CPU behind the SIMT shim of tests/cast_emu.cpp: one std::thread per GPU
// thread of a workgroup, the workgroups one after the other.  Every buffer has exactly the size the entry point requests, so that a
// sanitizer build sees any overrun.  Stand-alone program, built with -fsanitize=address,undefined.  TEST INFRASTRUCTURE, not product code.
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
template <typename T> inline T __shfl_down(T v, int off, int) {   // (a lane whose source lies beyond the wave keeps its own value)
    static_assert(sizeof(T) <= 8, "shuffle payload");
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    memcpy(&g_sh[w][l], &v, sizeof(T)); g_wave[w]->arrive_and_wait();
    T r; memcpy(&r, &g_sh[w][l + off < 64 ? l + off : l], sizeof(T)); g_wave[w]->arrive_and_wait();
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
#include "cast_score_kernel_text.inc"

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
// usage: cast_score_emu IN.bin OUT.bin
//   IN  = int32 {nb, trig, m, nodes, inflate, skip_cells, soa, stride, count_miss, qcap, want_classes, 0},
//         float {res_x, res_y, max_range, w_min, tol, u, z_min, z_max}, nodes x {x, y, z, w},
//         the poses: m x {x, y, theta} (soa 0), or the block [x | y | theta] of 3 * stride floats (soa 1, stride >= m), nb scan ranges
//   OUT = for the jumping walk (k_cast_score<true>), then for the plain walk: int64 stats[8] of pfslam_cast_score, m x 8 rows,
//         m * nb class bytes (only with want_classes)
int main(int argc, char **argv) {
    if (argc < 3) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const auto hd = rd<int>(f, 12);
    const auto fl = rd<float>(f, 8);
    const int nb = hd[0], m = hd[2], nn = hd[3], soa = hd[6], stride = hd[7], want_classes = hd[10];
    if (soa && stride < m) return 3;
    const auto nodes = rd<float>(f, (size_t)nn * 4);
    const auto poses = rd<float>(f, soa ? (size_t)3 * stride : (size_t)3 * m);
    const auto scan = rd<float>(f, (size_t)nb);
    fclose(f);
    CastParams p;
    p.res_x = fl[0]; p.res_y = fl[1]; p.max_range = fl[2]; p.w_min = fl[3]; p.no_hit = 0.0f;
    p.inflate = hd[4]; p.skip = hd[5]; p.nb = nb; p.trig = hd[1];
    CastScoreParams s;
    s.tol = fl[4]; s.u = fl[5]; s.z_min = fl[6]; s.z_max = fl[7];
    s.qcap = hd[9]; s.count_miss = hd[8];
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
    // what pfslam_cast_score does: the pose list through (base, base + 1, base + 2) and stride 3, the particle block through its three
    // arrays and stride 1
    const float *px = poses.data(), *py = soa ? px + stride : px + 1, *pth = soa ? px + 2 * stride : px + 2;
    const int ps = soa ? 1 : 3;
    const size_t rays = (size_t)m * nb;
    const int blocks = (int)((rays + 255) / 256);
    f = fopen(argv[2], "wb");
    for (int jump = 1; jump >= 0; jump--) {
        std::vector<int> rows((size_t)m * PF_CAST_SCORE_ROW, 0); // (the entry point clears them)
        std::vector<uint8_t> classes(want_classes ? rays : 0, 7);
        uint8_t *cl = want_classes ? classes.data() : nullptr;
        if (jump) launch_waves(blocks, [&] { k_cast_score<true>(px, py, pth, ps, scan.data(), (int)rays, p, s, B, tiles.data(), rows.data(), cl); });
        else launch_waves(blocks, [&] { k_cast_score<false>(px, py, pth, ps, scan.data(), (int)rays, p, s, B, tiles.data(), rows.data(), cl); });
        // as the entry point does: the hits leave the rows for stats[1], the cost takes their place
        int64_t hits = 0;
        for (int r = 0; r < m; r++) {
            int *row = &rows[(size_t)r * PF_CAST_SCORE_ROW];
            hits += row[7];
            row[7] = row[5] + (s.count_miss ? s.qcap * row[4] : 0);
        }
        const int64_t stats[8] = {(int64_t)rays, hits, st[4], st[5], B.x0, B.y0, B.W, B.H};
        fwrite(stats, 8, 8, f);
        fwrite(rows.data(), 4, rows.size(), f);
        fwrite(classes.data(), 1, classes.size(), f);
    }
    fclose(f);
    return 0;
}
