// The text of the pfslam_register_batch kernel (csrc/pfslam_register_batch.hip.inc, cut out by tests/test_register_batch_kernel_text.py into
// register_batch_kernel_text.inc behind the text of csrc/pfslam_register.hip.inc it reuses) run on the CPU behind a small SIMT shim: one
// std::thread per GPU thread, a std::barrier per workgroup for __syncthreads and one per wave for __shfl_xor, static LDS as function-local
// statics, DYNAMIC LDS as a heap buffer of exactly the bytes the launch requests, every other buffer at its exact size so that a sanitizer
// build sees any overrun.  The workgroups of a launch run one after the other.  What the kernel reuses is compiled from the product's own
// files, unchanged: csrc/pf_math.h and csrc/kd_device.h whole (behind an empty <hip/hip_runtime.h> the test provides), wave_sum_canonical
// and the svd3 block of csrc/pfslam_stages.hip.inc as cut text.  kd_device.h needs clang (ext_vector_type).
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
static float *g_dyn_lds;          // the launch's dynamic LDS
#define HIP_DYNAMIC_SHARED(type, var) type *var = (type *)g_dyn_lds;
using std::min; using std::max;
struct uint4 { uint32_t x, y, z, w; };
struct float4 { float x, y, z, w; };
inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
inline float __uint_as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
inline float __int_as_float(int u) { float f; memcpy(&f, &u, 4); return f; }
inline int __float_as_int(float f) { int u; memcpy(&u, &f, 4); return u; }
inline uint32_t __float_as_uint(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
inline int __ffsll(long long v) { return __builtin_ffsll(v); }
// a lane on its own: it is the whole "wave" as far as votes go (the traversal only asks whether ANY lane is inside its guard band)
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
#include "register_batch_kernel_text.inc"

template <typename K> void launch_block(int nthreads, K k) {
    std::barrier<> blk(nthreads); g_block = &blk;
    g_wave.clear();
    for (int w = 0; w < nthreads / 64; w++) g_wave.emplace_back(new std::barrier<>(64));
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; t++) th.emplace_back([&, t] { threadIdx.x = t; k(); });
    for (auto &x : th) x.join();
}
template <typename T> static std::vector<T> rd(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}
// usage: register_batch_emu IN.bin OUT.bin
//   IN  = int32 {n_nodes, planar, nb, m, threads (256 or 1024), trig, 0, 0}, hot[n] (16 B), z[n], parent[n], w[n], scan[nb],
//         the eight 32-bit words of pfslam_register_opts, starts[m * 3]
//   OUT = the m x 12 floats of k_register_batch's `out`
int main(int argc, char **argv) {
    if (argc < 3) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const auto hd = rd<int>(f, 8);
    const int n = hd[0], planar = hd[1], nb = hd[2], m = hd[3], nt = hd[4], trig = hd[5];
    const auto hot = rd<uint4>(f, n);
    const auto z = rd<float>(f, n);
    const auto parent = rd<int>(f, n);
    const auto w = rd<float>(f, n);
    const auto scan = rd<float>(f, nb);
    RegOpts o;
    if (fread(&o, sizeof(o), 1, f) != 1) return 2;
    const auto starts = rd<float>(f, (size_t)m * 3);
    fclose(f);
    if (nt != 256 && nt != 1024) return 4;
    const pf::KdView tree{hot.data(), z.data(), parent.data(), w.data(), planar};
    std::vector<float> out((size_t)PF_REGB_OUT * m, -1.0f);   // exact sizes: the sanitizer sees any overrun
    const size_t lds = (size_t)nb * 8 * sizeof(float);       // what pfslam_register_batch requests
    for (int row = 0; row < m; row++) {
        g_dyn_lds = (float *)malloc(lds);                      // (a fresh, uninitialised buffer per workgroup, as on the device)
        blockIdx.x = row;
        auto go = [&](auto kern) { launch_block(nt, [&] { kern(scan.data(), nb, starts.data(), tree, o, trig, out.data()); }); };
        if (planar && nt == 256) go(k_register_batch<true, 256>);
        else if (planar) go(k_register_batch<true, 1024>);
        else if (nt == 256) go(k_register_batch<false, 256>);
        else go(k_register_batch<false, 1024>);
        free(g_dyn_lds);
    }
    f = fopen(argv[2], "wb");
    fwrite(out.data(), 4, out.size(), f);
    fclose(f);
    return 0;
}
