// The text of the pfslam_estimate kernels (csrc/pfslam_stages.hip.inc, cut out by tests/test_estimate_kernel_text.py into estimate_kernel_text.inc)
// run on the CPU: one std::thread per GPU thread, a std::barrier per workgroup for __syncthreads and one per wave for __shfl_xor, LDS as a
// function-local static, the buffers at their exact sizes so that a sanitizer build sees any overrun.  TEST INFRASTRUCTURE, not product code.
#include <algorithm>
#include <barrier>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>
#define __device__
#define __forceinline__ inline
#define __global__
#define __launch_bounds__(x)
#define __restrict__
#define __shared__ static
#define PF_SUM_TILE 4096
using std::min; using std::max;
namespace pf { inline float fdiv(float a, float b) { return a / b; } }
struct Idx { int x; };
static thread_local Idx threadIdx;
static Idx blockIdx;
static std::barrier<> *g_block;
static std::vector<std::unique_ptr<std::barrier<>>> g_wave;
static float g_sh[16][64];
inline void __syncthreads() { g_block->arrive_and_wait(); }
inline float __shfl_xor(float v, int off, int) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    g_sh[w][l] = v; g_wave[w]->arrive_and_wait();
    const float r = g_sh[w][l ^ off]; g_wave[w]->arrive_and_wait();
    return r;
}
#include "estimate_kernel_text.inc"
template <typename K> void launch(int nblocks, int nthreads, K k) {
    for (int b = 0; b < nblocks; b++) {
        blockIdx.x = b;
        std::barrier<> blk(nthreads); g_block = &blk;
        g_wave.clear();
        for (int w = 0; w < nthreads / 64; w++) g_wave.emplace_back(new std::barrier<>(64));
        std::vector<std::thread> th;
        for (int t = 0; t < nthreads; t++) th.emplace_back([&, t] { threadIdx.x = t; k(); });
        for (auto &x : th) x.join();
    }
}
// usage: estimate_emu GN WORLD IN.bin OUT.bin   IN = gw[world * stride] then gpose[world][3][stride] as float32, OUT = the 16 floats
int main(int argc, char **argv) {
    const int gn = atoi(argv[1]), world = atoi(argv[2]);
    const int stride = (gn + world - 1) / world;
    std::vector<float> gw((size_t)world * stride), gpose((size_t)world * 3 * stride);   // exact sizes: the sanitizer sees any overrun
    FILE *f = fopen(argv[3], "rb");
    if (fread(gw.data(), 4, gw.size(), f) != gw.size() || fread(gpose.data(), 4, gpose.size(), f) != gpose.size()) return 2;
    fclose(f);
    const int nt = (gn + PF_SUM_TILE - 1) / PF_SUM_TILE;
    std::vector<float> scratch((size_t)11 * nt + 16, -1.0f);
    float *part = scratch.data(), *res = part + (size_t)11 * nt;
    if (nt == 1) {
        launch(1, 384, [&] { k_estimate_small(gw.data(), gpose.data(), stride, gn, part, res); });
    } else {
        launch(nt, 384, [&] { k_estimate_moments(gw.data(), gpose.data(), stride, gn, part, nt); });
        launch(nt, 384, [&] { k_estimate_centred(gw.data(), gpose.data(), stride, gn, part, part + (size_t)5 * nt, nt); });
        launch(1, 64, [&] { k_estimate_final(part, nt, gn, res); });
    }
    f = fopen(argv[4], "wb"); fwrite(res, 4, 16, f); fclose(f);
    return 0;
}
