// The SIMT shim of the kernel-text emulators (tests/*_emu.cpp): what a HIP kernel's text needs to compile and run on the CPU as a
// stand-alone program.  One std::thread per GPU thread, a std::barrier per workgroup for __syncthreads and one per wave for the shuffles,
// static LDS as function-local statics, dynamic LDS behind g_dyn_lds, the atomics as GCC builtins.  A lane is its own "wave" as far as
// votes go: read_exec / ballot / readfirstlane see that lane alone (the traversals only ask whether ANY lane is inside its guard band).
// What the kernels reuse is compiled from the product's own files, unchanged: csrc/pf_math.h and csrc/kd_device.h whole, behind an empty
// <hip/hip_runtime.h> and the kernel_defines.inc that tests/kernel_text.py writes.  kd_device.h needs clang (ext_vector_type).
// TEST INFRASTRUCTURE, not product code.
#pragma once
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
static float *g_dyn_lds;          // the launch's dynamic LDS: the emulator sets it
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

#include "kernel_defines.inc"     // the #define lines of csrc/pfslam_hip.hip that the test names
#include "pf_math.h"
#include "kd_device.h"
namespace pf {                    // kd_device.h only declares these outside a device compilation
kd_rsrc_t kd_rsrc(const void *base) { return kd_rsrc_t{base}; }
uint4 kd_load_hot(kd_rsrc_t r, int idx) { return ((const uint4 *)r.base)[idx]; }
int kd_load_i32(kd_rsrc_t r, int idx) { return ((const int *)r.base)[idx]; }
int kd_load_i32_bytes(kd_rsrc_t r, int byte_offset) { return ((const int *)r.base)[byte_offset / 4]; }
uint4 kd_load_hot_at(kd_rsrc_t r, int base, int imm) { return ((const uint4 *)r.base)[(base + imm) / 16]; }
}

// A grid whose threads meet at barriers or shuffles: `nthreads` host threads, started once, take the workgroups first .. first + blocks - 1
// one after the other (thread creation is what a sanitizer build spends its time on).  The waves' barriers expect 64 lanes each, so a
// launch whose last wave is partial AND shuffles would wait forever; no kernel does that.
template <typename K> void launch_threads(int blocks, int nthreads, K k, int first = 0) {
    std::barrier<> blk(nthreads); g_block = &blk;
    g_wave.clear();
    for (int w = 0; w < (nthreads + 63) / 64; w++) g_wave.emplace_back(new std::barrier<>(64));
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; t++)
        th.emplace_back([&, t] {
            threadIdx.x = t;
            for (int b = first; b < first + blocks; b++) {
                if (t == 0) blockIdx.x = b;
                blk.arrive_and_wait();
                k();
                blk.arrive_and_wait();
            }
        });
    for (auto &x : th) x.join();
}
// A grid whose threads meet nowhere (but in atomics): every thread of every workgroup one after the other, on the calling thread.
template <typename K> void launch_serial(int blocks, int nthreads, K k) {
    for (int b = 0; b < blocks; b++) {
        blockIdx.x = b;
        for (int t = 0; t < nthreads; t++) {
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
