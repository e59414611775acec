// pfslam_stages.hip.inc -- measurement reduce + weights, ICP, point-cloud map update, resample,
// 2-D grid path and the whole step.  Included by pfslam_hip.hip (same translation unit).
// tests/kernel_text.py cuts the text between each pair of ...-KERNEL-TEXT marks out; the kernel-text tests run it on the CPU.

// ------------------------------------------------------------------------------------------
// wave / block helpers (wave64)
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ long long wave_max_i64(long long v)
{
    for (int off = 32; off >= 1; off >>= 1) {
        long long o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ float wave_max_f32(float v)
{
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}
// Canonical reduction order standing in for thrust::reduce (whose order is unspecified):
// lane l accumulates elements l, l+64, ... in ascending order, then an xor butterfly
// 32,16,...,1.  Every lane returns the same bits.  Used for n <= 4096 (one tile).
// WAVE-SUM-KERNEL-TEXT-BEGIN
template <typename F>
__device__ __forceinline__ float wave_sum_canonical(int n, F elem)
{
    const int lane = threadIdx.x & 63;
    float acc = 0.0f;
    for (int i = lane; i < n; i += 64) acc = acc + elem(i);
    for (int off = 32; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off, 64);
    return acc;
}

// WAVE-SUM-KERNEL-TEXT-END
// float <-> order-preserving signed int (so that int64 MAX all-reduces implement min/max/argmax)
__device__ __forceinline__ int f32_to_ordered(float f)
{
    int s = __float_as_int(f);
    return s ^ ((s >> 31) & 0x7fffffff);
}
__device__ __forceinline__ float ordered_to_f32(int s) { return __int_as_float(s ^ ((s >> 31) & 0x7fffffff)); }

// ------------------------------------------------------------------------------------------
// A6: thrust::minmax_element (first occurrence) as one packed max-reduction
//     key = ordered(fit) << 32 | (0xFFFFFFFF - global index): max key == max fit, lowest index
// ------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ int fit_ordered(T v);
template <>
__device__ __forceinline__ int fit_ordered<float>(float v) { return f32_to_ordered(v); }
template <>
__device__ __forceinline__ int fit_ordered<int>(int v) { return v; }
template <typename T>
__device__ __forceinline__ int fit_neg_ordered(T v);
template <>
__device__ __forceinline__ int fit_neg_ordered<float>(float v) { return f32_to_ordered(-v); }
template <>
__device__ __forceinline__ int fit_neg_ordered<int>(int v) { return -v; }

template <typename T>
__global__ __launch_bounds__(256) void k_minmax(const T *__restrict__ fit, int n, int goff, long long *__restrict__ stats)
{
    long long kmax = LLONG_MIN, kmin = LLONG_MIN;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const T v = fit[i];
        const long long a = ((long long)fit_ordered<T>(v) << 32) | (long long)(0xFFFFFFFFu - (uint32_t)(goff + i));
        const long long b = ((long long)fit_neg_ordered<T>(v) << 32);
        kmax = a > kmax ? a : kmax;
        kmin = b > kmin ? b : kmin;
    }
    kmax = wave_max_i64(kmax);
    kmin = wave_max_i64(kmin);
    __shared__ long long smax[4], smin[4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        smax[wave] = kmax;
        smin[wave] = kmin;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; k++) {
            kmax = smax[k] > kmax ? smax[k] : kmax;
            kmin = smin[k] > kmin ? smin[k] : kmin;
        }
        atomicMax(&stats[0], kmax);
        atomicMax(&stats[1], kmin);
    }
}

__global__ void k_stats_reset(long long *stats)
{
    if (threadIdx.x < 8) stats[threadIdx.x] = threadIdx.x < 2 ? LLONG_MIN : 0;
}

// k_reduce_partials + k_minmax<float> in one launch (the frame loop's chain is bounded by its number of dependent
// launches): same chunk-order sum per slot, then the packed keys of the block go into stats with two atomics.
__global__ __launch_bounds__(256) void k_reduce_partials_minmax(const float *__restrict__ partial, int n, int chunks,
                                                                const int *__restrict__ order, float *__restrict__ fit, int goff,
                                                                long long *__restrict__ stats, const float *__restrict__ x,
                                                                const float *__restrict__ y, const float *__restrict__ th, int p16)
{
    // At most PF_REDUCE4_WGS workgroups take the slots in a grid-stride loop: one workgroup per 256 slots ended with three atomics (and, sharded,
    // a fence) on ONE cache line each -- 391 workgroups at 100 k particles, applied one after the other, and the launch behind this one
    // waited for them (the round-5 frame's k_reduce_groups had the same tail: 9 us, tools/experiments/r05/README.md).
    long long kmax = LLONG_MIN, kmin = LLONG_MIN;
    for (int slot = blockIdx.x * 256 + threadIdx.x; slot < n; slot += gridDim.x * 256) {
        float a = 0.0f;
        int c = 0;
        if (p16) { // 16-bit integer partials (k_score_kd_cells, out_mode 3): integer sums, exact in any order
            const short *p = (const short *)partial;
            int ia = 0;
            for (; c + 32 <= chunks; c += 32) {
                short v[32];
#pragma unroll
                for (int k = 0; k < 32; k++) v[k] = p[(size_t)(c + k) * n + slot];
#pragma unroll
                for (int k = 0; k < 32; k++) ia += v[k];
            }
            for (; c < chunks; c++) ia += p[(size_t)c * n + slot];
            a = (float)ia; // |sum| <= n_beams x largest |weight| <= 2^24 (upload_tree)
        }
        for (; c + 64 <= chunks; c += 64) {
            float v[64];
#pragma unroll
            for (int k = 0; k < 64; k++) v[k] = partial[(size_t)(c + k) * n + slot];
#pragma unroll
            for (int k = 0; k < 64; k++) a += v[k];
        }
        for (; c + 16 <= chunks; c += 16) {
            float v[16];
#pragma unroll
            for (int k = 0; k < 16; k++) v[k] = partial[(size_t)(c + k) * n + slot];
#pragma unroll
            for (int k = 0; k < 16; k++) a += v[k];
        }
        for (; c < chunks; c++) a += partial[(size_t)c * n + slot];
        const int i = order ? order[slot] : slot;
        fit[i] = a;
        const long long k1 = ((long long)f32_to_ordered(a) << 32) | (long long)(0xFFFFFFFFu - (uint32_t)(goff + i));
        const long long k2 = ((long long)f32_to_ordered(-a) << 32);
        kmax = k1 > kmax ? k1 : kmax;
        kmin = k2 > kmin ? k2 : kmin;
    }
    kmax = wave_max_i64(kmax);
    kmin = wave_max_i64(kmin);
    __shared__ long long smax[4], smin[4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        smax[wave] = kmax;
        smin[wave] = kmin;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; k++) {
            kmax = smax[k] > kmax ? smax[k] : kmax;
            kmin = smin[k] > kmin ? smin[k] : kmin;
        }
        atomicMax(&stats[0], kmax);
        atomicMax(&stats[1], kmin);
    }
}

// The same reduce for few particles and MANY beam chunks (below ~2000 particles a wave scores one beam, so there are 1081
// partials per particle): 16 threads share a particle's chunks instead of one thread walking all of them (24 us -> a few at
// 1000 particles).  Any summation order is exact here: beam-chunk partials exist only for integer map weights (score_chunks).
__global__ __launch_bounds__(1024) void k_reduce_partials_minmax_wide(const float *__restrict__ partial, int n, int chunks,
                                                                      const int *__restrict__ order, float *__restrict__ fit,
                                                                      long long *__restrict__ stats)
{
    __shared__ float s_part[16][64];
    const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6, slot = blockIdx.x * 64 + lane;
    const int per = (chunks + 15) / 16, c0 = seg * per, c1 = min(chunks, c0 + per);
    float a = 0.0f;
    if (slot < n) {
        int c = c0;
        for (; c + 16 <= c1; c += 16) {
            float v[16];
#pragma unroll
            for (int k = 0; k < 16; k++) v[k] = partial[(size_t)(c + k) * n + slot];
#pragma unroll
            for (int k = 0; k < 16; k++) a += v[k];
        }
        for (; c < c1; c++) a += partial[(size_t)c * n + slot];
    }
    s_part[seg][lane] = a;
    __syncthreads();
    if (seg != 0) return;
    long long kmax = LLONG_MIN, kmin = LLONG_MIN;
    if (slot < n) {
        for (int k = 1; k < 16; k++) a += s_part[k][lane];
        const int i = order ? order[slot] : slot;
        fit[i] = a;
        kmax = ((long long)f32_to_ordered(a) << 32) | (long long)(0xFFFFFFFFu - (uint32_t)i);
        kmin = ((long long)f32_to_ordered(-a) << 32);
    }
    kmax = wave_max_i64(kmax);
    kmin = wave_max_i64(kmin);
    if (lane == 0) {
        atomicMax(&stats[0], kmax);
        atomicMax(&stats[1], kmin);
    }
}

// kernUpdateWeights (kernel.cu:287-304) + the read-back of kernel.cu:1341 (H11) + best pose.
// `int min` parameter of the reference truncates the float minimum toward zero (A6/H8).
template <typename T>
__global__ __launch_bounds__(256) void k_weights_apply(float *__restrict__ w, float *__restrict__ wm,
                                                       const T *__restrict__ fit, int n, int goff, int mirror_count,
                                                       const long long *__restrict__ stats,
                                                       const float *__restrict__ x, const float *__restrict__ y,
                                                       const float *__restrict__ th, float *__restrict__ start)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const long long kmax = stats[0], kmin = stats[1];
    if (i == 0 && start) { // best particle's pose (zero on ranks that do not own it: merged with a SUM)
        const uint32_t best = 0xFFFFFFFFu - (uint32_t)(kmax & 0xFFFFFFFFll);
        const int lb = (int)best - goff;
        const bool mine = lb >= 0 && lb < n;
        start[0] = mine ? x[lb] : 0.0f;
        start[1] = mine ? y[lb] : 0.0f;
        start[2] = mine ? th[lb] : 0.0f;
        start[3] = 0.0f;
    }
    if (i >= n) return;
    float wi = w[i];
    if (sizeof(T) == 4 && std::is_same<T, float>::value) {
        const float fmax = ordered_to_f32((int)(kmax >> 32));
        const float fmin = -ordered_to_f32((int)(kmin >> 32));
        const float rng = fmax - fmin;
        if (rng > 0.0f) {
            const float c = pf::fdiv(1.0f, rng);
            const int mint = (int)fmin;
            wi = wi * ((float)fit[i] - (float)mint) * c;
        }
    } else {
        const int imax = (int)(kmax >> 32), imin = -(int)(kmin >> 32);
        const int rng = imax - imin;
        if (rng > 0) {
            const float c = pf::fdiv(1.0f, (float)rng);
            wi = wi * ((float)fit[i] - (float)imin) * c;
        }
    }
    w[i] = wi;
    if (goff + i < mirror_count) wm[i] = wi;
}

// ---- sharded measurement merge (multi-GPU; no reference counterpart) ---------------------------------------------
// A rank's record for the ONE small all-gather on the frame's critical chain is what its reduce leaves anyway: the packed
// {max key, negated-min key} (16 bytes; the max key's low word carries the GLOBAL index of the shard's best particle).  Every rank
// derives the global min / max / first argmax from the `world` gathered records by itself, and reads the best particle's pose out
// of the pose blocks of every rank, which were gathered under the scan-match kernel (buffer 17) -- no pack kernel between the
// reduce and the collective.  gkeys == nullptr: an unsharded job, the keys are the handle's own.
__device__ __forceinline__ void frame_keys(const long long *__restrict__ stats, const long long *__restrict__ gkeys, int world,
                                           long long &kmax, long long &kmin)
{
    if (!gkeys) {
        kmax = stats[0];
        kmin = stats[1];
        return;
    }
    kmax = LLONG_MIN;
    kmin = LLONG_MIN;
    for (int r = 0; r < world; r++) { // wave-uniform loads of <= a few hundred bytes
        const long long a = gkeys[2 * r], b = gkeys[2 * r + 1];
        kmax = a > kmax ? a : kmax;
        kmin = b > kmin ? b : kmin;
    }
}

// kernUpdateWeights (kernel.cu:297-304) on a shard, with the global min / max taken from the gathered keys.  Block 0 also leaves the
// merged keys for the frame's header (mkeys) and, when asked (the staged frame of maps the cell rows do not cover), the best particle's
// pose and the frame's pose = best + ICP increment (kernel.cu:1081-1092).
__global__ __launch_bounds__(256) void k_weights_apply_sharded(float *__restrict__ w, float *__restrict__ wm,
                                                               const float *__restrict__ fit, int n, int goff, int mirror_count,
                                                               const long long *__restrict__ stats_local, const long long *__restrict__ gkeys, int world,
                                                               const float *__restrict__ gpose, int stride,
                                                               long long *__restrict__ mkeys, float *__restrict__ start,
                                                               const float *__restrict__ icp_dbg, float *__restrict__ pose,
                                                               unsigned long long *__restrict__ probe = nullptr)
{
    pf_stamp(probe);
    long long kmax, kmin;
    frame_keys(stats_local, gkeys, world, kmax, kmin);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) {
        mkeys[0] = kmax;
        mkeys[1] = kmin;
        if (start) {
            const uint32_t best = 0xFFFFFFFFu - (uint32_t)(kmax & 0xFFFFFFFFll);
            const uint32_t r = best / (uint32_t)stride, j = best - r * (uint32_t)stride;
            const bool ok = r < (uint32_t)world;
            const float *blk = gpose + (size_t)(ok ? r : 0u) * 3 * stride;
            const float bx = ok ? blk[j] : 0.0f, by = ok ? blk[stride + j] : 0.0f, bt = ok ? blk[2 * stride + j] : 0.0f;
            start[0] = bx;
            start[1] = by;
            start[2] = bt;
            start[3] = 0.0f;
            if (icp_dbg) {
                pose[0] = bx + icp_dbg[24];
                pose[1] = by + icp_dbg[25];
                pose[2] = bt + icp_dbg[27];
                pose[3] = 0.0f;
            }
        }
    }
    if (i >= n) return;
    float wi = w[i];
    const float fmax = ordered_to_f32((int)(kmax >> 32));
    const float fmin = -ordered_to_f32((int)(kmin >> 32));
    const float rng = fmax - fmin;
    if (rng > 0.0f) {
        const float c = pf::fdiv(1.0f, rng);
        const int mint = (int)fmin;
        wi = wi * (fit[i] - (float)mint) * c;
    }
    w[i] = wi;
    if (goff + i < mirror_count) wm[i] = wi;
}

// Largest |heading| over EVERY rank's particles, from the gathered pose blocks: what the host's choice of the scan-match kernel's
// instantiation (sincos_sum_spec<GUARD>) needs of a job whose resample imports particles from the other shards.  The launch sits on
// the particle stream right behind the pose blocks' all-gather, under the scan-match kernel; as the first launch behind the collective
// it also says so (flag: the gathered blocks are there -- a kernel boundary has made them visible).  out: ring of 4 by ticket.
__global__ __launch_bounds__(256) void k_theta_gmax(const float *__restrict__ gpose, int world, int stride, float *__restrict__ out4, int seq,
                                                    int *__restrict__ flag_word)
{
    if (flag_word && blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(flag_word, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    __shared__ float red[4];
    float tm = 0.0f;
    const int total = world * stride;
    for (int g = blockIdx.x * 256 + threadIdx.x; g < total; g += gridDim.x * 256) {
        const int r = g / stride, j = g - r * stride;
        const float t = gpose[(size_t)r * 3 * stride + 2 * (size_t)stride + j]; // (the pad of a short last shard is zero)
        tm = fmaxf(tm, t == t ? fabsf(t) : INFINITY);
    }
    tm = wave_max_f32(tm);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = tm;
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMax((int *)&out4[seq & 3], __float_as_int(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])))); // non-negative floats order like their bits
        if (blockIdx.x == 0) out4[(seq + 1) & 3] = 0.0f; // the next ticket's maximum starts over (its launch is behind this one on the stream)
    }
}

// ------------------------------------------------------------------------------------------
// A9: 3x3 SVD of McAdams et al. with the operation order of the reference's svd3.h:52-401
// ------------------------------------------------------------------------------------------
// SVD3-KERNEL-TEXT-BEGIN
namespace pf {
struct Sym3 { float s11, s21, s22, s31, s32, s33; };

PF_HD float rsqrt1(float x) // svd3.h:52-60
{
    float xhalf = 0.5f * x;
    union { float f; int i; } u;
    u.f = x;
    u.i = 0x5f37599e - (u.i >> 1);
    x = u.f;
    x = x * (1.5f - xhalf * x * x);
    x = x * (1.5f - xhalf * x * x);
    return x;
}
PF_HD void cswap(bool c, float &X, float &Y) { float Z = X; X = c ? Y : X; Y = c ? Z : Y; }
PF_HD void cnswap(bool c, float &X, float &Y) { float Z = -X; X = c ? Y : X; Y = c ? Z : Y; }

PF_HD void jacobi_conj(int x, int y, int z, Sym3 &S, float *qV) // svd3.h:145-216
{
    float ch = 2 * (S.s11 - S.s22), sh = S.s21;
    const bool b = 5.828427124 * sh * sh < ch * ch;
    const float wq = rsqrtf_spec(ch * ch + sh * sh);
    ch = b ? wq * ch : (float)0.923879532;
    sh = b ? wq * sh : (float)0.3826834323;
    const float scale = ch * ch + sh * sh;
    const float a = fdiv(ch * ch - sh * sh, scale);
    const float bb = fdiv(2 * sh * ch, scale);
    const float o11 = S.s11, o21 = S.s21, o22 = S.s22, o31 = S.s31, o32 = S.s32, o33 = S.s33;
    const float n11 = a * (a * o11 + bb * o21) + bb * (a * o21 + bb * o22);
    const float n21 = a * (-bb * o11 + a * o21) + bb * (-bb * o21 + a * o22);
    const float n22 = -bb * (-bb * o11 + a * o21) + a * (-bb * o21 + a * o22);
    const float n31 = a * o31 + bb * o32;
    const float n32 = -bb * o31 + a * o32;
    const float n33 = o33;
    float tmp[3] = {qV[0] * sh, qV[1] * sh, qV[2] * sh};
    sh *= qV[3];
    qV[0] *= ch; qV[1] *= ch; qV[2] *= ch; qV[3] *= ch;
    qV[z] += sh;
    qV[3] -= tmp[z];
    qV[x] += tmp[y];
    qV[y] -= tmp[x];
    // cyclic re-arrangement for the next pair
    S.s11 = n22;
    S.s21 = n32; S.s22 = n33;
    S.s31 = n21; S.s32 = n31; S.s33 = n11;
}

PF_HD void qr_givens(float a1, float a2, float &ch, float &sh) // svd3.h:277-292
{
    const float eps = PF_SVD_EPSILON;
    const float ssq = a1 * a1 + a2 * a2;
    const float rho = ssq * rsqrt1(ssq);
    sh = rho > eps ? a2 : 0;
    ch = fabsf(a1) + fmaxf(rho, eps);
    cswap(a1 < 0, sh, ch);
    const float wq = rsqrtf_spec(ch * ch + sh * sh);
    ch *= wq;
    sh *= wq;
}

// a, u, s, v: row-major 3x3 (a11..a33), exactly svd(...) of svd3.h:354-401
PF_HD void svd3(const float *A, float *U, float *Sg, float *V)
{
    const float a11 = A[0], a12 = A[1], a13 = A[2], a21 = A[3], a22 = A[4], a23 = A[5], a31 = A[6], a32 = A[7], a33 = A[8];
    Sym3 S;
    S.s11 = a11 * a11 + a21 * a21 + a31 * a31;
    S.s21 = a12 * a11 + a22 * a21 + a32 * a31;
    S.s22 = a12 * a12 + a22 * a22 + a32 * a32;
    S.s31 = a13 * a11 + a23 * a21 + a33 * a31;
    S.s32 = a13 * a12 + a23 * a22 + a33 * a32;
    S.s33 = a13 * a13 + a23 * a23 + a33 * a33;
    float qV[4] = {0, 0, 0, 1};
    for (int it = 0; it < 4; it++) {
        jacobi_conj(0, 1, 2, S, qV);
        jacobi_conj(1, 2, 0, S, qV);
        jacobi_conj(2, 0, 1, S, qV);
    }
    const float w = qV[3], x = qV[0], y = qV[1], z = qV[2];
    const float qxx = x * x, qyy = y * y, qzz = z * z, qxz = x * z, qxy = x * y, qyz = y * z;
    const float qwx = w * x, qwy = w * y, qwz = w * z;
    float v11 = 1 - 2 * (qyy + qzz), v12 = 2 * (qxy - qwz), v13 = 2 * (qxz + qwy);
    float v21 = 2 * (qxy + qwz), v22 = 1 - 2 * (qxx + qzz), v23 = 2 * (qyz - qwx);
    float v31 = 2 * (qxz - qwy), v32 = 2 * (qyz + qwx), v33 = 1 - 2 * (qxx + qyy);
    float b11 = a11 * v11 + a12 * v21 + a13 * v31, b12 = a11 * v12 + a12 * v22 + a13 * v32, b13 = a11 * v13 + a12 * v23 + a13 * v33;
    float b21 = a21 * v11 + a22 * v21 + a23 * v31, b22 = a21 * v12 + a22 * v22 + a23 * v32, b23 = a21 * v13 + a22 * v23 + a23 * v33;
    float b31 = a31 * v11 + a32 * v21 + a33 * v31, b32 = a31 * v12 + a32 * v22 + a33 * v32, b33 = a31 * v13 + a32 * v23 + a33 * v33;
    float rho1 = b11 * b11 + b21 * b21 + b31 * b31;
    float rho2 = b12 * b12 + b22 * b22 + b32 * b32;
    float rho3 = b13 * b13 + b23 * b23 + b33 * b33;
    bool c = rho1 < rho2;
    cnswap(c, b11, b12); cnswap(c, v11, v12); cnswap(c, b21, b22); cnswap(c, v21, v22); cnswap(c, b31, b32); cnswap(c, v31, v32);
    cswap(c, rho1, rho2);
    c = rho1 < rho3;
    cnswap(c, b11, b13); cnswap(c, v11, v13); cnswap(c, b21, b23); cnswap(c, v21, v23); cnswap(c, b31, b33); cnswap(c, v31, v33);
    cswap(c, rho1, rho3);
    c = rho2 < rho3;
    cnswap(c, b12, b13); cnswap(c, v12, v13); cnswap(c, b22, b23); cnswap(c, v22, v23); cnswap(c, b32, b33); cnswap(c, v32, v33);
    float ch1, sh1, ch2, sh2, ch3, sh3, aa, bb;
    float r11, r12, r13, r21, r22, r23, r31, r32, r33;
    qr_givens(b11, b21, ch1, sh1);
    aa = 1 - 2 * sh1 * sh1;
    bb = 2 * ch1 * sh1;
    r11 = aa * b11 + bb * b21; r12 = aa * b12 + bb * b22; r13 = aa * b13 + bb * b23;
    r21 = -bb * b11 + aa * b21; r22 = -bb * b12 + aa * b22; r23 = -bb * b13 + aa * b23;
    r31 = b31; r32 = b32; r33 = b33;
    qr_givens(r11, r31, ch2, sh2);
    aa = 1 - 2 * sh2 * sh2;
    bb = 2 * ch2 * sh2;
    b11 = aa * r11 + bb * r31; b12 = aa * r12 + bb * r32; b13 = aa * r13 + bb * r33;
    b21 = r21; b22 = r22; b23 = r23;
    b31 = -bb * r11 + aa * r31; b32 = -bb * r12 + aa * r32; b33 = -bb * r13 + aa * r33;
    qr_givens(b22, b32, ch3, sh3);
    aa = 1 - 2 * sh3 * sh3;
    bb = 2 * ch3 * sh3;
    r11 = b11; r12 = b12; r13 = b13;
    r21 = aa * b21 + bb * b31; r22 = aa * b22 + bb * b32; r23 = aa * b23 + bb * b33;
    r31 = -bb * b21 + aa * b31; r32 = -bb * b22 + aa * b32; r33 = -bb * b23 + aa * b33;
    const float sh12 = sh1 * sh1, sh22 = sh2 * sh2, sh32 = sh3 * sh3;
    U[0] = (-1 + 2 * sh12) * (-1 + 2 * sh22);
    U[1] = 4 * ch2 * ch3 * (-1 + 2 * sh12) * sh2 * sh3 + 2 * ch1 * sh1 * (-1 + 2 * sh32);
    U[2] = 4 * ch1 * ch3 * sh1 * sh3 - 2 * ch2 * (-1 + 2 * sh12) * sh2 * (-1 + 2 * sh32);
    U[3] = 2 * ch1 * sh1 * (1 - 2 * sh22);
    U[4] = -8 * ch1 * ch2 * ch3 * sh1 * sh2 * sh3 + (-1 + 2 * sh12) * (-1 + 2 * sh32);
    U[5] = -2 * ch3 * sh3 + 4 * sh1 * (ch3 * sh1 * sh3 + ch1 * ch2 * sh2 * (-1 + 2 * sh32));
    U[6] = 2 * ch2 * sh2;
    U[7] = 2 * ch3 * (1 - 2 * sh22) * sh3;
    U[8] = (-1 + 2 * sh22) * (-1 + 2 * sh32);
    Sg[0] = r11; Sg[1] = r12; Sg[2] = r13; Sg[3] = r21; Sg[4] = r22; Sg[5] = r23; Sg[6] = r31; Sg[7] = r32; Sg[8] = r33;
    V[0] = v11; V[1] = v12; V[2] = v13; V[3] = v21; V[4] = v22; V[5] = v23; V[6] = v31; V[7] = v32; V[8] = v33;
}
} // namespace pf

// SVD3-KERNEL-TEXT-END
// ------------------------------------------------------------------------------------------
// A7/A8: kernGetWallsKD (kernel.cu:974-991) + findCorrespondenceKD (kernel.cu:874-922), fused.
// Target cloud at the PREVIOUS robot pose; out-of-range slots are zero (H2) and still matched.
// ------------------------------------------------------------------------------------------
template <bool PLANAR>
__global__ __launch_bounds__(256) void k_icp_correspond(const float *__restrict__ scan, int nb,
                                                        const float *__restrict__ pose, pf::KdView tree,
                                                        float4 *__restrict__ tar, float4 *__restrict__ cor, int trig = 0)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nb) return;
    const float rx = pose[0], ry = pose[1], rt = pose[2];
    float wx, wy;
    pf::clean_lidar_scan(i, scan[i], rt, wx, wy, trig);
    float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (fabsf(wx) < PF_LIDAR_RANGE && fabsf(wy) < PF_LIDAR_RANGE) {
        t.x = rx + wx;
        t.y = ry + wy;
        t.z = 0.0f;
        t.w = PF_OCCUPIED_WEIGHT;
    }
    const int b = pf::kd_nearest_ref<PLANAR>(tree, t.x, t.y, t.z);
    const uint4 nd = tree.hot[b];
    tar[i] = t;
    cor[i] = make_float4(__uint_as_float(nd.x), __uint_as_float(nd.y), PLANAR ? 0.0f : tree.z[b], tree.w[b]);
}

// A9: means, centring, covariance, SVD, pose (transformPointICP, kernel.cu:1018-1084) in one 1024-thread block:
// the 6 mean components, then the 9 covariance entries, are each one wave's canonical sum (the three
// thrust::reduce calls of the reference have unspecified order); wave 0 finishes with the SVD.
// (the body, for a 1024-thread workgroup: also the tail of k_icp_fused, pfslam_frame.hip.inc)
__device__ __forceinline__ void icp_solve_block(const float4 *__restrict__ tar, const float4 *__restrict__ cor,
                                                int nb, const float *__restrict__ start_ptr,
                                                float *__restrict__ pose_out, float *__restrict__ dbg, float *s_mu, float *s_A)
{
    const float *tf = (const float *)tar, *cf = (const float *)cor;
    const int wave = threadIdx.x >> 6;
    if (wave < 6) {
        const int k = wave % 3;
        const float *src = wave < 3 ? tf : cf;
        const float v = pf::fdiv(wave_sum_canonical(nb, [&](int i) { return src[4 * i + k]; }), (float)nb);
        if ((threadIdx.x & 63) == 0) s_mu[wave] = v;
    }
    __syncthreads();
    if (wave < 9) {
        // W[col j][row r] = sum (tar_r - mu) * (cor_j - mu)  (outerProduct, kernel.cu:862-872);
        // a_rc as handed to svd(): A[j*3+r] = W[col j][row r]
        const int j = wave / 3, r = wave % 3;
        const float mt = s_mu[r], mc = s_mu[3 + j];
        const float v = wave_sum_canonical(nb, [&](int i) {
            const float t = tf[4 * i + r] + (-mt);
            const float c = cf[4 * i + j] + (-mc);
            return t * c;
        });
        if ((threadIdx.x & 63) == 0) s_A[wave] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    float A[9], mu_t[3], mu_c[3];
    for (int e = 0; e < 9; e++) A[e] = s_A[e];
    for (int k = 0; k < 3; k++) {
        mu_t[k] = s_mu[k];
        mu_c[k] = s_mu[3 + k];
    }
    float U[9], S[9], V[9];
    pf::svd3(A, U, S, V);
    // R = U * V^T with glm's column-major evaluation order (kernel.cu:1065-1069)
    float R[9];
    for (int j = 0; j < 3; j++)
        for (int i = 0; i < 3; i++)
            R[j * 3 + i] = U[i * 3 + 0] * V[j * 3 + 0] + U[i * 3 + 1] * V[j * 3 + 1] + U[i * 3 + 2] * V[j * 3 + 2];
    float t[3];
    for (int i = 0; i < 3; i++)
        t[i] = mu_c[i] - (R[0 * 3 + i] * mu_t[0] + R[1 * 3 + i] * mu_t[1] + R[2 * 3 + i] * mu_t[2]);
    const float theta = pf::asinf_spec(R[0 * 3 + 1]);
    if (start_ptr) { // start == nullptr: only the increment (dbg[24..27]); k_icp_apply adds it to the best particle later
        pose_out[0] = start_ptr[0] + t[0];
        pose_out[1] = start_ptr[1] + t[1];
        pose_out[2] = start_ptr[2] + theta;
        pose_out[3] = 0.0f;
    }
    for (int e = 0; e < 9; e++) dbg[e] = A[e];
    for (int k = 0; k < 3; k++) {
        dbg[9 + k] = mu_t[k];
        dbg[12 + k] = mu_c[k];
        dbg[24 + k] = t[k];
    }
    for (int e = 0; e < 9; e++) dbg[15 + e] = R[e];
    dbg[27] = theta;
    dbg[28] = 0.0f;
}
__global__ __launch_bounds__(1024) void k_icp_solve(const float4 *__restrict__ tar, const float4 *__restrict__ cor,
                                                    int nb, const float *__restrict__ start_ptr,
                                                    float *__restrict__ pose_out, float *__restrict__ dbg)
{
    __shared__ float s_mu[6];
    __shared__ float s_A[9];
    icp_solve_block(tar, cor, nb, start_ptr, pose_out, dbg, s_mu, s_A);
}

// ------------------------------------------------------------------------------------------
// A10: kernGetWalls + traceRay (kernel.cu:190-240, 524-549): Bresenham free cells + wall cell
// into a robot-centred local grid.  One lane per beam; the marks are idempotent byte stores.
// ------------------------------------------------------------------------------------------
// traceRay (kernel.cu:190-240) in closed form, one wave per ray ("warp-cooperative write"): after the reference's
// octant swaps the loop runs x = sx .. ex-1 with an integer error term e0 = dx/2, e -= dy, and a y step whenever
// e < 0 (then e += dx).  Since dy <= dx the error stays in [0, dx), so the number of y steps taken before cell k is
// c_k = ceil((k*dy - e0) / dx) -- every cell of the ray is independent and the 64 lanes mark cells k, k+64, ...
// The direction-dependent end-point rule (smaller major coordinate marked, larger not) is the swap itself.
__device__ __forceinline__ void trace_ray_wave(int sx, int sy, int ex, int ey, int dimx, int dimy, uint8_t *__restrict__ out, int lane)
{
    const bool steep = abs(ey - sy) > abs(ex - sx);
    if (steep) {
        int t = sx; sx = sy; sy = t;
        t = ex; ex = ey; ey = t;
    }
    if (sx > ex) {
        int t = sx; sx = ex; ex = t;
        t = sy; sy = ey; ey = t;
    }
    const int deltax = ex - sx;
    const int deltay = abs(ey - sy);
    const int e0 = deltax / 2;
    const int ystep = (ey > sy) ? 1 : -1;
    for (int k = lane; k < deltax; k += 64) {
        const int c = (k * deltay - e0 + deltax - 1) / deltax;
        const int xx = sx + k, yy = sy + ystep * c;
        const int idx = steep ? yy * dimx + xx : xx * dimx + yy;
        if (xx < dimx && yy < dimy && xx >= 0 && yy >= 0 && idx < dimx * dimy) out[idx] = 1;
    }
}

// Round-5 frames: the frame's pose -- best particle (the reduce's global max key) + ICP increment, kernel.cu:1081-1092 -- is formed by
// every kernel that needs it from the keys themselves (one dependent load), so that no launch and no last-workgroup fence sits between
// the reduce and its consumers on three streams.  stats == nullptr: the pose array as before.
struct PoseSrc {
    const long long *stats;
    const float *x, *y, *th, *icp;
    int n;
    // sharded job: every rank's packed keys (world x 16 bytes) and every rank's pose block [x | y | theta] (stride floats each)
    const long long *gkeys = nullptr;
    const float *gpose = nullptr;
    int world = 1, stride = 0;
};
__device__ __forceinline__ void frame_pose(const PoseSrc &s, float start[3], float pose[3])
{
    if (s.gkeys) {
        long long kmax, kmin;
        frame_keys(s.stats, s.gkeys, s.world, kmax, kmin);
        const uint32_t best = 0xFFFFFFFFu - (uint32_t)(kmax & 0xFFFFFFFFll);
        const uint32_t r = best / (uint32_t)s.stride, j = best - r * (uint32_t)s.stride;
        const bool ok = r < (uint32_t)s.world;
        const float *blk = s.gpose + (size_t)(ok ? r : 0u) * 3 * s.stride;
        start[0] = ok ? blk[j] : 0.0f;
        start[1] = ok ? blk[s.stride + j] : 0.0f;
        start[2] = ok ? blk[2 * s.stride + j] : 0.0f;
    } else {
        const uint32_t best = 0xFFFFFFFFu - (uint32_t)(s.stats[0] & 0xFFFFFFFFll);
        const bool mine = best < (uint32_t)s.n;
        start[0] = mine ? s.x[best] : 0.0f;
        start[1] = mine ? s.y[best] : 0.0f;
        start[2] = mine ? s.th[best] : 0.0f;
    }
    pose[0] = start[0] + s.icp[24]; // icp_apply
    pose[1] = start[1] + s.icp[25];
    pose[2] = start[2] + s.icp[27];
}
// kernGetWalls (kernel.cu:524-549): one wave per beam
// centre_from_pose: the 2-D path's cell of the robot (PFUpdateMap, kernel.cu:552-555) computed here from the
// device-resident pose, so the grid step needs no host round trip; otherwise (cx, cy) is the fixed centre of
// the KD path's local grid (kernel.cu:1408-1411).
__global__ __launch_bounds__(256) void k_get_walls(const float *__restrict__ scan, int nb, const float *__restrict__ pose,
                                                   int cx, int cy, uint8_t *__restrict__ free_mask,
                                                   uint8_t *__restrict__ wall_mask, int dimx, int dimy, float resx, float resy,
                                                   int centre_from_pose, PoseSrc src = PoseSrc{nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 1, 0},
                                                   int trig = 0)
{
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= nb) return;
    float ps[3], st[3];
    if (src.stats) frame_pose(src, st, ps);
    else { ps[0] = pose[0]; ps[1] = pose[1]; ps[2] = pose[2]; }
    if (centre_from_pose) {
        cx = (int)roundf(0.5f * (float)dimx + pf::fdiv(ps[0], resx) + resx / 2);
        cy = (int)roundf(0.5f * (float)dimy + pf::fdiv(ps[1], resy) + resy / 2);
    }
    float wx, wy;
    pf::clean_lidar_scan(i, scan[i], ps[2], wx, wy, trig);
    if (fabsf(wx) < PF_LIDAR_RANGE && fabsf(wy) < PF_LIDAR_RANGE) {
        wx = roundf(pf::fdiv(wx, resx));
        wy = roundf(pf::fdiv(wy, resy));
        wx += (float)cx;
        wy += (float)cy;
        trace_ray_wave(cx, cy, (int)wx, (int)wy, dimx, dimy, free_mask, lane);
        if (lane == 0 && wx >= 0 && wx < dimx && wy >= 0 && wy < dimy) wall_mask[(int)(wx * dimx + wy)] = 1;
    }
}

// ------------------------------------------------------------------------------------------
// A11: masks -> ordered point lists (the reference's host double loop, kernel.cu:1435-1461),
// done on the device as count / scan / scatter over 4096-cell blocks so that list order is the
// reference's x-major cell order.  Thread t of a block owns 16 consecutive cells.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int popcount_bytes16(const uint4 v)
{
    // bytes are 0 or 1
    return __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
}

__global__ __launch_bounds__(256) void k_count_cells(const uint8_t *__restrict__ free_mask, const uint8_t *__restrict__ wall_mask,
                                                     int M, int *__restrict__ blk_cnt)
{
    const int base = (blockIdx.x * 256 + threadIdx.x) * 16;
    int cw = 0, cf = 0;
    if (base + 16 <= M) {
        cw = popcount_bytes16(*(const uint4 *)(wall_mask + base));
        cf = popcount_bytes16(*(const uint4 *)(free_mask + base));
    } else {
        for (int k = base; k < M; k++) {
            cw += wall_mask[k] != 0;
            cf += free_mask[k] != 0;
        }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        cw += __shfl_xor(cw, off, 64);
        cf += __shfl_xor(cf, off, 64);
    }
    __shared__ int sw[4], sf[4];
    if ((threadIdx.x & 63) == 0) {
        sw[threadIdx.x >> 6] = cw;
        sf[threadIdx.x >> 6] = cf;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        blk_cnt[2 * blockIdx.x] = sw[0] + sw[1] + sw[2] + sw[3];
        blk_cnt[2 * blockIdx.x + 1] = sf[0] + sf[1] + sf[2] + sf[3];
    }
}

__device__ __forceinline__ float4 cell_to_point(int idx, int dimx, float resx, float resy, float scalex, float scaley,
                                                float rx, float ry)
{
    const int cx = idx / dimx, cy = idx - cx * dimx;
    float px = (float)cx * resx - scalex / 2.0f + rx;
    float py = (float)cy * resy - scaley / 2.0f + ry;
    px = roundf(pf::fdiv(px, resx)) * resx; // ROUND_FRAC, kernel.cu:52
    py = roundf(pf::fdiv(py, resy)) * resy;
    return make_float4(px, py, 0.0f, 0.0f);
}

// clear: this is the last reader of the masks (point-cloud map update): it wipes what it finds, so the masks end the frame
// zeroed and no 5 MB memset is needed before the next k_get_walls
__global__ __launch_bounds__(256) void k_scatter_cells(uint8_t *free_mask, uint8_t *wall_mask,
                                                       int M, const int *__restrict__ blk_cnt, int *__restrict__ counts, int dimx, float resx, float resy,
                                                       float scalex, float scaley, const float *__restrict__ pose,
                                                       int *__restrict__ wall_cell, float4 *__restrict__ wall_pts, int wall_cap,
                                                       int *__restrict__ free_cell, float4 *__restrict__ free_pts, int free_cap, int clear,
                                                       PoseSrc src = PoseSrc{nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 1, 0})
{
    const int base = (blockIdx.x * 256 + threadIdx.x) * 16;
    uint8_t mw[16], mf[16];
    int cw = 0, cf = 0;
    if (base + 16 <= M) { // one 16-byte load per mask
        const uint4 vw = *(const uint4 *)(wall_mask + base), vf = *(const uint4 *)(free_mask + base);
        if (clear) {
            if (vw.x | vw.y | vw.z | vw.w) *(uint4 *)(wall_mask + base) = make_uint4(0, 0, 0, 0);
            if (vf.x | vf.y | vf.z | vf.w) *(uint4 *)(free_mask + base) = make_uint4(0, 0, 0, 0);
        }
        const uint32_t ww[4] = {vw.x, vw.y, vw.z, vw.w}, wf[4] = {vf.x, vf.y, vf.z, vf.w};
#pragma unroll
        for (int k = 0; k < 16; k++) {
            mw[k] = (ww[k >> 2] >> (8 * (k & 3))) & 0xff;
            mf[k] = (wf[k >> 2] >> (8 * (k & 3))) & 0xff;
            cw += mw[k] != 0;
            cf += mf[k] != 0;
        }
    } else {
        for (int k = 0; k < 16; k++) {
            const bool in = base + k < M;
            mw[k] = in ? wall_mask[base + k] : 0;
            mf[k] = in ? free_mask[base + k] : 0;
            cw += mw[k] != 0;
            cf += mf[k] != 0;
            if (clear && in) wall_mask[base + k] = free_mask[base + k] = 0;
        }
    }
    // block-exclusive scan of (cw, cf)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int iw = cw, jf = cf;
    for (int off = 1; off < 64; off <<= 1) {
        const int a = __shfl_up(iw, off, 64), b = __shfl_up(jf, off, 64);
        if (lane >= off) {
            iw += a;
            jf += b;
        }
    }
    __shared__ int sw[4], sf[4];
    if (lane == 63) {
        sw[wave] = iw;
        sf[wave] = jf;
    }
    // offsets of this block = counts of all blocks before it (k_count_cells' raw counts): summed here by the block itself, which
    // saves the separate single-block scan launch; the last block also publishes the list lengths
    int pw = 0, pfr = 0;
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += 256) {
        pw += blk_cnt[2 * b];
        pfr += blk_cnt[2 * b + 1];
    }
    for (int off = 32; off >= 1; off >>= 1) {
        pw += __shfl_xor(pw, off, 64);
        pfr += __shfl_xor(pfr, off, 64);
    }
    __shared__ int spw[4], spf[4];
    if (lane == 0) {
        spw[wave] = pw;
        spf[wave] = pfr;
    }
    __syncthreads();
    const int base_w = spw[0] + spw[1] + spw[2] + spw[3], base_f = spf[0] + spf[1] + spf[2] + spf[3];
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        counts[0] = base_w + sw[0] + sw[1] + sw[2] + sw[3];
        counts[1] = base_f + sf[0] + sf[1] + sf[2] + sf[3];
    }
    // Emission, balanced over the block: a thread whose 16 cells are all marked (the rays' fan around the robot) would otherwise run 16
    // dependent cell_to_point + store rounds while its neighbours idle, and the kernel took as long as its densest wave (19 us, 14 of
    // them here).  Every thread drops the block-local indices of its marked cells into LDS at its place in the block's order, then
    // the block's 256 threads take the list entries round robin: the same lists in the same order, coalesced stores.
    __shared__ unsigned short lw[4096], lf[4096];
    int ow = iw - cw, of = jf - cf; // block-local exclusive offsets
    for (int k = 0; k < wave; k++) {
        ow += sw[k];
        of += sf[k];
    }
    const int tw = sw[0] + sw[1] + sw[2] + sw[3], tf = sf[0] + sf[1] + sf[2] + sf[3];
    if (tw == 0 && tf == 0) return; // (block-uniform)
    const int local = threadIdx.x * 16;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        if (mw[k]) lw[ow++] = (unsigned short)(local + k);
        if (mf[k]) lf[of++] = (unsigned short)(local + k);
    }
    __syncthreads();
    float rx, ry;
    if (src.stats) {
        float ps[3], st[3];
        frame_pose(src, st, ps);
        rx = ps[0];
        ry = ps[1];
    } else {
        rx = pose[0];
        ry = pose[1];
    }
    const int cell0 = blockIdx.x * 4096;
    for (int t = threadIdx.x; t < tw; t += 256) {
        const int o = base_w + t, cell = cell0 + lw[t];
        if (o < wall_cap) {
            wall_cell[o] = cell;
            wall_pts[o] = cell_to_point(cell, dimx, resx, resy, scalex, scaley, rx, ry);
        }
    }
    for (int t = threadIdx.x; t < tf; t += 256) {
        const int o = base_f + t, cell = cell0 + lf[t];
        if (o < free_cap) {
            free_cell[o] = cell;
            free_pts[o] = cell_to_point(cell, dimx, resx, resy, scalex, scaley, rx, ry);
        }
    }
}

__device__ __forceinline__ float node_dist(const pf::KdView &t, int idx, const float4 p)
{
    const uint4 nd = t.hot[idx];
    const float dx = __uint_as_float(nd.x) - p.x, dy = __uint_as_float(nd.y) - p.y, dz = (t.planar ? 0.0f : t.z[idx]) - p.z;
    return pf::fsqrt(dx * dx + dy * dy + dz * dz);
}

// A13: kernUpdateMapKD (kernel.cu:1350-1364) for one cell: the node within a cell diagonal of it gains `val`, clamped.
// H4: the reference's read-modify-write races when several cells map to one node; here every hit is applied (clamped add
// through a CAS loop -- all hits of one pass apply the same function, so the result does not depend on their order).  The free
// pass (-1) is complete before the wall pass (+4) starts, as in the reference: the first rides on k_list_traverse, the second
// on k_test_new, which is launched behind it.
// times: the same step applied that often in one exchange (stops early at a fixed point: the clamp, or a weight so large that the
// step no longer changes it -- further applications would leave the same bits)
__device__ __forceinline__ void map_weight_add(float *kw, int b, int val, int times = 1)
{
    int *addr = (int *)&kw[b];
    int old = *addr, assumed;
    do {
        assumed = old;
        float v = __int_as_float(assumed);
        for (int k = 0; k < times; k++) {
            float nv = v + (float)val;
            nv = (nv < -PF_CLAMP_VAL) ? -PF_CLAMP_VAL : (nv > PF_CLAMP_VAL) ? PF_CLAMP_VAL : nv; // CLAMP, kernel.cu:51
            if (__float_as_int(nv) == __float_as_int(v)) break;
            v = nv;
        }
        old = atomicCAS(addr, assumed, __float_as_int(v));
    } while (old != assumed);
}

// A12: findCorrespondenceIndexKD over the free and the wall list in ONE launch (both are short, latency-bound
// chains; list lengths live on the device).  Virtual index space: [0, n_free) = free list, [n_free, n_free + n_wall) =
// wall list.  zero_tail reproduces the H6 upload bug: free entries >= n_wall are the zero point.
template <bool PLANAR>
__global__ __launch_bounds__(256) void k_list_traverse(float4 *__restrict__ free_pts, int *__restrict__ free_idx, int free_cap,
                                                       const float4 *__restrict__ wall_pts, int *__restrict__ wall_idx, int wall_cap,
                                                       const int *__restrict__ counts, pf::KdView tree, int zero_tail,
                                                       int *__restrict__ wall_leaf, float *kw, float resx, float resy)
{
    const int n_wall = min(counts[0], wall_cap), n_free = min(counts[1], free_cap);
    const float cellDiag = pf::fsqrt(resx * resx + resy * resy);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n_free + n_wall; i += gridDim.x * 256) {
        if (i < n_free) {
            float4 p = free_pts[i];
            if (zero_tail && i >= n_wall) {
                p = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                free_pts[i] = p;
            }
            const int b = pf::kd_nearest_ref<PLANAR>(tree, p.x, p.y, p.z);
            free_idx[i] = b;
            const bool hit = node_dist(tree, b, p) < cellDiag;
            if (zero_tail && i >= n_wall) {
                // H6: every entry behind the first n_wall is the SAME query, so tens of thousands of lanes want the same -1 on the same
                // node -- one compare-and-swap per wave that applies the step as often as the wave has such lanes (the steps are
                // one function applied over and over: their order and grouping cannot matter) instead of one per lane on one address
                const unsigned long long m = __ballot(hit);
                if (hit && (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) map_weight_add(kw, b, PF_FREE_WEIGHT, __popcll(m));
            } else if (hit) map_weight_add(kw, b, PF_FREE_WEIGHT); // the free pass of A13
        } else {
            // the first descent of the same traversal ends on the link KDTree::InsertNode would hang this point on
            const float4 p = wall_pts[i - n_free];
            int leaf;
            wall_idx[i - n_free] = pf::kd_resume<PLANAR, false, true>(tree, p.x, p.y, p.z, INFINITY, 0, 0, nullptr, &leaf);
            wall_leaf[i - n_free] = leaf;
        }
    }
}

// everything the host needs from a frame, written by the frame's last map-update kernel into pinned host memory; `seq` last
__device__ __forceinline__ void write_header(HostHeader *__restrict__ hdr, const int *__restrict__ counts, int n_new, int kd_size,
                                             int flags, const float *__restrict__ sums, const long long *__restrict__ stats,
                                             const float *__restrict__ pose, int seq, const float *__restrict__ sigma, float theta_max)
{
    hdr->cloud_sigma = sigma[0];
    hdr->theta_max = theta_max;
    hdr->n_wall = counts[0];
    hdr->n_free = counts[1];
    hdr->n_new = n_new;
    hdr->kd_size = kd_size;
    hdr->r = sums[0];
    hdr->r2 = sums[1];
    hdr->neff = sums[2];
    hdr->flags = flags;
    for (int k = 0; k < 4; k++) hdr->pose[k] = pose[k];
    hdr->stats[0] = stats[0];
    hdr->stats[1] = stats[1];
    __threadfence_system();
    __hip_atomic_store(&hdr->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM); // the host may poll this word
}

// largest |heading| of the frame's particles: the 64 partial maxima k_group_box leaves (all 64 lanes of a wave call this)
__device__ __forceinline__ float theta_max_of(const float *__restrict__ sigma)
{
    float v = sigma[2 + (threadIdx.x & 63)];
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

__device__ __forceinline__ uint32_t ld_agent(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// A14 + A15: kernTestCorrespondance (kernel.cu:1367-1379), ordered compaction of the walls to insert, and KDTree::InsertNode
// (kdtree.cpp:69-105) for each of them in list order (kernel.cu:1512-1517) -- on the device, one workgroup.
//
// InsertNode walks from the root taking `point < node` on the node's split axis until it falls off, and hangs the new node
// (index = current size, axis = parent's + 1) on that link.  Sequential only among points that fall off the SAME link:
//   * where a new wall falls off the existing tree is the end of the first descent of the traversal k_list_traverse already
//     ran for it (wall_leaf).  Round 1: every new wall claims its link with an atomicMin of its future index; the smallest
//     list position wins -- exactly the point the sequential loop would have hung there first;
//   * everybody else continues below the winner, i.e. among NEW nodes only.  Those live in LDS (x, y, z, axis, links), and
//     the same claim / resolve rounds run there with LDS atomics and two barriers per round, until every point hangs.
//     A round costs ~0.5 us; the number of rounds is the depth of the deepest all-new sub-tree (a few, typically).
// Equal to the sequential result: a point's path only ever contains old nodes and new nodes of SMALLER list position, and
// below one link the contenders are served in list order.  Then the new nodes are written out and the size is bumped.
#define PF_KD_TAG 0x40000000u  /* LDS link claimed in the current round, not yet resolved */
#define PF_KD_NULL 0x7fffffffu /* LDS link: no child */
#define PF_HDR_KD_FULL 1       /* header flag: kd_capacity exhausted, nothing inserted */
#define PF_HDR_CELLS_WIPE 2    /* header flag: the persistent cell rows ask for a wipe (the cloud has left the middle of the window) */
#define PF_HDR_CELLS_FULL 4    /* header flag: ... because the list of claimed cells or the row pool is exhausted */
#define PF_HDR_INTERNAL 8      /* header flag (round-5 frames): the two chains of the map update disagree on the frame's wall list (a bug, reported loudly) */
__global__ __launch_bounds__(1024) void k_test_new(const float4 *__restrict__ pts, const int *__restrict__ idx,
                                                  const int *__restrict__ leaf, int *__restrict__ counts, int cap, pf::KdView tree,
                                                  float resx, float resy, uint4 *hot, int *parent, float *kz, float *kw,
                                                  int *__restrict__ kd_state, int kd_cap, const float *__restrict__ sums,
                                                  const long long *__restrict__ stats, const float *__restrict__ pose,
                                                  HostHeader *__restrict__ hdr, int seq, const int *__restrict__ cell_state, int *__restrict__ touched,
                                                  const float *__restrict__ sigma)
{
    extern __shared__ uint32_t s_dyn[];
    float *lx = (float *)s_dyn, *ly = lx + cap, *lz = ly + cap;
    uint32_t *ll = (uint32_t *)(lz + cap), *lr = ll + cap;
    int *lpar = (int *)(lr + cap), *lax = lpar + cap, *lcur = lax + cap;
    const int n = min(counts[0], cap);
    const float cellDiag = pf::fsqrt(resx * resx + resy * resy), minDist = cellDiag / 2.0f;
    __shared__ int swave[16];
    __shared__ int sbase;
    if (threadIdx.x == 0) sbase = 0;
    __syncthreads();
    for (int r0 = 0; r0 < n; r0 += 1024) {
        const int i = r0 + threadIdx.x;
        bool flag = false;
        float4 p = make_float4(0, 0, 0, 0);
        if (i < n) {
            p = pts[i];
            const float d = node_dist(tree, idx[i], p);
            if (d < cellDiag) map_weight_add(kw, idx[i], PF_OCCUPIED_WEIGHT); // the wall pass of A13 (the free pass is complete)
            flag = d > minDist;
        }
        const unsigned long long m = __ballot(flag);
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) swave[wave] = __popcll(m);
        __syncthreads();
        int off = sbase;
        for (int k = 0; k < wave; k++) off += swave[k];
        if (flag) {
            const int o = off + before;
            lx[o] = p.x;
            ly[o] = p.y;
            lz[o] = p.z;
            ll[o] = PF_KD_NULL;
            lr[o] = PF_KD_NULL;
            lcur[o] = leaf[i];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int tot = 0;
            for (int k = 0; k < 16; k++) tot += swave[k];
            sbase += tot;
        }
        __syncthreads();
    }
    const int n_new = sbase, old = kd_state[0];
    const bool full = n_new > kd_cap - old;
    const int n_ins = full ? 0 : n_new;
    __shared__ int s_touched; // links of the existing tree that gain a node here: what k_cells_update looks its records' links up in
    if (threadIdx.x == 0) s_touched = 0;
    __syncthreads();
    if (n_ins > 0) { // block-uniform
        uint32_t *hw = (uint32_t *)hot;
        const bool planar = tree.planar != 0;
        // round 1: the links of the existing tree
        for (int k = threadIdx.x; k < n_ins; k += 1024) {
            const int at = lcur[k] >> 1, right = lcur[k] & 1;
            const uint32_t cand = (uint32_t)(old + k), axis = ld_agent(&hw[4 * at + 2]) >> 30;
            if (right) {
                atomicMin(&hw[4 * at + 3], cand);
                if (planar && axis == 2) atomicMin(&hw[4 * at + 2], cand | (2u << 30)); // z level of a planar map: both links
            } else {
                atomicMin(&hw[4 * at + 2], cand | (axis << 30));
            }
        }
        __threadfence();
        __syncthreads();
        int pend = 0;
        for (int k = threadIdx.x; k < n_ins; k += 1024) {
            const int at = lcur[k] >> 1, right = lcur[k] & 1;
            const uint32_t la = ld_agent(&hw[4 * at + 2]);
            const uint32_t link = right ? ld_agent(&hw[4 * at + 3]) : (la & 0x3fffffffu);
            if (link == (uint32_t)(old + k)) {
                if (touched) touched[1 + atomicAdd(&s_touched, 1)] = at * 2 + right;
                lpar[k] = at;
                lax[k] = (int)((la >> 30) + 1u) % 3;
                lcur[k] = -1;
            } else {
                lcur[k] = (int)link - old; // continue below the winner, a new node
                pend = 1;
            }
        }
        pend = __syncthreads_or(pend);
        // rounds 2..: among the new nodes, in LDS
        while (pend) {
            for (int k = threadIdx.x; k < n_ins; k += 1024) {
                int a = lcur[k];
                if (a < 0) continue;
                uint32_t *lnk;
                for (;;) {
                    const int ax = lax[a];
                    const float key = ax == 0 ? lx[a] : ax == 1 ? ly[a] : lz[a];
                    const float pv = ax == 0 ? lx[k] : ax == 1 ? ly[k] : lz[k];
                    lnk = pv < key ? &ll[a] : &lr[a];
                    const uint32_t v = *(volatile uint32_t *)lnk;
                    if (v >= PF_KD_TAG) break; // no child yet (or one claimed in this round)
                    a = (int)v;
                }
                atomicMin(lnk, (uint32_t)k | PF_KD_TAG);
                lcur[k] = a * 2 + (lnk == &lr[a] ? 1 : 0);
            }
            __syncthreads();
            pend = 0;
            for (int k = threadIdx.x; k < n_ins; k += 1024) {
                if (lcur[k] < 0) continue;
                const int a = lcur[k] >> 1;
                uint32_t *lnk = (lcur[k] & 1) ? &lr[a] : &ll[a];
                const uint32_t w = *(volatile uint32_t *)lnk & ~PF_KD_TAG; // the winner may already have cleared the tag
                if (w == (uint32_t)k) {
                    *(volatile uint32_t *)lnk = (uint32_t)k;
                    lpar[k] = old + a;
                    lax[k] = (lax[a] + 1) % 3;
                    lcur[k] = -1;
                } else {
                    lcur[k] = (int)w;
                    pend = 1;
                }
            }
            pend = __syncthreads_or(pend);
        }
        for (int k = threadIdx.x; k < n_ins; k += 1024) {
            const int g = old + k, ax = lax[k];
            const int left = ll[k] == PF_KD_NULL ? -1 : old + (int)ll[k], right = lr[k] == PF_KD_NULL ? -1 : old + (int)lr[k];
            hot[g] = pf::pack_hot(lx[k], ly[k], ax, left, right, planar);
            parent[g] = lpar[k];
            kz[g] = (planar && ax == 2) ? __int_as_float(left) : lz[k]; // planar z level: the true left child lives here
            kw[g] = -100.0f;                                            // kernel.cu:1514
        }
    }
    const float theta_max = threadIdx.x < 64 ? theta_max_of(sigma) : 0.0f; // (wave 0)
    __syncthreads();
    if (threadIdx.x == 0) {
        if (touched) touched[0] = s_touched;
        // the cell rows' requests as of the previous update (this frame's k_cells_update runs behind this kernel)
        const int cf = cell_state ? cell_state[PF_CS_FLAGS] : 0;
        const int cflag = ((cf & PF_CF_FAR) ? PF_HDR_CELLS_WIPE : 0) | ((cf & (PF_CF_LIST_FULL | PF_CF_POOL_FULL)) ? PF_HDR_CELLS_FULL : 0);
        counts[2] = n_new;
        counts[3] = (full ? PF_HDR_KD_FULL : 0) | cflag; // for a header written later (k_pack_header, sharded frame)
        kd_state[0] = old + n_ins;
        if (hdr) write_header(hdr, counts, n_new, old + n_ins, (full ? PF_HDR_KD_FULL : 0) | cflag, sums, stats, pose, seq, sigma, theta_max);
    }
}

// the header on its own: frames without a KD map update (first scan, 2-D path) and the sharded frame, whose Neff is only
// known after the weight all-gather
__global__ void k_pack_header(const int *__restrict__ counts, const int *__restrict__ kd_state, const float *__restrict__ sums,
                              const long long *__restrict__ stats, const float *__restrict__ pose, HostHeader *__restrict__ hdr,
                              int after_kd_update, int seq, const float *__restrict__ sigma)
{
    const float theta_max = theta_max_of(sigma); // (launched with one wave)
    if (threadIdx.x != 0) return;
    // after_kd_update: n_new and the flags of the frame's k_test_new, which ran without a header of its own
    write_header(hdr, counts, after_kd_update ? counts[2] : 0, kd_state[0], after_kd_update ? counts[3] : 0, sums, stats, pose, seq, sigma, theta_max);
}

// ------------------------------------------------------------------------------------------
// A16: PFResample (kernel.cu:447-511).  Sums and scan use the canonical orders of DESIGN.md.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_weight_tiles(const float *__restrict__ w, int n, float *__restrict__ tile_r,
                                                     float *__restrict__ tile_r2)
{
    const int t0 = blockIdx.x * PF_SUM_TILE;
    const int cnt = min(PF_SUM_TILE, n - t0);
    // both canonical sums in one pass over the tile (same per-lane order as two separate wave_sum_canonical calls)
    const int lane = threadIdx.x & 63;
    float r = 0.0f, r2 = 0.0f;
#pragma unroll 8
    for (int i = lane; i < cnt; i += 64) {
        const float v = w[t0 + i];
        r = r + v;
        r2 = r2 + v * v;
    }
    for (int off = 32; off >= 1; off >>= 1) {
        r = r + __shfl_xor(r, off, 64);
        r2 = r2 + __shfl_xor(r2, off, 64);
    }
    if (threadIdx.x == 0) {
        tile_r[blockIdx.x] = r;
        tile_r2[blockIdx.x] = r2;
    }
}

// pose = start + (t.x, t.y, theta) of transformPointICP (kernel.cu:1081-1092) when the solve ran ahead on the aux stream
__device__ __forceinline__ void icp_apply(const float *__restrict__ start, const float *__restrict__ dbg, float *__restrict__ pose)
{
    pose[0] = start[0] + dbg[24];
    pose[1] = start[1] + dbg[25];
    pose[2] = start[2] + dbg[27];
    pose[3] = 0.0f;
}
__global__ void k_icp_apply(const float *__restrict__ start, const float *__restrict__ dbg, float *__restrict__ pose)
{
    if (threadIdx.x == 0) icp_apply(start, dbg, pose);
}
// KD frame loop: the frame's pose -- best particle (global max key of the reduce) + ICP increment -- as soon as the scores are
// reduced, so that the map update (the longer branch of the frame's tail) can start without waiting for the weight sums
__global__ void k_best_pose(const long long *__restrict__ stats, const float *__restrict__ x, const float *__restrict__ y,
                            const float *__restrict__ th, int n, float *__restrict__ start, const float *__restrict__ icp_dbg,
                            float *__restrict__ pose)
{
    if (threadIdx.x != 0) return;
    const uint32_t best = 0xFFFFFFFFu - (uint32_t)(stats[0] & 0xFFFFFFFFll);
    const bool mine = best < (uint32_t)n;
    start[0] = mine ? x[best] : 0.0f;
    start[1] = mine ? y[best] : 0.0f;
    start[2] = mine ? th[best] : 0.0f;
    start[3] = 0.0f;
    icp_apply(start, icp_dbg, pose);
}
__global__ __launch_bounds__(64) void k_weight_final(const float *__restrict__ tile_r, const float *__restrict__ tile_r2, int nt,
                                                     int n, float *__restrict__ sums, const float *__restrict__ icp_start,
                                                     const float *__restrict__ icp_dbg, float *__restrict__ pose)
{
    if (icp_start && threadIdx.x == 0) icp_apply(icp_start, icp_dbg, pose); // rides along: one launch less on the chain
    float r, r2;
    if (n <= PF_SUM_TILE) { // a single tile IS the canonical sum
        r = tile_r[0];
        r2 = tile_r2[0];
    } else {
        r = wave_sum_canonical(nt, [&](int i) { return tile_r[i]; });
        r2 = wave_sum_canonical(nt, [&](int i) { return tile_r2[i]; });
    }
    if (threadIdx.x == 0) {
        sums[0] = r;
        sums[1] = r2;
        sums[2] = pf::fdiv(r * r, r2); // Neff, kernel.cu:472
    }
}

// Up to one sum tile (4096 particles -- the reference runs 50 .. 1000): k_weights_apply + k_weight_tiles + k_weight_final as ONE
// workgroup, one launch instead of three on the frame's chain of dependent launches (~5 us each; a frame of the reference's
// own size is nothing but that chain).  No cross-workgroup step, so no device-scope fence: barriers only.
template <typename T>
__global__ __launch_bounds__(256) void k_weights_small(float *__restrict__ w, float *__restrict__ wm, const T *__restrict__ fit, int n,
                                                       int mirror_count, const long long *__restrict__ stats,
                                                       const float *__restrict__ x, const float *__restrict__ y,
                                                       const float *__restrict__ th, float *__restrict__ start,
                                                       float *__restrict__ sums, const float *__restrict__ icp_dbg,
                                                       float *__restrict__ pose)
{
    __shared__ float s_w[PF_SUM_TILE];
    const long long kmax = stats[0], kmin = stats[1];
    bool scale = false;
    float c = 0.0f, base = 0.0f;
    if (std::is_same<T, float>::value) { // kernUpdateWeights (kernel.cu:287-304): w *= (fit - (int)min) / (max - min)
        const float fmax = ordered_to_f32((int)(kmax >> 32));
        const float fmin = -ordered_to_f32((int)(kmin >> 32));
        const float rng = fmax - fmin;
        scale = rng > 0.0f;
        if (scale) {
            c = pf::fdiv(1.0f, rng);
            base = (float)(int)fmin;
        }
    } else {
        const int imax = (int)(kmax >> 32), imin = -(int)(kmin >> 32);
        const int rng = imax - imin;
        scale = rng > 0;
        if (scale) {
            c = pf::fdiv(1.0f, (float)rng);
            base = (float)imin;
        }
    }
    for (int i = threadIdx.x; i < n; i += 256) {
        float wi = w[i];
        if (scale) wi = wi * ((float)fit[i] - base) * c;
        w[i] = wi;
        if (i < mirror_count) wm[i] = wi;
        s_w[i] = wi;
    }
    __syncthreads();
    if (threadIdx.x >= 64) return;
    // the canonical sums of one tile (k_weight_tiles), on the first wave
    const int lane = threadIdx.x;
    float r = 0.0f, r2 = 0.0f;
    for (int i = lane; i < n; i += 64) {
        const float v = s_w[i];
        r = r + v;
        r2 = r2 + v * v;
    }
    for (int off = 32; off >= 1; off >>= 1) {
        r = r + __shfl_xor(r, off, 64);
        r2 = r2 + __shfl_xor(r2, off, 64);
    }
    if (lane == 0) {
        if (start) { // not already done by k_best_pose
            const uint32_t best = 0xFFFFFFFFu - (uint32_t)(kmax & 0xFFFFFFFFll); // best particle's pose (unsharded: goff == 0)
            const bool mine = best < (uint32_t)n;
            const float bx = mine ? x[best] : 0.0f, by = mine ? y[best] : 0.0f, bt = mine ? th[best] : 0.0f;
            start[0] = bx;
            start[1] = by;
            start[2] = bt;
            start[3] = 0.0f;
            if (icp_dbg) { // pose = start + increment of transformPointICP (kernel.cu:1081-1092)
                pose[0] = bx + icp_dbg[24];
                pose[1] = by + icp_dbg[25];
                pose[2] = bt + icp_dbg[27];
                pose[3] = 0.0f;
            }
        }
        sums[0] = r;
        sums[1] = r2;
        sums[2] = pf::fdiv(r * r, r2); // Neff, kernel.cu:472
    }
}

// canonical inclusive scan, pass 1: totals of 1024-element tiles (lane = 16-element chunk)
__device__ __forceinline__ float chunk_run(const float *__restrict__ w, int c0, int n, float *local /*16*/)
{
    float run = 0.0f;
    for (int k = 0; k < PF_SCAN_CHUNK; k++) {
        if (c0 + k < n) run = (k == 0) ? w[c0 + k] : run + w[c0 + k];
        local[k] = run;
    }
    return run;
}
__device__ __forceinline__ float chunk_offset_seq(float tot, int lane, float &tile_total)
{
    float run = 0.0f, mine = 0.0f;
    for (int k = 0; k < 64; k++) {
        const float t = __shfl(tot, k, 64);
        if (lane == k) mine = run;
        run = run + t;
    }
    tile_total = run;
    return mine;
}
// Resample gate: the frame loop launches the resample kernels in EVERY frame and they decide on the device whether the frame
// resamples -- Neff < 0.7 N, kernel.cu:474, on the sums k_weight_final left -- so that no frame waits for the host.
// gate == nullptr: the caller has decided (stage-level API, sharded frame).
__device__ __forceinline__ bool resample_gate(const float *__restrict__ gate, double threshold)
{
    return gate == nullptr || (double)gate[2] < threshold;
}
__global__ __launch_bounds__(64) void k_scan_tiles(const float *__restrict__ w, int n, float *__restrict__ tile_tot,
                                                   const float *__restrict__ gate, double thr)
{
    if (!resample_gate(gate, thr)) return;
    const int lane = threadIdx.x, c0 = blockIdx.x * PF_SCAN_TILE + lane * PF_SCAN_CHUNK;
    float local[PF_SCAN_CHUNK];
    const float tot = (c0 < n) ? chunk_run(w, c0, n, local) : 0.0f;
    float total;
    chunk_offset_seq(tot, lane, total);
    if (lane == 0) tile_tot[blockIdx.x] = total;
}
// tile offsets: strictly sequential float adds in tile order (the canonical scan order) -- but only the adds are serial:
// the 64 lanes stage 1024 tile totals at a time in LDS, lane 0 runs the chain out of LDS, all lanes store.
// (At 8 x 100 k particles a resample frame has 782 tiles; with a global load and store per step this kernel took ~40 us.)
__global__ __launch_bounds__(64) void k_scan_offsets(const float *__restrict__ tile_tot, int nt, float *__restrict__ tile_off,
                                                     const float *__restrict__ gate, double thr)
{
    if (!resample_gate(gate, thr)) return;
    __shared__ float buf[1024];
    float off = 0.0f;
    for (int t0 = 0; t0 < nt; t0 += 1024) {
        const int m = min(1024, nt - t0);
        for (int k = threadIdx.x; k < m; k += 64) buf[k] = tile_tot[t0 + k];
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int k = 0; k < m; k++) {
                const float v = buf[k];
                buf[k] = off;
                off = off + v;
            }
        }
        __syncthreads();
        for (int k = threadIdx.x; k < m; k += 64) tile_off[t0 + k] = buf[k];
        __syncthreads();
    }
}
__global__ __launch_bounds__(64) void k_scan_apply(const float *__restrict__ w, int n, const float *__restrict__ tile_off,
                                                   float *__restrict__ cdf, float *__restrict__ chunk_max,
                                                   float *__restrict__ tile_max, const float *__restrict__ gate, double thr)
{
    if (!resample_gate(gate, thr)) return;
    const int lane = threadIdx.x, c0 = blockIdx.x * PF_SCAN_TILE + lane * PF_SCAN_CHUNK;
    float local[PF_SCAN_CHUNK];
    const float tot = (c0 < n) ? chunk_run(w, c0, n, local) : 0.0f;
    float total;
    const float coff = chunk_offset_seq(tot, lane, total);
    float cmax = -INFINITY;
    if (c0 < n) {
        const float base = tile_off[blockIdx.x] + coff;
        for (int k = 0; k < PF_SCAN_CHUNK && c0 + k < n; k++) {
            const float v = base + local[k];
            cdf[c0 + k] = v;
            cmax = fmaxf(cmax, v);
        }
        chunk_max[c0 / PF_SCAN_CHUNK] = cmax;
    }
    const float tmax = wave_max_f32(cmax);
    if (lane == 0) tile_max[blockIdx.x] = tmax;
}
__global__ __launch_bounds__(64) void k_scan_pmax(float *__restrict__ tile_max, int nt, const float *__restrict__ gate, double thr)
{
    if (!resample_gate(gate, thr)) return;
    // running maximum over the tiles: max is associative, so a plain wave scan per 64 tiles + a carried maximum
    float carry = -INFINITY;
    for (int t0 = 0; t0 < nt; t0 += 64) {
        const int t = t0 + (int)threadIdx.x;
        float m = t < nt ? tile_max[t] : -INFINITY;
        for (int off = 1; off < 64; off <<= 1) {
            const float u = __shfl_up(m, off, 64);
            if ((int)threadIdx.x >= off) m = fmaxf(m, u);
        }
        m = fmaxf(m, carry);
        if (t < nt) tile_max[t] = m;
        carry = __shfl(m, 63, 64);
    }
}

// ---- frame loops above 4096 particles: the same passes in five launches instead of eight -----------------------------------------
// Both first passes read every weight once and keep nothing: the tile sums of Neff (k_weight_tiles, 4096-element tiles) and the
// tile totals of the scan (k_scan_tiles, 1024-element tiles) -- one launch, always (the scan's share costs ~1 us when the frame
// then does not resample, a launch of its own ~5 us either way).
__global__ __launch_bounds__(256) void k_weight_scan_tiles(const float *__restrict__ w, int n, float *__restrict__ tile_r,
                                                           float *__restrict__ tile_r2, float *__restrict__ tile_tot)
{
    // four waves per 4096-element sum tile: each takes one of its four 1024-element scan tiles, the first also the sums
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nt = (n + PF_SCAN_TILE - 1) / PF_SCAN_TILE;
    static_assert(PF_SUM_TILE / PF_SCAN_TILE == 4, "one wave per scan tile of a sum tile");
    const int t = blockIdx.x * (PF_SUM_TILE / PF_SCAN_TILE) + wave;
    if (t < nt) {
        const int c0 = t * PF_SCAN_TILE + lane * PF_SCAN_CHUNK;
        float local[PF_SCAN_CHUNK];
        const float tot = (c0 < n) ? chunk_run(w, c0, n, local) : 0.0f;
        float total;
        chunk_offset_seq(tot, lane, total);
        if (lane == 0) tile_tot[t] = total;
    }
    if (wave != 0) return;
    const int t0 = blockIdx.x * PF_SUM_TILE;
    const int cnt = min(PF_SUM_TILE, n - t0);
    float r = 0.0f, r2 = 0.0f;
#pragma unroll 8
    for (int i = lane; i < cnt; i += 64) {
        const float v = w[t0 + i];
        r = r + v;
        r2 = r2 + v * v;
    }
    for (int off = 32; off >= 1; off >>= 1) {
        r = r + __shfl_xor(r, off, 64);
        r2 = r2 + __shfl_xor(r2, off, 64);
    }
    if (lane == 0) {
        tile_r[blockIdx.x] = r;
        tile_r2[blockIdx.x] = r2;
    }
}
// k_weight_final, and -- when its Neff says the frame resamples -- k_scan_offsets right behind it in the same workgroup
__global__ __launch_bounds__(64) void k_weight_final_offsets(const float *__restrict__ tile_r, const float *__restrict__ tile_r2, int nt_sum,
                                                             int n, float *__restrict__ sums, const float *__restrict__ icp_start,
                                                             const float *__restrict__ icp_dbg, float *__restrict__ pose,
                                                             const float *__restrict__ tile_tot, int nt, float *__restrict__ tile_off,
                                                             double thr)
{
    if (icp_start && threadIdx.x == 0) icp_apply(icp_start, icp_dbg, pose);
    float r, r2;
    if (n <= PF_SUM_TILE) {
        r = tile_r[0];
        r2 = tile_r2[0];
    } else {
        r = wave_sum_canonical(nt_sum, [&](int i) { return tile_r[i]; });
        r2 = wave_sum_canonical(nt_sum, [&](int i) { return tile_r2[i]; });
    }
    const float neff = pf::fdiv(r * r, r2); // kernel.cu:472
    if (threadIdx.x == 0) {
        sums[0] = r;
        sums[1] = r2;
        sums[2] = neff;
    }
    if (!((double)neff < thr)) return; // every lane holds the same bits
    __shared__ float buf[1024];
    float off = 0.0f;
    for (int t0 = 0; t0 < nt; t0 += 1024) {
        const int m = min(1024, nt - t0);
        for (int k = threadIdx.x; k < m; k += 64) buf[k] = tile_tot[t0 + k];
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int k = 0; k < m; k++) {
                const float v = buf[k];
                buf[k] = off;
                off = off + v;
            }
        }
        __syncthreads();
        for (int k = threadIdx.x; k < m; k += 64) tile_off[t0 + k] = buf[k];
        __syncthreads();
    }
}

// kernWeightedSample (kernel.cu:429-444): `while (rnd > cdf[idx]) idx++` = first idx with
// rnd <= cdf[idx]; found through tile prefix-maxima, chunk maxima, then the chunk itself, which
// is exact for any cdf (also a non-monotone one, H8).  The engine is seeded exactly as the
// reference does, collisions included (H5).  gn = number of global particles (cdf length).
// mode (pfslam_set_resampler, uniform over the launch) changes only where thread i takes its rnd from: 0 = the reference's seeding (the
// particle index lands in the key's 9-bit field: 512 distinct draws whatever gn is); 1 = the same function with the particle index in
// the argument that is hashed whole (one multinomial draw per particle); 2 = systematic: one draw u of the frame, rnd_i =
// ((i + u) * maxv) / gn in double -- add, multiply, divide, in that order (nothing there can contract into an fma), rounded to float once.
__device__ __forceinline__ float sample_rnd(float maxv, int gn, float neff, int frame, int global_i, int mode)
{
    if (mode == 2) {
        uint32_t gen = pf::engine_seed((int)neff, frame, 0);
        const float u = pf::uniform_real(gen, 0.0f, 1.0f);
        return (float)((((double)global_i + (double)u) * (double)maxv) / (double)gn);
    }
    uint32_t gen = mode == 1 ? pf::engine_seed((int)neff, global_i, frame) : pf::engine_seed((int)neff, frame, global_i);
    return pf::uniform_real(gen, 0.0f, maxv);
}
__device__ __forceinline__ int sample_index(const float *__restrict__ cdf, const float *__restrict__ chunk_max,
                                            const float *__restrict__ tile_pmax, int gn, float neff, int frame, int global_i, int mode)
{
    const float maxv = cdf[gn - 1];
    const float rnd = sample_rnd(maxv, gn, neff, frame, global_i, mode);
    const int nt = (gn + PF_SCAN_TILE - 1) / PF_SCAN_TILE;
    int lo = 0, hi = nt; // first tile with prefix-max >= rnd
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tile_pmax[mid] >= rnd) hi = mid; else lo = mid + 1;
    }
    int idx = gn - 1;
    if (lo < nt) {
        const int c_begin = lo * (PF_SCAN_TILE / PF_SCAN_CHUNK);
        const int c_end = min((gn + PF_SCAN_CHUNK - 1) / PF_SCAN_CHUNK, c_begin + PF_SCAN_TILE / PF_SCAN_CHUNK);
        int c = c_begin;
        while (c < c_end && !(chunk_max[c] >= rnd)) c++;
        if (c < c_end) {
            int k = c * PF_SCAN_CHUNK;
            const int k_end = min(gn, k + PF_SCAN_CHUNK);
            while (k < k_end && rnd > cdf[k]) k++;
            idx = min(k, gn - 1);
        }
    }
    return idx;
}
__global__ __launch_bounds__(256) void k_sample(const float *__restrict__ cdf, const float *__restrict__ chunk_max,
                                                const float *__restrict__ tile_pmax, int gn, int n, int goff, int frame,
                                                const float *__restrict__ sums, int *__restrict__ src,
                                                const float *__restrict__ gate, double thr, int mode)
{
    if (!resample_gate(gate, thr)) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    src[i] = sample_index(cdf, chunk_max, tile_pmax, gn, sums[2], frame, goff + i, mode);
}

// Frame loops (unsharded): k_sample + k_gather in one launch that runs in EVERY frame and always moves the particles from one
// pose block to the other -- from their sampled sources when the frame resamples (Neff < 0.7 N, decided here on the device), from
// themselves otherwise -- so the host can swap the two blocks unconditionally and no copy back is needed.
#define PF_PMAX_LDS 4096 /* tile maxima a workgroup of k_sample_gather turns into prefix maxima itself: up to 4 M particles */
// gn = global particle count (length of the cdf), n = particles of this handle = global [goff, goff + n); gpose = the rank-major
// pose blocks [rank][x | y | theta] (stride floats each) every sampled source is read from -- the handle's own block when it is
// not sharded (goff == 0, gn == n, SHARDED == false: no division).
template <bool LOCAL_PMAX, bool SHARDED> // LOCAL_PMAX false: tile_max already holds the prefix maxima (k_scan_pmax ran)
__global__ __launch_bounds__(256) void k_sample_gather(const float *__restrict__ cdf, const float *__restrict__ chunk_max,
                                                       const float *__restrict__ tile_max, int gn, int n, int goff, int frame,
                                                       const float *__restrict__ sums, int *__restrict__ src,
                                                       const float *__restrict__ gpose, float *__restrict__ blk2, int stride,
                                                       float *__restrict__ w, float *__restrict__ wm, double thr, int mode)
{
    __shared__ float s_pmax[LOCAL_PMAX ? PF_PMAX_LDS : 1];
    const bool doit = (double)sums[2] < thr;
    if (LOCAL_PMAX && doit) { // k_scan_pmax, per workgroup: the running maximum over the tiles is associative, so a wave scan + a carry
        const int nt = (gn + PF_SCAN_TILE - 1) / PF_SCAN_TILE;
        if (threadIdx.x < 64) {
            float carry = -INFINITY;
            for (int t0 = 0; t0 < nt; t0 += 64) {
                const int t = t0 + (int)threadIdx.x;
                float m = t < nt ? tile_max[t] : -INFINITY;
                for (int off = 1; off < 64; off <<= 1) {
                    const float u = __shfl_up(m, off, 64);
                    if ((int)threadIdx.x >= off) m = fmaxf(m, u);
                }
                m = fmaxf(m, carry);
                if (t < nt) s_pmax[t] = m;
                carry = __shfl(m, 63, 64);
            }
        }
        __syncthreads();
    }
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int s = goff + i;
    if (doit) {
        s = sample_index(cdf, chunk_max, LOCAL_PMAX ? (const float *)s_pmax : tile_max, gn, sums[2], frame, goff + i, mode);
        src[i] = s;
        w[i] = 1.0f; // kernel.cu:441-442
        wm[i] = 1.0f;
    }
    const float *blk = gpose;
    if (SHARDED) {
        const int r = s / stride;
        s -= r * stride;
        blk += (size_t)r * 3 * stride;
    }
    blk2[i] = blk[s];
    blk2[stride + i] = blk[stride + s];
    blk2[2 * stride + i] = blk[2 * stride + s];
}

// particles[i] = particles[idx]; w = 1 (kernel.cu:441-442), gathered from a snapshot (H3).  The snapshot is the rank-major
// array of pose blocks [rank][x | y | theta] (stride floats each): global index s lives in block s / stride.
__global__ __launch_bounds__(256) void k_gather(const float *__restrict__ gpose, int stride, const int *__restrict__ src, int n,
                                                float *__restrict__ x2, float *__restrict__ y2, float *__restrict__ th2,
                                                float *__restrict__ w, float *__restrict__ wm)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int s = src[i];
    const int r = s / stride, k = s - r * stride;
    const float *blk = gpose + (size_t)r * 3 * stride;
    x2[i] = blk[k];
    y2[i] = blk[stride + k];
    th2[i] = blk[2 * stride + k];
    w[i] = 1.0f;
    wm[i] = 1.0f;
}

// Up to 4096 particles (four scan tiles): the whole gated resample of a frame as ONE workgroup -- the four scan passes and
// k_sample_gather, tile for tile and lane for lane, separated by barriers instead of kernel boundaries.
__global__ __launch_bounds__(1024) void k_resample_small(const float *w_in, int n, float *__restrict__ cdf,
                                                        float *__restrict__ chunk_max, float *__restrict__ tile_pmax, int frame,
                                                        const float *__restrict__ sums, int *__restrict__ src,
                                                        const float *__restrict__ blk, float *__restrict__ blk2, int stride,
                                                        float *w, float *__restrict__ wm, double thr, int mode)
{
    const bool doit = (double)sums[2] < thr; // Neff < 0.7 N (kernel.cu:474)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nt = (n + PF_SCAN_TILE - 1) / PF_SCAN_TILE; // <= 4: one tile per wave
    __shared__ float s_tot[4], s_off[4], s_max[4];
    if (doit) {
        float local[PF_SCAN_CHUNK];
        const int c0 = wave * PF_SCAN_TILE + lane * PF_SCAN_CHUNK;
        float tot = 0.0f, total = 0.0f, coff = 0.0f;
        if (wave < nt) { // k_scan_tiles
            tot = (c0 < n) ? chunk_run(w_in, c0, n, local) : 0.0f;
            coff = chunk_offset_seq(tot, lane, total);
            if (lane == 0) s_tot[wave] = total;
        }
        __syncthreads();
        if (threadIdx.x == 0) { // k_scan_offsets: strictly sequential
            float off = 0.0f;
            for (int t = 0; t < nt; t++) {
                s_off[t] = off;
                off = off + s_tot[t];
            }
        }
        __syncthreads();
        if (wave < nt) { // k_scan_apply
            float cmax = -INFINITY;
            if (c0 < n) {
                const float base = s_off[wave] + coff;
                for (int k = 0; k < PF_SCAN_CHUNK && c0 + k < n; k++) {
                    const float v = base + local[k];
                    cdf[c0 + k] = v;
                    cmax = fmaxf(cmax, v);
                }
                chunk_max[c0 / PF_SCAN_CHUNK] = cmax;
            }
            const float tmax = wave_max_f32(cmax);
            if (lane == 0) s_max[wave] = tmax;
        }
        __syncthreads();
        if (threadIdx.x == 0) { // k_scan_pmax
            float m = -INFINITY;
            for (int t = 0; t < nt; t++) {
                m = fmaxf(m, s_max[t]);
                tile_pmax[t] = m;
            }
        }
        __threadfence_block();
        __syncthreads(); // cdf, chunk_max, tile_pmax of this workgroup are visible to all its threads from here on
    }
    const float neff = sums[2];
    for (int i = threadIdx.x; i < n; i += 1024) { // k_sample_gather
        int sidx = i;
        if (doit) {
            sidx = sample_index(cdf, chunk_max, tile_pmax, n, neff, frame, i, mode);
            src[i] = sidx;
        }
        blk2[i] = blk[sidx];
        blk2[stride + i] = blk[stride + sidx];
        blk2[2 * stride + i] = blk[2 * stride + sidx];
    }
    if (doit) {
        for (int i = threadIdx.x; i < n; i += 1024) { // the scan read every weight before the barriers above
            w[i] = 1.0f; // kernel.cu:441-442
            wm[i] = 1.0f;
        }
    }
}

// ------------------------------------------------------------------------------------------
// A17/A18: 2-D occupancy-grid path (GPU-branch semantics of the reference, H7)
// ------------------------------------------------------------------------------------------
// EvaluateParticle + mapCorrelation (kernel.cu:243-274): int accumulate, no range reject.
__global__ __launch_bounds__(256) void k_score_grid(const int8_t *__restrict__ grid, int dimx, int dimy, float scalex, float scaley,
                                                    float resx, float resy, const float *__restrict__ px,
                                                    const float *__restrict__ py, const float *__restrict__ pth, int n,
                                                    const float *__restrict__ scan, const pf::BeamParts *__restrict__ beams, int nb,
                                                    int beams_per_chunk, int *__restrict__ out, int trig = 0)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int j0 = blockIdx.y * beams_per_chunk, j1 = min(nb, j0 + beams_per_chunk);
    if (i >= n) return;
    const float x = px[i], y = py[i], th = pth[i];
    const pf::AngleParts T = pf::angle_parts(th);
    const float offx = pf::fdiv(0.5f * scalex, resx), offy = pf::fdiv(0.5f * scaley, resy);
    int acc = 0;
    for (int j = j0; j < j1; j++) {
        float wx, wy;
        beam_end_point_rt(beams, j, scan[j], th, T, wx, wy, trig);
        wx += x;
        wy += y;
        wx = roundf(offx + pf::fdiv(wx, resx));
        wy = roundf(offy + pf::fdiv(wy, resy));
        if (wx >= 0 && wx < dimx && wy >= 0 && wy < dimy) acc += grid[(int)wx * dimx + (int)wy];
    }
    out[(size_t)blockIdx.y * n + i] = acc;
}
// integer partials: any order gives the reference's sum, so the four waves of a block split the chunks of 64 particles
__global__ __launch_bounds__(256) void k_reduce_partials_i32(const int *__restrict__ partial, int n, int chunks, int *__restrict__ fit)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + lane;
    __shared__ int part[4][64];
    int a = 0;
    if (i < n) {
        int c = wave;
        for (; c + 28 < chunks; c += 32) {
            int v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] = partial[(size_t)(c + 4 * k) * n + i];
#pragma unroll
            for (int k = 0; k < 8; k++) a += v[k];
        }
        for (; c < chunks; c += 4) a += partial[(size_t)c * n + i];
    }
    part[wave][lane] = a;
    __syncthreads();
    if (wave == 0 && i < n) fit[i] = part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane];
}
// kernUpdateMap (kernel.cu:513-522)
__global__ __launch_bounds__(256) void k_update_grid(int M, int8_t *__restrict__ grid, const uint8_t *__restrict__ mask, int val)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    if (mask[i]) {
        int v = (int)grid[i] + val;
        v = v < -113 ? -113 : v > 113 ? 113 : v;
        grid[i] = (int8_t)v;
    }
}

// ==========================================================================================
// C-ABI, stages
// ==========================================================================================
static int mirror_count(const pfslam_handle *h)
{
    // cudaMemcpy(particles, dev_particles, N * sizeof(glm::vec4)) copies 16*N of the 32*N bytes: the weights
    // (offset 12) of particles 0 .. ceil(N/2)-1 reach the host array (kernel.cu:1341, H11)
    return h->cfg.strict_host_mirror ? (h->gn + 1) / 2 : INT_MAX;
}

static int launch_stats_reset(pfslam_handle *h, hipStream_t st)
{
    hipLaunchKernelGGL(k_stats_reset, dim3(1), dim3(64), 0, st, (long long *)h->stats);
    HIPCHK(hipGetLastError());
    return 0;
}
static int launch_minmax(pfslam_handle *h, bool int_fit)
{
    if (!h->stats_clean) CHK(launch_stats_reset(h, h->stream));
    h->stats_clean = false;
    const int blocks = std::min(1024, (h->n + 255) / 256);
    if (int_fit)
        hipLaunchKernelGGL(k_minmax<int>, dim3(blocks), dim3(256), 0, h->stream, (const int *)h->fit_i, h->n, h->goff, (long long *)h->stats);
    else
        hipLaunchKernelGGL(k_minmax<float>, dim3(blocks), dim3(256), 0, h->stream, (const float *)h->fit, h->n, h->goff, (long long *)h->stats);
    HIPCHK(hipGetLastError());
    return 0;
}
static int launch_weights(pfslam_handle *h, bool int_fit, bool write_start = true)
{
    const dim3 g((h->n + 255) / 256);
    float *start = write_start ? h->start : (float *)nullptr;
    if (int_fit)
        hipLaunchKernelGGL(k_weights_apply<int>, g, dim3(256), 0, h->stream, h->w, h->wm, (const int *)h->fit_i, h->n, h->goff,
                           mirror_count(h), (const long long *)h->stats, h->x, h->y, h->th, start);
    else
        hipLaunchKernelGGL(k_weights_apply<float>, g, dim3(256), 0, h->stream, h->w, h->wm, (const float *)h->fit, h->n, h->goff,
                           mirror_count(h), (const long long *)h->stats, h->x, h->y, h->th, start);
    HIPCHK(hipGetLastError());
    return 0;
}

// frame loops with up to one sum tile of particles: weight update, sums, Neff, best pose (+ ICP increment) in one launch
static int launch_weights_small(pfslam_handle *h, bool int_fit, bool apply_icp, bool write_start = true)
{
    const float *dbg = apply_icp ? (const float *)h->icp_dbg : (const float *)nullptr;
    float *start = write_start ? h->start : (float *)nullptr;
    if (int_fit)
        hipLaunchKernelGGL(k_weights_small<int>, dim3(1), dim3(256), 0, h->stream, h->w, h->wm, (const int *)h->fit_i, h->n,
                           mirror_count(h), (const long long *)h->stats, h->x, h->y, h->th, start, h->sums, dbg, h->pose);
    else
        hipLaunchKernelGGL(k_weights_small<float>, dim3(1), dim3(256), 0, h->stream, h->w, h->wm, (const float *)h->fit, h->n,
                           mirror_count(h), (const long long *)h->stats, h->x, h->y, h->th, start, h->sums, dbg, h->pose);
    HIPCHK(hipGetLastError());
    return 0;
}

static int host_ordered_to_f32(int s)
{
    return s ^ ((s >> 31) & 0x7fffffff);
}
static int read_stats(pfslam_handle *h, int *best, float *fmin, float *fmax, bool int_fit)
{
    int64_t st[2];
    HIPCHK(hipMemcpyAsync(st, h->stats, 16, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const uint32_t b = 0xFFFFFFFFu - (uint32_t)(st[0] & 0xFFFFFFFFll);
    if (best) *best = (int)b;
    int hi = (int)(st[0] >> 32), lo = (int)(st[1] >> 32);
    if (int_fit) {
        if (fmax) *fmax = (float)hi;
        if (fmin) *fmin = (float)(-lo);
    } else {
        int a = host_ordered_to_f32(hi), c = host_ordered_to_f32(lo);
        float fa, fc;
        memcpy(&fa, &a, 4);
        memcpy(&fc, &c, 4);
        if (fmax) *fmax = fa;
        if (fmin) *fmin = -fc;
    }
    h->trace[0] = (int)b;
    return 0;
}

extern "C" int pfslam_measurement_local(pfslam_handle *h)
{
    if (!h) return fail("null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    CHK(settle_staged(h));
    return launch_minmax(h, false);
}
extern "C" int pfslam_measurement_apply(pfslam_handle *h, int *best_global, float *fmin, float *fmax)
{
    if (!h) return fail("null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    CHK(settle_staged(h));
    CHK(launch_weights(h, false));
    if (best_global || fmin || fmax) CHK(read_stats(h, best_global, fmin, fmax, false));
    return 0;
}
extern "C" int pfslam_measurement_update(pfslam_handle *h, int *best, float *fmin, float *fmax)
{
    if (!h) return fail("null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    CHK(settle_staged(h));
    CHK(launch_minmax(h, false));
    CHK(launch_weights(h, false));
    if (best || fmin || fmax) CHK(read_stats(h, best, fmin, fmax, false));
    return 0;
}

// ---- ICP ---------------------------------------------------------------------------------
static int launch_icp(pfslam_handle *h, hipStream_t st = nullptr, bool with_start = true)
{
    if (h->kd_size <= 0) return fail("pfslam_icp: no map loaded");
    if (h->nb > PF_SUM_TILE) return fail("pfslam_icp: n_beams > 4096 not supported");
    if (!st) st = h->stream;
    const dim3 g((h->nb + 255) / 256);
    if (h->planar)
        hipLaunchKernelGGL(k_icp_correspond<true>, g, dim3(256), 0, st, h->scan, h->nb, h->pose, kd_view(h),
                           (float4 *)h->icp_tar, (float4 *)h->icp_cor, h->trig);
    else
        hipLaunchKernelGGL(k_icp_correspond<false>, g, dim3(256), 0, st, h->scan, h->nb, h->pose, kd_view(h),
                           (float4 *)h->icp_tar, (float4 *)h->icp_cor, h->trig);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_icp_solve, dim3(1), dim3(1024), 0, st, (const float4 *)h->icp_tar, (const float4 *)h->icp_cor,
                       h->nb, with_start ? h->start : (const float *)nullptr, h->pose, h->icp_dbg);
    HIPCHK(hipGetLastError());
    return 0;
}
// The single-step ICP of the reference matches the scan, placed at the PREVIOUS frame's pose, against the map and only adds
// the resulting increment to the best particle (kernel.cu:984-990, 1081-1092): nothing in it depends on this frame's scores.
// fork: correspondences + covariance + SVD on the aux stream (after the scan upload), hidden under the score kernel;
// join: the main stream waits for it; the increment is then added by k_weight_final / k_icp_apply.
static int fork_icp(pfslam_handle *h)
{
    HIPCHK(hipEventRecord(h->ev_fork, h->stream));
    // on a stream of its own: it needs the tree as the previous frame's insert left it (ev_tree), not that frame's k_cells_update,
    // which follows on the aux stream -- queued behind that, the solve started when the scan-match kernel did and its one
    // 1024-thread workgroup took 340 us instead of 33 among the 131 k single-wave workgroups
    // (only when the cell rows are in use: without a k_cells_update behind the insert the aux stream is free in time, and the extra
    // cross-stream hop costs the launch-bound frame of a small particle count 15 us: 0.187 vs 0.170 ms at 1000 particles)
    const bool own_now = h->cells_valid;
    hipStream_t st = own_now ? h->istream : h->aux;
    HIPCHK(hipStreamWaitEvent(st, h->ev_fork, 0));
    if (own_now && h->tree_event) HIPCHK(hipStreamWaitEvent(st, h->ev_tree, 0));
    h->tree_event = false;
    CHK(launch_icp(h, st, false));
    // two more nodes that do not depend on the scores leave the chain behind the score kernel: the mask memset of the map
    // update -- only when the last map update did not leave the masks clean (k_scatter_cells wipes them) -- and the reset of
    // the min/max keys (both are only touched again after the join)
    if (!h->masks_cleared) HIPCHK(hipMemsetAsync(h->free_mask, 0, mask_bytes(h), st));
    CHK(launch_stats_reset(h, st));
    HIPCHK(hipEventRecord(h->ev_join, st));
    h->icp_forked = true;
    h->icp_delta_ready = false;
    return 0;
}
static int join_icp(pfslam_handle *h)
{
    HIPCHK(hipStreamWaitEvent(h->stream, h->ev_join, 0));
    h->icp_forked = false;
    h->icp_delta_ready = h->masks_cleared = h->stats_clean = true;
    return 0;
}

extern "C" int pfslam_icp(pfslam_handle *h, const float start[3], float pose_out[3], float *dbg29)
{
    if (!h) return fail("null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    CHK(settle_staged(h));
    if (start) {
        float s4[4] = {start[0], start[1], start[2], 0.0f};
        HIPCHK(hipMemcpyAsync(h->start, s4, 16, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    if (!start && h->icp_delta_ready) { // the solve already ran under the score kernel (pfslam_shard_begin): add its increment
        hipLaunchKernelGGL(k_icp_apply, dim3(1), dim3(64), 0, h->stream, h->start, h->icp_dbg, h->pose);
        HIPCHK(hipGetLastError());
    } else {
        CHK(launch_icp(h));
    }
    h->icp_delta_ready = false;
    if (pose_out || dbg29) {
        float p4[4], dbg[32];
        HIPCHK(hipMemcpyAsync(p4, h->pose, 16, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(dbg, h->icp_dbg, 32 * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (pose_out) memcpy(pose_out, p4, 12);
        if (dbg29) memcpy(dbg29, dbg, 29 * 4);
        memcpy(h->h_pose, p4, 12);
    }
    return 0;
}

// ---- point-cloud map update ----------------------------------------------------------------
static int launch_walls_and_lists(pfslam_handle *h, hipStream_t st, int cx, int cy, int centre_from_pose = 0)
{
    if (!h->masks_cleared) HIPCHK(hipMemsetAsync(h->free_mask, 0, mask_bytes(h), st)); // free + wall masks
    h->masks_cleared = false;
    hipLaunchKernelGGL(k_get_walls, dim3((h->nb + 3) / 4), dim3(256), 0, st, h->scan, h->nb, h->pose, cx, cy,
                       h->free_mask, h->wall_mask, h->dimx, h->dimy, h->cfg.map_res_x, h->cfg.map_res_y, centre_from_pose,
                       PoseSrc{nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 1, 0}, h->trig);
    HIPCHK(hipGetLastError());
    return 0;
}
static int launch_lists(pfslam_handle *h, hipStream_t st, bool clear_masks)
{
    const int M = h->dimx * h->dimy;
    const int nblk = (M + 4095) / 4096;
    hipLaunchKernelGGL(k_count_cells, dim3(nblk), dim3(256), 0, st, h->free_mask, h->wall_mask, M, h->blk_cnt);
    hipLaunchKernelGGL(k_scatter_cells, dim3(nblk), dim3(256), 0, st, h->free_mask, h->wall_mask, M, h->blk_cnt, h->counts,
                       h->dimx, h->cfg.map_res_x, h->cfg.map_res_y, h->cfg.map_scale_x, h->cfg.map_scale_y, h->pose,
                       h->wall_cell, h->wall_pts, h->max_wall, h->free_cell, h->free_pts, h->max_free, clear_masks ? 1 : 0);
    HIPCHK(hipGetLastError());
    if (clear_masks) h->masks_cleared = true; // stream-ordered in front of the next k_get_walls (same stream, or behind join_map)
    return 0;
}

// ---- frame pipeline: headers, tickets, settling --------------------------------------------------
static HostHeader *header_dev(pfslam_handle *h, int seq) { return h->hdr_dev + (seq % PF_HDR_SLOTS); }

// Wait for the header frame `seq` wrote.  The device stores the sequence word last, after a system-scope fence, into coherent
// pinned memory, so the host polls it (a stream synchronisation would also wait for the frames enqueued BEHIND it, which is
// exactly what the pipeline avoids); the stream is queried now and then so that a device fault cannot hang the caller.
static int wait_header(pfslam_handle *h, int seq, const HostHeader **out, bool two_parts = false)
{
    volatile HostHeader *hd = h->h_hdr + (seq % PF_HDR_SLOTS);
    auto last = std::chrono::steady_clock::now();
    auto there = [&]() { // (a round-5 frame's header comes in two parts, from two streams)
        return __atomic_load_n((const int32_t *)&hd->seq, __ATOMIC_ACQUIRE) == seq &&
               (!two_parts || __atomic_load_n((const int32_t *)&hd->seq2, __ATOMIC_ACQUIRE) == seq);
    };
    for (unsigned spin = 1;; spin++) {
        if (there()) break;
        __builtin_ia32_pause();
        if ((spin & 0xfff) == 0) {
            const auto now = std::chrono::steady_clock::now();
            if (now - last > std::chrono::milliseconds(2)) {
                last = now;
                // the header is written on the aux stream when the map update was forked there: both streams count
                hipError_t q = hipStreamQuery(h->stream);
                if (q == hipSuccess) q = hipStreamQuery(h->aux);
                if (q == hipSuccess) q = hipStreamQuery(h->istream);
                if (q == hipSuccess) q = hipStreamQuery(h->cstream);
                if (q == hipSuccess) { // everything enqueued has run: the header is there, or it never will be
                    if (there()) break;
                    return fail("frame header missing after the streams drained");
                }
                if (q != hipErrorNotReady) return fail(std::string("device error while waiting for a frame: ") + hipGetErrorString(q));
            }
        }
    }
    *out = (const HostHeader *)hd;
    return 0;
}

static int frame_topology(pfslam_handle *h, hipStream_t st);
// host bookkeeping of one finished frame: trace, pose, map size, deferred errors
static int consume_frame(pfslam_handle *h)
{
    const pfslam_handle::Frame f = h->in_flight.front();
    h->in_flight.pop_front();
    const HostHeader *hdr = nullptr;
    CHK(wait_header(h, f.seq, &hdr, f.v2));
    memset(h->trace, 0, sizeof(h->trace));
    h->trace[0] = (int)(0xFFFFFFFFu - (uint32_t)(hdr->stats[0] & 0xFFFFFFFFll));
    h->trace[1] = ((double)hdr->neff < PF_EFFECTIVE_PARTICLES * h->gn) ? 1 : 0; // the predicate the device gated the resample on
    memcpy(&h->trace[5], &hdr->neff, 4);
    memcpy(h->h_pose, hdr->pose, 12);
    if (std::isfinite(hdr->cloud_sigma)) h->cloud_sigma = hdr->cloud_sigma; // how the next scoring pass is organised (launch_score)
    if (f.boxes && hdr->theta_max > 0.0f) { // the device's own maximum of |heading| (k_group_box): replaces the host's running bound
        if (f.seq > h->theta_shift_seq) h->theta_shift = 0.0f; // the frame was enqueued behind the last odometry shift: it has seen it
        h->theta_bound = hdr->theta_max + 1.0f + h->theta_shift;
        // a sharded job's bound must cover the OTHER shards' particles too (the resample imports them): only a header with the job-wide
        // maximum (round-5 sharded frames, k_theta_gmax) lifts the guard
        if (h->world > 1) h->theta_global_known = f.gtheta;
    }
    if (f.kind == 0) {
        h->trace[2] = hdr->n_wall;
        h->trace[3] = hdr->n_free;
        // what the device did is booked BEFORE a deferred error is reported: after a cell list overflow the (truncated) lists were
        // still applied and their new walls inserted, so the host's map size must follow the device's.  Frames enqueued behind the
        // failed one have already run against that map.
        h->trace[4] = (hdr->flags & PF_HDR_KD_FULL) ? 0 : hdr->n_new;
        h->kd_size = hdr->kd_size;
        h->trace[6] = h->kd_size;
        if ((hdr->flags & (PF_HDR_CELLS_WIPE | PF_HDR_CELLS_FULL)) && f.seq >= h->cells_wipe_seq) {
            h->cells_wipe_pending = true; // before the next scoring pass
            // The list / pool fills when the cloud is so wide that its beam ends cover more lattice cells than there are records (a
            // 1 m cloud: millions): wiping every few frames would rebuild the same overfull table over and over.  A second overflow
            // whose frame NUMBER -- the caller's, not a count of frames -- differs from the first one's and is at most 16 above it (a
            // lower or far lower number passes this test too): the scan-match kernel goes back to the round-2 plan until the map is
            // replaced or re-balanced (upload_tree).  Numbers more than 16 apart never suspend, however many frames overflow.
            if (hdr->flags & PF_HDR_CELLS_FULL) {
                if (h->cells_full_frame >= 0 && f.frame - h->cells_full_frame <= 16 && f.frame != h->cells_full_frame) h->cells_suspended = true;
                h->cells_full_frame = f.frame;
            }
        }
        if (hdr->n_wall > h->max_wall || hdr->n_free > h->max_free) return fail("map update: cell list overflow");
        if (h->gate_err && __atomic_load_n(h->gate_err, __ATOMIC_ACQUIRE) != 0)
            return fail("a stream gate of frame ticket " + std::to_string(*h->gate_err) + " gave up waiting after 1 s (two of the handle's streams on one hardware queue, or a multi-GPU peer that never arrived). "
                        "The launches behind that gate ran without what they waited for: map, weights and particles of this handle are no longer the "
                        "reference's -- discard the handle (the error is sticky: every later frame reports it too)");
        if (hdr->flags & PF_HDR_INTERNAL) return fail("map update: the wall lists of the insert chain and of the free-cell chain differ (internal error, frame " + std::to_string(f.frame) + ")");
        // The reference appends into a static array of KD_MAX_SIZE nodes without a bound check (kernel.cu:79, 1515).  Here a
        // full map is an error, not a silent truncation: nothing was inserted (the weight updates of the frame have been
        // applied; the caller decides whether to re-create the handle with a larger kd_capacity).
        if (hdr->flags & PF_HDR_KD_FULL)
            return fail("map update: kd_capacity exhausted (" + std::to_string(hdr->kd_size) + " nodes + " + std::to_string(hdr->n_new) +
                        " new walls > " + std::to_string(h->kd_cap) + ", frame " + std::to_string(f.frame) + ")");
        // //UpdateTopology(); //CheckLoopClosure(); (kernel.cu:1750-1751) booked with the frame: the pose is the header's, the
        // visibility counts run on a stream of their own (frames enqueued behind this one keep running)
        if (h->topo_in_step == 2) CHK(frame_topology(h, h->topo_stream));
    }
    return 0;
}
// every entry point but the step functions starts here: the frames in flight are finished and booked first
static int settle(pfslam_handle *h)
{
    int rc = join_map(h);
    {
        const int r = join_all(h);
        if (r && !rc) rc = r;
    }
    while (!h->in_flight.empty()) {
        const int r = consume_frame(h);
        if (r && !rc) rc = r;
    }
    return rc;
}

// The staged calls (one phase at a time, for the host layer's debugging and the stage tests) work on the handle's stream with the
// round-4 kernels: behind round-5 frames they leave that loop first -- the next pfslam_step starts its frame ring over.
static int settle_staged(pfslam_handle *h)
{
    CHK(settle(h));
    if (h->pipe_live) {
        HIPCHK(hipStreamSynchronize(h->stream));
        h->pipe_live = false;
    }
    return 0;
}

// The map update of frame t only feeds the NEXT frame's scan-match (and ICP), so pfslam_step lets it
// run on the aux stream, beside the resample chain of frame t and the dispersion / lane order of frame t + 1; the main stream
// picks the map up again right before it plans the next scoring pass (join_map).
static int join_map(pfslam_handle *h)
{
    if (!h->map_forked) return 0;
    // (the scan-match kernel of a frame loop runs on the aux stream itself -- launch_score points h->stream there --: stream order, and an
    // event wait less in front of the kernel the whole frame waits for)
    if (h->stream != h->aux) HIPCHK(hipStreamWaitEvent(h->stream, h->ev_map, 0));
    h->map_forked = false;
    return 0;
}

// device part of PFUpdateMapKD when a map exists: lists, correspondences, weight updates, new walls tested, compacted and
// INSERTED (k_test_new).  hdr_seq > 0: the same kernel also writes the frame's header.  fork: see join_map.
// part: 0 = the whole chain; 1 = up to the traversal of the lists (needs the pose only); 2 = k_test_new (its header also needs
// the weight sums of the frame: a forked chain waits for the main stream once more in between)
static int launch_map_update_device(pfslam_handle *h, int hdr_seq = 0, bool fork = false, int part = 0)
{
    // centre of the local grid (kernel.cu:1408-1411)
    const int cx = (int)roundf(0.5f * h->dimx + h->cfg.map_res_x / 2), cy = (int)roundf(0.5f * h->dimy + h->cfg.map_res_y / 2);
    hipStream_t st = h->stream;
    if (fork && h->kd_size > 0) {
        if (!(h->scored_on_aux && part == 1)) { // (the scan-match kernel ran on the aux stream: the pose is there already)
            HIPCHK(hipEventRecord(h->ev_mapfork, h->stream));
            HIPCHK(hipStreamWaitEvent(h->aux, h->ev_mapfork, 0));
        }
        st = h->aux;
    }
    if (part != 2) {
        CHK(launch_walls_and_lists(h, st, cx, cy)); // reads the frame's own scan slot: the next frame's upload goes elsewhere
        CHK(launch_lists(h, st, /*clear_masks=*/true));
        h->header_packed = false;
    }
    if (h->kd_size > 0) {
        const pf::KdView tv = kd_view(h);
        const dim3 gf(1024);
        if (part != 2) {
            if (h->planar)
                hipLaunchKernelGGL(k_list_traverse<true>, gf, dim3(256), 0, st, h->free_pts, h->free_c, h->max_free,
                                   (const float4 *)h->wall_pts, h->wall_c, h->max_wall, (const int *)h->counts, tv, h->cfg.free_upload_bug,
                                   h->wall_leaf, h->kw, h->cfg.map_res_x, h->cfg.map_res_y);
            else
                hipLaunchKernelGGL(k_list_traverse<false>, gf, dim3(256), 0, st, h->free_pts, h->free_c, h->max_free,
                                   (const float4 *)h->wall_pts, h->wall_c, h->max_wall, (const int *)h->counts, tv, h->cfg.free_upload_bug,
                                   h->wall_leaf, h->kw, h->cfg.map_res_x, h->cfg.map_res_y);
        }
        HIPCHK(hipGetLastError());
        if (part == 1) return 0;
        const size_t lds = (size_t)h->max_wall * 8 * sizeof(uint32_t); // the frame's new walls as LDS-resident nodes
        if (lds > 48 * 1024 && !h->lds_attr_set) {
            HIPCHK(hipFuncSetAttribute((const void *)k_test_new, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            h->lds_attr_set = true;
        }
        if (h->walk_pending) { // the walks of this frame's new lattice cells read the tree this kernel appends to
            HIPCHK(hipStreamWaitEvent(st, h->ev_walked, 0));
            h->walk_pending = false;
        }
        hipLaunchKernelGGL(k_test_new, dim3(1), dim3(1024), lds, st, (const float4 *)h->wall_pts, (const int *)h->wall_c,
                           (const int *)h->wall_leaf, h->counts, h->max_wall, tv, h->cfg.map_res_x, h->cfg.map_res_y, h->hot, h->parent,
                           h->kz, h->kw, h->kd_state, h->kd_cap, (const float *)h->sums, (const long long *)h->stats,
                           (const float *)h->pose, hdr_seq > 0 ? header_dev(h, hdr_seq) : (HostHeader *)nullptr, hdr_seq,
                           (h->cell_tab && !h->cells_wipe_pending) ? (const int *)h->cell_state : (const int *)nullptr,
                           (h->cell_tab && !h->cells_wipe_pending) ? h->cell_touched : (int *)nullptr, (const float *)h->d_sigma);
        HIPCHK(hipGetLastError());
        if (st != h->stream) { // the next frame's ICP solve may start here
            HIPCHK(hipEventRecord(h->ev_tree, st));
            h->tree_event = true;
        }
        CHK(launch_cells_update(h, st)); // the persistent cell rows follow the insert (kd_cells.hip.inc)
        h->pipe_live = false; // (an insert by the round-4 chain: the tree-size words of the round-5 frame ring are stale)
        h->header_packed = hdr_seq > 0;
        h->mirror_stale = true; // links (and, past mirror_n, nodes) of the host mirror are behind the device now
        if (st != h->stream) {
            HIPCHK(hipEventRecord(h->ev_map, st));
            h->map_forked = true;
        }
    }
    return 0;
}
// the header on its own (first scan, 2-D frame, sharded frame); after_kd_update: n_new and flags of this frame's k_test_new
static int launch_header(pfslam_handle *h, int seq, bool after_kd_update)
{
    hipLaunchKernelGGL(k_pack_header, dim3(1), dim3(64), 0, h->stream, (const int *)h->counts, (const int *)h->kd_state,
                       (const float *)h->sums, (const long long *)h->stats, (const float *)h->pose, header_dev(h, seq),
                       after_kd_update ? 1 : 0, seq, (const float *)h->d_sigma);
    HIPCHK(hipGetLastError());
    return 0;
}

// First scan: the wall list itself seeds the map, KDTree::Create(wallPC) on the host (kernel.cu:1532-1536).  Synchronous.
static int seed_map_from_walls(pfslam_handle *h)
{
    const int seq = ++h->seq;
    CHK(launch_header(h, seq, false));
    const HostHeader *hdr = nullptr;
    CHK(wait_header(h, seq, &hdr));
    if (hdr->n_wall > h->max_wall || hdr->n_free > h->max_free) return fail("map update: cell list overflow");
    memset(h->trace, 0, sizeof(h->trace));
    h->trace[0] = -1;
    h->trace[2] = hdr->n_wall;
    h->trace[3] = hdr->n_free;
    memcpy(h->h_pose, hdr->pose, 12);
    if (hdr->n_wall > 0) {
        if (hdr->n_wall > h->kd_cap) return fail("map update: kd_capacity too small for the first scan");
        std::vector<float> pts((size_t)hdr->n_wall * 4);
        HIPCHK(hipMemcpyAsync(pts.data(), h->wall_pts, pts.size() * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        std::vector<pfslam_node> nodes((size_t)hdr->n_wall);
        if (pfslam_kd_create(pts.data(), hdr->n_wall, nodes.data())) return fail("kd_create failed");
        CHK(upload_tree(h, nodes.data(), hdr->n_wall));
    }
    h->trace[6] = h->kd_size;
    return 0;
}

// map update as a stage: device chain, then the frame is settled at once
static int map_update_and_settle(pfslam_handle *h)
{
    if (h->kd_size == 0) {
        CHK(launch_map_update_device(h));
        return seed_map_from_walls(h);
    }
    const int seq = ++h->seq;
    CHK(launch_map_update_device(h, seq));
    h->in_flight.push_back(pfslam_handle::Frame{seq, -1, 0});
    int keep[8];
    memcpy(keep, h->trace, sizeof(keep));
    CHK(settle(h));
    h->trace[0] = keep[0]; h->trace[1] = keep[1]; h->trace[5] = keep[5]; // the stage did not touch best / resampled / Neff
    return 0;
}

extern "C" int pfslam_update_map_kd(pfslam_handle *h)
{
    if (!h) return fail("null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    CHK(settle_staged(h));
    return map_update_and_settle(h);
}

extern "C" int pfslam_get_cells(pfslam_handle *h, int which, int32_t *out, int cap, int *n)
{
    if (!h || !out || !n || (which != 0 && which != 1)) return fail("pfslam_get_cells: bad argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    CHK(settle(h));
    const int cnt = h->trace[2 + which];
    *n = cnt;
    const int m = std::min(cnt, cap);
    if (m > 0) {
        HIPCHK(hipMemcpyAsync(out, which == 0 ? h->wall_cell : h->free_cell, (size_t)m * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return 0;
}

// ---- resample --------------------------------------------------------------------------------
// All resample arithmetic runs on the GLOBAL weight array (gw, gn entries) so that sums, cdf and
// sampled indices do not depend on how the particles are sharded; unsharded handles alias gw = w.
static const float *global_w(const pfslam_handle *h) { return h->gw; }
static int launch_weight_sums(pfslam_handle *h, bool apply_icp = false)
{
    const int nt = (h->gn + PF_SUM_TILE - 1) / PF_SUM_TILE;
    hipLaunchKernelGGL(k_weight_tiles, dim3(nt), dim3(64), 0, h->stream, global_w(h), h->gn, h->tile_r, h->tile_r2);
    hipLaunchKernelGGL(k_weight_final, dim3(1), dim3(64), 0, h->stream, h->tile_r, h->tile_r2, nt, h->gn, h->sums,
                       apply_icp ? h->start : (const float *)nullptr, h->icp_dbg, h->pose);
    HIPCHK(hipGetLastError());
    return 0;
}
static void swap_pose_blocks(pfslam_handle *h)
{
    std::swap(h->pblk, h->pblk2);
    std::swap(h->x, h->x2);
    std::swap(h->y, h->y2);
    std::swap(h->th, h->th2);
    if (!h->own_global) h->gpose = h->pblk;
}
// gated: the kernels decide on the device whether the frame resamples (frame loops); otherwise the caller has decided
// frame loops above one sum tile: weight sums + Neff (+ ICP increment) and the first two passes of the scan in two launches
static int launch_weight_sums_with_scan_front(pfslam_handle *h, bool apply_icp)
{
    // on the global weight array (gw aliases w when the handle is not sharded)
    const int nts = (h->gn + PF_SUM_TILE - 1) / PF_SUM_TILE, nt = (h->gn + PF_SCAN_TILE - 1) / PF_SCAN_TILE;
    hipLaunchKernelGGL(k_weight_scan_tiles, dim3(nts), dim3(256), 0, h->stream, global_w(h), h->gn, h->tile_r, h->tile_r2, h->tile_tot);
    hipLaunchKernelGGL(k_weight_final_offsets, dim3(1), dim3(64), 0, h->stream, (const float *)h->tile_r, (const float *)h->tile_r2, nts,
                       h->gn, h->sums, apply_icp ? (const float *)h->start : (const float *)nullptr, (const float *)h->icp_dbg, h->pose,
                       (const float *)h->tile_tot, nt, h->tile_off, PF_EFFECTIVE_PARTICLES * h->gn);
    HIPCHK(hipGetLastError());
    h->scan_front_done = true;
    return 0;
}
static int launch_resample_plan(pfslam_handle *h, int frame, bool gated = false, bool with_sample = true)
{
    const int gn = h->gn, n = h->n, nt = (gn + PF_SCAN_TILE - 1) / PF_SCAN_TILE;
    const float *gw = global_w(h);
    const float *gate = gated ? (const float *)h->sums : (const float *)nullptr;
    const double thr = PF_EFFECTIVE_PARTICLES * h->gn;
    hipLaunchKernelGGL(k_scan_tiles, dim3(nt), dim3(64), 0, h->stream, gw, gn, h->tile_tot, gate, thr);
    hipLaunchKernelGGL(k_scan_offsets, dim3(1), dim3(64), 0, h->stream, h->tile_tot, nt, h->tile_off, gate, thr);
    hipLaunchKernelGGL(k_scan_apply, dim3(nt), dim3(64), 0, h->stream, gw, gn, h->tile_off, h->cdf, h->chunk_max, h->tile_pmax, gate, thr);
    hipLaunchKernelGGL(k_scan_pmax, dim3(1), dim3(64), 0, h->stream, h->tile_pmax, nt, gate, thr);
    if (with_sample)
        hipLaunchKernelGGL(k_sample, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->cdf, h->chunk_max, h->tile_pmax, gn, n, h->goff,
                           frame, h->sums, h->src, gate, thr, h->resampler);
    HIPCHK(hipGetLastError());
    return 0;
}
static int launch_resample_gather(pfslam_handle *h)
{
    const int n = h->n;
    hipLaunchKernelGGL(k_gather, dim3((n + 255) / 256), dim3(256), 0, h->stream, (const float *)h->gpose, h->stride, h->src, n,
                       h->x2, h->y2, h->th2, h->w, h->wm);
    HIPCHK(hipGetLastError());
    swap_pose_blocks(h);
    return 0;
}
static int launch_resample(pfslam_handle *h, int frame, bool gated = false)
{
    if (gated && !h->own_global && h->n <= 4 * PF_SCAN_TILE) { // the reference's own sizes: one workgroup, one launch
        hipLaunchKernelGGL(k_resample_small, dim3(1), dim3(1024), 0, h->stream, (const float *)h->w, h->n, h->cdf, h->chunk_max,
                           h->tile_pmax, frame, (const float *)h->sums, h->src, (const float *)h->pblk, h->pblk2, h->stride, h->w,
                           h->wm, PF_EFFECTIVE_PARTICLES * h->gn, h->resampler);
        HIPCHK(hipGetLastError());
        swap_pose_blocks(h);
        return 0;
    }
    if (gated) { // frame loops: the scan's first two passes rode along with the weight sums; everything on the GLOBAL weights
        const int n = h->n, gn = h->gn, nt = (gn + PF_SCAN_TILE - 1) / PF_SCAN_TILE;
        const double thr = PF_EFFECTIVE_PARTICLES * h->gn;
        const bool local_pmax = nt <= PF_PMAX_LDS;
        if (!h->scan_front_done) { // all four scan passes; above 4 M particles also when the front passes are done: k_scan_pmax
            CHK(launch_resample_plan(h, frame, true, /*with_sample=*/false));
        } else {
            hipLaunchKernelGGL(k_scan_apply, dim3(nt), dim3(64), 0, h->stream, global_w(h), gn, h->tile_off, h->cdf, h->chunk_max,
                               h->tile_pmax, (const float *)h->sums, thr);
            if (!local_pmax) hipLaunchKernelGGL(k_scan_pmax, dim3(1), dim3(64), 0, h->stream, h->tile_pmax, nt, (const float *)h->sums, thr);
        }
        h->scan_front_done = false;
        const dim3 g((n + 255) / 256);
#define PF_SG_ARGS (const float *)h->cdf, (const float *)h->chunk_max, (const float *)h->tile_pmax, gn, n, h->goff, frame, (const float *)h->sums, \
                   h->src, (const float *)h->gpose, h->pblk2, h->stride, h->w, h->wm, thr, h->resampler
        if (h->own_global) { // sources come from the all-gathered pose blocks of every rank
            if (local_pmax) hipLaunchKernelGGL((k_sample_gather<true, true>), g, dim3(256), 0, h->stream, PF_SG_ARGS);
            else hipLaunchKernelGGL((k_sample_gather<false, true>), g, dim3(256), 0, h->stream, PF_SG_ARGS);
        } else {
            if (local_pmax) hipLaunchKernelGGL((k_sample_gather<true, false>), g, dim3(256), 0, h->stream, PF_SG_ARGS);
            else hipLaunchKernelGGL((k_sample_gather<false, false>), g, dim3(256), 0, h->stream, PF_SG_ARGS);
        }
#undef PF_SG_ARGS
        HIPCHK(hipGetLastError());
        swap_pose_blocks(h);
        return 0;
    }
    CHK(launch_resample_plan(h, frame, gated));
    return launch_resample_gather(h);
}

// Neff on the global weights and, when it is below 0.7 N (kernel.cu:474), the cdf + source indices of this
// handle's slots.  Sharded callers all-gather the weights into buffer 10 before, and the poses into
// buffers 11-13 between this call and pfslam_resample_gather.
extern "C" int pfslam_resample_plan(pfslam_handle *h, int frame, int *resampled, float *neff)
{
    if (!h) return fail("null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    CHK(settle_staged(h));
    CHK(launch_weight_sums(h));
    float s[4];
    HIPCHK(hipMemcpyAsync(s, h->sums, 12, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const bool doit = (double)s[2] < PF_EFFECTIVE_PARTICLES * h->gn;
    if (doit) CHK(launch_resample_plan(h, frame));
    if (resampled) *resampled = doit ? 1 : 0;
    if (neff) *neff = s[2];
    h->trace[1] = doit ? 1 : 0;
    memcpy(&h->trace[5], &s[2], 4);
    return 0;
}
extern "C" int pfslam_resample_gather(pfslam_handle *h)
{
    if (!h) return fail("null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    return launch_resample_gather(h);
}

extern "C" int pfslam_resample(pfslam_handle *h, int frame, int *resampled, float *neff)
{
    if (!h) return fail("null handle");
    if (h->own_global) return fail("pfslam_resample: sharded handles use pfslam_resample_plan / _gather around the caller's all-gathers");
    int did = 0;
    CHK(pfslam_resample_plan(h, frame, &did, neff));
    if (did) CHK(launch_resample_gather(h));
    if (resampled) *resampled = did;
    return 0;
}

// ------------------------------------------------------------------------------------------
// pfslam_estimate: weighted mean pose and 3x3 covariance of the cloud (no reference counterpart; specification in include/pfslam.h).
// Every sum is the canonical one over GLOBAL particle indices: tile t holds the particles [t * 4096, min((t + 1) * 4096, gn)) whatever
// the sharding, its eleven sums are one wave each (wave_sum_canonical out of LDS), and the tile sums are summed the same way.
//   part[q * nt + t], q = 0 w, 1 w*w, 2 w*x, 3 w*y, 4 w*theta (pass A), 5 .. 10 xx, xy, xtheta, yy, ytheta, thetatheta (pass B)
// Particle g of the rank-major buffers: weight gw[g]; pose in block g / stride at g % stride ([x | y | theta], stride floats each).
// ------------------------------------------------------------------------------------------
// ESTIMATE-DEVICE-KERNEL-TEXT-BEGIN
#define PF_EST_WAVES 6
__device__ __forceinline__ void est_stage(float (*s)[PF_SUM_TILE], const float *gw, const float *gpose, int stride, int g0, int cnt)
{
    for (int i = threadIdx.x; i < cnt; i += PF_EST_WAVES * 64) {
        const int g = g0 + i;
        const int r = g / stride, j = g - r * stride;
        const float *blk = gpose + (size_t)r * 3 * stride;
        s[0][i] = gw[g];
        s[1][i] = blk[j];
        s[2][i] = blk[(size_t)stride + j];
        s[3][i] = blk[2 * (size_t)stride + j];
    }
}
// wave q < 5 of the workgroup: its quantity's sum over the staged tile -> part[q * nt + t]
__device__ __forceinline__ void est_moments(const float (*s)[PF_SUM_TILE], int cnt, float *part, int nt, int t)
{
    const int q = threadIdx.x >> 6;
    if (q >= 5) return;
    const float *p = s[q < 2 ? 0 : q - 1];
    const float v = q == 0 ? wave_sum_canonical(cnt, [&](int i) { return s[0][i]; })
                           : wave_sum_canonical(cnt, [&](int i) { return s[0][i] * p[i]; });
    if ((threadIdx.x & 63) == 0) part[q * nt + t] = v;
}
// S0 and the three means from pass A's tile sums: the canonical sum gives every wave of every workgroup the same bits
__device__ __forceinline__ void est_means(const float *part, int nt, float *s0, float m[3])
{
    *s0 = wave_sum_canonical(nt, [&](int i) { return part[i]; });
    for (int k = 0; k < 3; k++) m[k] = pf::fdiv(wave_sum_canonical(nt, [&](int i) { return part[(2 + k) * nt + i]; }), *s0);
}
// the staged poses become deviations d = p - m (each element once), then wave q: sum of (w * d_k) * d_l -> cen[q * nt + t]
__device__ __forceinline__ void est_centred(float (*s)[PF_SUM_TILE], int cnt, const float m[3], float *cen, int nt, int t)
{
    for (int i = threadIdx.x; i < cnt; i += PF_EST_WAVES * 64) {
        s[1][i] = s[1][i] - m[0];
        s[2][i] = s[2][i] - m[1];
        s[3][i] = s[3][i] - m[2];
    }
    __syncthreads();
    const int q = threadIdx.x >> 6; // xx, xy, xtheta, yy, ytheta, thetatheta
    const int k = q < 3 ? 0 : (q < 5 ? 1 : 2), l = q < 3 ? q : (q < 5 ? q - 2 : 2);
    const float *dk = s[1 + k], *dl = s[1 + l];
    const float v = wave_sum_canonical(cnt, [&](int i) { return (s[0][i] * dk[i]) * dl[i]; });
    if ((threadIdx.x & 63) == 0) cen[q * nt + t] = v;
}
// the 16 output floats from the tile sums (first wave of the workgroup)
__device__ __forceinline__ void est_finish(const float *part, int nt, int gn, float *out)
{
    if (threadIdx.x >= 64) return;
    float s0, m[3], c[6];
    est_means(part, nt, &s0, m);
    const float s2 = wave_sum_canonical(nt, [&](int i) { return part[nt + i]; });
    for (int q = 0; q < 6; q++) c[q] = pf::fdiv(wave_sum_canonical(nt, [&](int i) { return part[(5 + q) * nt + i]; }), s0);
    if (threadIdx.x != 0) return;
    for (int k = 0; k < 3; k++) out[k] = m[k];
    for (int q = 0; q < 6; q++) out[3 + q] = c[q];
    out[9] = pf::fdiv(s0 * s0, s2);
    out[10] = s0;
    out[11] = s2;
    out[12] = (float)gn;
    out[13] = out[14] = out[15] = 0.0f;
}
// ESTIMATE-DEVICE-KERNEL-TEXT-END
// ESTIMATE-KERNEL-TEXT-BEGIN
__global__ __launch_bounds__(PF_EST_WAVES * 64) void k_estimate_moments(const float *__restrict__ gw, const float *__restrict__ gpose,
                                                                        int stride, int gn, float *__restrict__ part, int nt)
{
    __shared__ float s[4][PF_SUM_TILE];
    const int t = blockIdx.x, cnt = min(PF_SUM_TILE, gn - t * PF_SUM_TILE);
    est_stage(s, gw, gpose, stride, t * PF_SUM_TILE, cnt);
    __syncthreads();
    est_moments(s, cnt, part, nt, t);
}
// pass A's sums are complete (stream order): `mom` = part[0 .. 5 nt) is read-only here, `cen` = part + 5 nt is written
__global__ __launch_bounds__(PF_EST_WAVES * 64) void k_estimate_centred(const float *__restrict__ gw, const float *__restrict__ gpose,
                                                                        int stride, int gn, const float *__restrict__ mom,
                                                                        float *__restrict__ cen, int nt)
{
    __shared__ float s[4][PF_SUM_TILE];
    const int t = blockIdx.x, cnt = min(PF_SUM_TILE, gn - t * PF_SUM_TILE);
    est_stage(s, gw, gpose, stride, t * PF_SUM_TILE, cnt);
    float s0, m[3];
    est_means(mom, nt, &s0, m);
    __syncthreads();
    est_centred(s, cnt, m, cen, nt, t);
}
__global__ __launch_bounds__(64) void k_estimate_final(const float *__restrict__ part, int nt, int gn, float *__restrict__ out)
{
    est_finish(part, nt, gn, out);
}
// up to one tile: the three passes as one workgroup.  The tile sums cross from wave to wave through `part` in global memory, a barrier
// between writer and readers (not __restrict__: the loads must not be taken for loads of kernel-invariant memory).
__global__ __launch_bounds__(PF_EST_WAVES * 64) void k_estimate_small(const float *gw, const float *gpose, int stride, int gn, float *part,
                                                                      float *out)
{
    __shared__ float s[4][PF_SUM_TILE];
    est_stage(s, gw, gpose, stride, 0, gn);
    __syncthreads();
    est_moments(s, gn, part, 1, 0);
    __syncthreads();
    float s0, m[3];
    est_means(part, 1, &s0, m);
    est_centred(s, gn, m, part + 5, 1, 0);
    __syncthreads();
    est_finish(part, 1, gn, out);
}

// ESTIMATE-KERNEL-TEXT-END
extern "C" int pfslam_estimate(pfslam_handle *h, float out[16])
{
    if (!h || !out) return fail("pfslam_estimate: bad argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    CHK(settle(h));
    if (!h->est_part) return fail("pfslam_estimate: more than 4096 * 4096 particles (the tile sums of the canonical sum must fit one tile)");
    const int gn = h->gn, nt = (gn + PF_SUM_TILE - 1) / PF_SUM_TILE;
    float *part = h->est_part, *res = h->est_part + (size_t)11 * nt;
    const dim3 wg(PF_EST_WAVES * 64);
    if (nt == 1) {
        hipLaunchKernelGGL(k_estimate_small, dim3(1), wg, 0, h->stream, (const float *)h->gw, (const float *)h->gpose, h->stride, gn, part, res);
    } else {
        hipLaunchKernelGGL(k_estimate_moments, dim3(nt), wg, 0, h->stream, (const float *)h->gw, (const float *)h->gpose, h->stride, gn, part, nt);
        hipLaunchKernelGGL(k_estimate_centred, dim3(nt), wg, 0, h->stream, (const float *)h->gw, (const float *)h->gpose, h->stride, gn,
                           (const float *)part, part + (size_t)5 * nt, nt);
        hipLaunchKernelGGL(k_estimate_final, dim3(1), dim3(64), 0, h->stream, (const float *)part, nt, gn, res);
    }
    HIPCHK(hipGetLastError());
    float r[16];
    HIPCHK(hipMemcpyAsync(r, res, sizeof(r), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (!(r[10] > 0.0f) || !std::isfinite(r[10])) {
        char msg[160];
        snprintf(msg, sizeof(msg), "pfslam_estimate: the weights sum to %g (it must be finite and > 0): no mean, no covariance", (double)r[10]);
        return fail(msg);
    }
    memcpy(out, r, sizeof(r));
    return 0;
}

// ---- 2-D grid path -------------------------------------------------------------------------
extern "C" int pfslam_set_grid(pfslam_handle *h, const int8_t *grid, int dimx, int dimy)
{
    if (!h || !grid || dimx != h->dimx || dimy != h->dimy) return fail("pfslam_set_grid: grid must be dimx x dimy of the config");
    HIPCHK(hipSetDevice(h->cfg.device));
    CHK(settle_staged(h));
    HIPCHK(hipMemcpyAsync(h->grid, grid, (size_t)dimx * dimy, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}
extern "C" int pfslam_get_grid(pfslam_handle *h, const int8_t **grid, int *dimx, int *dimy)
{
    if (!h || !grid || !dimx || !dimy) return fail("pfslam_get_grid: bad argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    CHK(settle_staged(h));
    h->h_grid.resize((size_t)h->dimx * h->dimy);
    HIPCHK(hipMemcpyAsync(h->h_grid.data(), h->grid, h->h_grid.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *grid = h->h_grid.data();
    *dimx = h->dimx;
    *dimy = h->dimy;
    return 0;
}
static int score_grid_launch(pfslam_handle *h, bool with_sums = false, bool kernel_only = false)
{
    // a grid beam is ~100 instructions (no traversal): 16 k waves fill the chip, more only adds partials
    const int groups = (h->n + 63) / 64;
    const int chunks = std::max(1, std::min((16384 + groups - 1) / groups, h->nb));
    const int bpc = (h->nb + chunks - 1) / chunks, used = (h->nb + bpc - 1) / bpc;
    const size_t need = (size_t)used * h->n;
    if (need > h->partial_elems) {
        if (h->partial) HIPCHK(hipFree(h->partial));
        h->partial = nullptr;
        CHK(dalloc(&h->partial, need));
        h->partial_elems = need;
    }
    hipLaunchKernelGGL(k_score_grid, dim3((h->n + 255) / 256, used), dim3(256), 0, h->stream, h->grid, h->dimx, h->dimy,
                       h->cfg.map_scale_x, h->cfg.map_scale_y, h->cfg.map_res_x, h->cfg.map_res_y, h->x, h->y, h->th, h->n,
                       h->scan, (const pf::BeamParts *)h->beam_angle, h->nb, bpc, (int *)h->partial, h->trig);
    if (kernel_only) return 0; // pfslam_time_score_grid
    hipLaunchKernelGGL(k_reduce_partials_i32, dim3((h->n + 63) / 64), dim3(256), 0, h->stream, (const int *)h->partial, h->n,
                       used, h->fit_i);
    HIPCHK(hipGetLastError());
    // PFMeasurementUpdate (kernel.cu:307-339): int min/max/argmax + int kernUpdateWeights
    CHK(launch_minmax(h, true));
    if (with_sums && h->n <= PF_SUM_TILE) return launch_weights_small(h, true, false); // weights, sums and Neff in one launch
    CHK(launch_weights(h, true));
    return with_sums ? launch_weight_sums_with_scan_front(h, false) : 0;
}
// measurement support (bench.py extras, tools/profile_grid.sh): mean duration of k_score_grid alone and of the whole 2-D scoring pass
// (score + partial sums + int min / max / argmax + weights), HIP events on the handle's stream, `iters` launches each
extern "C" int pfslam_time_score_grid(pfslam_handle *h, int iters, float *ms_kernel, float *ms_pass)
{
    if (!h || iters <= 0 || !ms_kernel || !ms_pass) return fail("pfslam_time_score_grid: bad argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    CHK(settle_staged(h));
    // The timed pass ends in kernUpdateWeights, which multiplies the weights in place: iters + 1 of them would leave the handle with other
    // weights than it came with (tests/test_gpu_observers.py).  They and their mirror are put back behind the last pass -- also when a
    // launch of the timed passes fails.  What a scoring pass derives from particles and grid -- the integer fits, the min / max keys
    // (buffer 0) and the best particle's pose (buffer 8) -- stays as the last timed pass wrote it, as behind pfslam_score_grid.
    // (One allocation per call: a measurement helper, off every frame's path.)
    struct Keep {
        float *p = nullptr;
        ~Keep() { if (p) (void)hipFree(p); }
    } keep;
    const size_t S = (size_t)h->stride;
    CHK(dalloc(&keep.p, 2 * S));
    HIPCHK(hipMemcpyAsync(keep.p, h->w, S * 4, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(keep.p + S, h->wm, S * 4, hipMemcpyDeviceToDevice, h->stream));
    const int timed = [&]() -> int {
        CHK(score_grid_launch(h)); // warm
        for (int pass = 0; pass < 2; pass++) {
            HIPCHK(hipEventRecord(h->ev0, h->stream));
            for (int k = 0; k < iters; k++) CHK(score_grid_launch(h, false, pass == 0));
            HIPCHK(hipEventRecord(h->ev1, h->stream));
            HIPCHK(hipEventSynchronize(h->ev1));
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
            *(pass == 0 ? ms_kernel : ms_pass) = ms / iters;
        }
        return 0;
    }();
    const int restored = [&]() -> int {
        HIPCHK(hipMemcpyAsync(h->w, keep.p, S * 4, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->wm, keep.p + S, S * 4, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        return 0;
    }();
    return timed ? timed : restored;
}
extern "C" int pfslam_score_grid(pfslam_handle *h, int32_t *fit_host)
{
    if (!h) return fail("null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    CHK(settle_staged(h));
    CHK(score_grid_launch(h));
    if (fit_host) {
        HIPCHK(hipMemcpyAsync(fit_host, h->fit_i, (size_t)h->n * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return 0;
}
static int launch_update_map_grid(pfslam_handle *h)
{
    CHK(launch_walls_and_lists(h, h->stream, 0, 0, 1)); // PFUpdateMap centre (kernel.cu:552-555) from the device pose
    const int M = h->dimx * h->dimy;
    hipLaunchKernelGGL(k_update_grid, dim3((M + 255) / 256), dim3(256), 0, h->stream, M, h->grid, h->free_mask, PF_FREE_WEIGHT);
    hipLaunchKernelGGL(k_update_grid, dim3((M + 255) / 256), dim3(256), 0, h->stream, M, h->grid, h->wall_mask, PF_OCCUPIED_WEIGHT);
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int pfslam_update_map_grid(pfslam_handle *h)
{
    if (!h) return fail("null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    CHK(settle_staged(h));
    return launch_update_map_grid(h);
}

// ---- topology graph / loop-closure proposal (kernel.cu:623-795) --------------------------------
// FindWalls + CheckVisibility: the ray between two grid cells in the closed form of trace_ray_wave, one block;
// every ray cell is distinct, so the count needs no mask (the reference marks a mask, then counts map > 30 under it).
__global__ __launch_bounds__(256) void k_find_walls(const int8_t *__restrict__ grid, int dimx, int dimy, int sx, int sy, int ex,
                                                    int ey, int *__restrict__ out)
{
    const bool steep = abs(ey - sy) > abs(ex - sx);
    if (steep) {
        int t = sx; sx = sy; sy = t;
        t = ex; ex = ey; ey = t;
    }
    if (sx > ex) {
        int t = sx; sx = ex; ex = t;
        t = sy; sy = ey; ey = t;
    }
    const int deltax = ex - sx, deltay = abs(ey - sy), e0 = deltax / 2, ystep = (ey > sy) ? 1 : -1;
    int cnt = 0;
    for (int k = threadIdx.x; k < deltax; k += 256) {
        const int c = (k * deltay - e0 + deltax - 1) / deltax;
        const int xx = sx + k, yy = sy + ystep * c;
        const int idx = steep ? yy * dimx + xx : xx * dimx + yy;
        if (xx < dimx && yy < dimy && xx >= 0 && yy >= 0 && idx < dimx * dimy) cnt += grid[idx] > 30; // WALL_CONFIDENCE
    }
    for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    __shared__ int s[4];
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) *out = s[0] + s[1] + s[2] + s[3];
}

static float dist2d(float ax, float ay, float bx, float by)
{
    const float dx = bx - ax, dy = by - ay;
    return sqrtf(dx * dx + dy * dy);
}
// st: the stream the count runs on -- the handle's own, or (topology booked with the frames, pfslam_set_topology 2) a stream of
// its own that does not wait for the frames enqueued behind the one being booked
static int find_walls(pfslam_handle *h, float ax, float ay, float bx, float by, int *n_walls, hipStream_t st = nullptr)
{
    if (!st) st = h->stream;
    const float rx = h->cfg.map_res_x, ry = h->cfg.map_res_y;
    const int aix = (int)roundf(0.5f * h->dimx + ax / rx + rx / 2), aiy = (int)roundf(0.5f * h->dimy + ay / ry + ry / 2);
    const int bix = (int)roundf(0.5f * h->dimx + bx / rx + rx / 2), biy = (int)roundf(0.5f * h->dimy + by / ry + ry / 2);
    hipLaunchKernelGGL(k_find_walls, dim3(1), dim3(256), 0, st, h->grid, h->dimx, h->dimy, aix, aiy, bix, biy, h->d_count);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(n_walls, h->d_count, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}
static int refresh_host_pose(pfslam_handle *h)
{
    float p4[4];
    HIPCHK(hipMemcpyAsync(p4, h->pose, 16, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    memcpy(h->h_pose, p4, 12);
    return 0;
}

extern "C" int pfslam_find_walls(pfslam_handle *h, const float a_xy[2], const float b_xy[2], int *n_walls)
{
    if (!h || !a_xy || !b_xy || !n_walls) return fail("pfslam_find_walls: bad argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    CHK(settle(h));
    return find_walls(h, a_xy[0], a_xy[1], b_xy[0], b_xy[1], n_walls);
}

// UpdateTopology (kernel.cu:695-726) at pose (rx, ry)
static void topology_update_at(pfslam_handle *h, float rx, float ry)
{
    bool newNode = true; // farther than MAX_NODE_DIST (2.5 m) from every node
    for (const auto &nd : h->topo_nodes) newNode &= dist2d(rx, ry, nd.x, nd.y) > 2.5f;
    if (newNode) { // CreateNode, kernel.cu:623-648
        const auto &cur = h->topo_nodes[h->topo_idx];
        const float edgeLen = dist2d(rx, ry, cur.x, cur.y);
        for (auto &nd : h->topo_nodes) nd.dist += edgeLen;
        h->topo_nodes.push_back(pfslam_handle::TopoNode{rx, ry, 0.0f});
        h->topo_edges.push_back(std::vector<unsigned>{h->topo_idx});
        h->topo_edges[h->topo_idx].push_back((unsigned)h->topo_nodes.size() - 1);
        h->topo_idx = (unsigned)h->topo_nodes.size() - 1;
    }
}
// CheckLoopClosure (kernel.cu:738-795) at pose (rx, ry): pairs (candidate node j, visible node k)
static int loop_closure_at(pfslam_handle *h, float rx, float ry, std::vector<int32_t> &pairs, hipStream_t st = nullptr)
{
    pairs.clear();
    for (size_t j = 0; j < h->topo_nodes.size(); j++) {
        if (!(dist2d(rx, ry, h->topo_nodes[j].x, h->topo_nodes[j].y) < 6.0f)) continue;             // CLOSURE_MAP_DIST
        const auto &cur = h->topo_nodes[h->topo_idx];
        const float edgeLen = dist2d(rx, ry, cur.x, cur.y);
        if (!(edgeLen + h->topo_nodes[j].dist > 20.0f)) continue;                                     // CLOSURE_GRAPH_DIST
        for (size_t k = 0; k < h->topo_nodes.size(); k++) {
            int nWalls = 0;
            CHK(find_walls(h, rx, ry, h->topo_nodes[k].x, h->topo_nodes[k].y, &nWalls, st));
            if (nWalls < 2) { // MIN_WALL_COUNT: node k is visible from the robot
                pairs.push_back((int32_t)j);
                pairs.push_back((int32_t)k);
            }
        }
    }
    return 0;
}

extern "C" int pfslam_topology_update(pfslam_handle *h, int *n_nodes)
{
    if (!h) return fail("null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    CHK(settle(h));
    CHK(refresh_host_pose(h));
    topology_update_at(h, h->h_pose[0], h->h_pose[1]);
    if (n_nodes) *n_nodes = (int)h->topo_nodes.size();
    return 0;
}

extern "C" int pfslam_check_loop_closure(pfslam_handle *h, int32_t *pairs, int cap, int *n)
{
    if (!h || !n || (cap > 0 && !pairs)) return fail("pfslam_check_loop_closure: bad argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    CHK(settle(h));
    CHK(refresh_host_pose(h));
    std::vector<int32_t> found;
    CHK(loop_closure_at(h, h->h_pose[0], h->h_pose[1], found));
    const int count = (int)found.size() / 2;
    if (std::min(count, cap) > 0) memcpy(pairs, found.data(), (size_t)std::min(count, cap) * 8);
    *n = count;
    return 0;
}

// The two calls the reference leaves commented out at the end of particleFilter (kernel.cu:1750-1751), run where they stand
// when pfslam_set_topology enabled them.  The pose of the frame is already on the host (the step's header).
static int frame_topology(pfslam_handle *h, hipStream_t st = nullptr)
{
    if (!h->topo_in_step) return 0;
    topology_update_at(h, h->h_pose[0], h->h_pose[1]);
    return loop_closure_at(h, h->h_pose[0], h->h_pose[1], h->frame_closures, st);
}
// enable: 0 = off; 1 = at the end of every frame, the frame booked at once (the reference's synchronous call order); 2 = with the
// booking of the frame, i.e. `lag` steps later (KD frames: their visibility test reads the 2-D grid, which KD frames never write;
// a 2-D frame is still booked at once).  The graph and every frame's proposals are the same; pfslam_get_closures then returns
// those of the last BOOKED frame.
extern "C" int pfslam_set_topology(pfslam_handle *h, int enable)
{
    if (!h || enable < 0 || enable > 2) return fail("pfslam_set_topology: 0, 1 or 2");
    CHK(settle(h));
    if (enable == 2 && !h->topo_stream) HIPCHK(hipStreamCreateWithFlags(&h->topo_stream, hipStreamNonBlocking));
    h->topo_in_step = enable;
    h->frame_closures.clear();
    return 0;
}
extern "C" int pfslam_get_closures(pfslam_handle *h, int32_t *pairs, int cap, int *n)
{
    if (!h || !n || (cap > 0 && !pairs)) return fail("pfslam_get_closures: bad argument");
    const int count = (int)h->frame_closures.size() / 2;
    if (std::min(count, cap) > 0) memcpy(pairs, h->frame_closures.data(), (size_t)std::min(count, cap) * 8);
    *n = count;
    return 0;
}

extern "C" int pfslam_get_topology(pfslam_handle *h, float *nodes_xyd, int cap, int *n, int *node_idx)
{
    if (!h || !n) return fail("pfslam_get_topology: bad argument");
    const int cnt = (int)h->topo_nodes.size();
    for (int k = 0; k < std::min(cnt, cap); k++) {
        nodes_xyd[3 * k] = h->topo_nodes[k].x;
        nodes_xyd[3 * k + 1] = h->topo_nodes[k].y;
        nodes_xyd[3 * k + 2] = h->topo_nodes[k].dist;
    }
    *n = cnt;
    if (node_idx) *node_idx = (int)h->topo_idx;
    return 0;
}

// KDTree::Balance is due in front of this frame (kernel.cu:1707-1711): the one predicate for every caller (balance_if_due included)
static bool balance_due(const pfslam_handle *h, int frame)
{
    return h->cfg.balance_period > 0 && frame % h->cfg.balance_period == 5;
}
// KDTree::Balance on the host with the current weights when frame % period == 5 (kernel.cu:1707-1711)
static int balance_if_due(pfslam_handle *h, int frame)
{
    if (!(balance_due(h, frame) && h->kd_size > 0)) return 0;
    // KDTree::Balance re-creates the tree from the current node VALUES in array order (kdtree.cpp:31-40): positions of the nodes the
    // host has seen are in its mirror, so only the weights (every frame changes them) and the records of the nodes the device has
    // appended since come back -- not the links, which the re-build discards
    const int n = h->kd_size;
    const size_t K = (size_t)n, M0 = std::min((size_t)h->mirror_n, K);
    std::vector<float> pts(4 * K), wv(K), zn(K - M0);
    std::vector<uint4> hn(K - M0);
    HIPCHK(hipMemcpyAsync(wv.data(), h->kw, K * 4, hipMemcpyDeviceToHost, h->stream));
    if (K > M0) {
        HIPCHK(hipMemcpyAsync(hn.data(), h->hot + M0, (K - M0) * 16, hipMemcpyDeviceToHost, h->stream));
        if (!h->planar) HIPCHK(hipMemcpyAsync(zn.data(), h->kz + M0, (K - M0) * 4, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    {
        const pfslam_node *mir = h->h_nodes.data();
        const bool planar = h->planar != 0;
        parallel_chunks(n, [&](int lo, int hi, int) {
            for (int i = lo; i < hi; i++) {
                float *p = &pts[4 * (size_t)i];
                if ((size_t)i < M0) {
                    p[0] = mir[i].x; p[1] = mir[i].y; p[2] = mir[i].z;
                } else {
                    memcpy(&p[0], &hn[i - M0].x, 4);
                    memcpy(&p[1], &hn[i - M0].y, 4);
                    p[2] = planar ? 0.0f : zn[i - M0];
                }
                p[3] = wv[i];
            }
        });
    }
    std::vector<pfslam_node> tmp(K);
    if (pfslam_kd_create(pts.data(), n, tmp.data())) return fail("kd_balance failed");
    return upload_tree(h, tmp.data(), n, &tmp);
}
// ---- multi-GPU: ONE KDTree::Balance per node ---------------------------------------------------------------------------------
// Every rank holds the same map, so by default every rank of a sharded job would re-build it at frame % period == 5 -- eight
// concurrent 500 k-point builds on the cores one of them already fills (the reference has no counterpart: single GPU).  With
// pfslam_set_shard_balance(h, 1) the sharded frame leaves the re-balance to its caller:
//     pfslam_shard_balance_due(h, frame, &due, &n)     every rank, in front of pfslam_shard_disperse (books the frames in flight)
//     due:  root: pfslam_shard_balance_build(h, frame)  the host build of csrc/kd_host.cpp with all the node's usable cores
//           broadcast buffers 20 .. 24 from root        n x {16, 4, 4, 4} bytes of map records + 16 bytes of state (28 B per node)
//           others: pfslam_shard_balance_adopt(h)       host bookkeeping only: size, flags, mirror and cell rows start over
extern "C" int pfslam_set_shard_balance(pfslam_handle *h, int external)
{
    if (!h) return fail("null handle");
    h->balance_external = external != 0;
    return 0;
}
extern "C" int pfslam_shard_balance_due(pfslam_handle *h, int frame, int *due, int *n_nodes)
{
    if (!h || !due || !n_nodes) return fail("pfslam_shard_balance_due: bad argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    const bool period_hit = balance_due(h, frame);
    if (period_hit) CHK(settle(h)); // the map size is the host's view of it
    *due = period_hit && h->kd_size > 0 ? 1 : 0;
    *n_nodes = h->kd_size;
    return 0;
}
extern "C" int pfslam_shard_balance_build(pfslam_handle *h, int frame)
{
    if (!h) return fail("null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    CHK(settle(h));
    // the node's only build (every other rank waits for the broadcast): all usable cores, not this rank's 1 / LOCAL_WORLD_SIZE share
    pfslam_kd_whole_node(1);
    const int rc = balance_if_due(h, frame);
    pfslam_kd_whole_node(0);
    return rc;
}
extern "C" int pfslam_shard_balance_adopt(pfslam_handle *h)
{
    if (!h) return fail("null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    CHK(settle(h));
    int st[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(st, h->kd_state, 16, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (st[0] != h->kd_size) return fail("pfslam_shard_balance_adopt: the broadcast map has " + std::to_string(st[0]) + " nodes, this rank's " + std::to_string(h->kd_size));
    h->planar = st[1];
    h->integral_w = st[2] != 0 && (double)st[2] * (double)h->nb <= (double)PF_SUM_EXACT; // (upload_tree's class, with this rank's beam count)
    h->w_absmax = st[2] != 0 ? (float)st[2] : 113.0f;
    h->lattice_ok = st[3] != 0;
    h->mirror_n = 0; // the host mirror knows nothing of the new topology: read back whole when somebody asks (pfslam_get_map)
    h->mirror_stale = true;
    h->cells_wipe_pending = true;
    return 0;
}

extern "C" int pfslam_maybe_balance(pfslam_handle *h, int frame)
{
    if (!h) return fail("null handle");
    HIPCHK(hipSetDevice(h->cfg.device));
    CHK(settle(h));
    return balance_if_due(h, frame);
}
extern "C" int pfslam_kd_size(pfslam_handle *h)
{
    if (!h || settle(h)) return -1;
    return h->kd_size;
}

// pinned staging slot of a frame's scan (one per ticket: the copy of an earlier frame may still be queued), reach hint, upload
static int stage_scan(pfslam_handle *h, int seq, const float *scan_host)
{
    float *hs = h->h_scan + (size_t)(seq % PF_HDR_SLOTS) * h->nb;
    h->scan = h->scan_base + (size_t)(seq % PF_HDR_SLOTS) * h->nb;
    memcpy(hs, scan_host, (size_t)h->nb * 4);
    scan_reach_of(h, hs);
    HIPCHK(hipMemcpyAsync(h->scan, hs, (size_t)h->nb * 4, hipMemcpyHostToDevice, h->stream));
    return 0;
}

// ---- whole step: particleFilter (kernel.cu:1702-1762) ----------------------------------------
// The frame is ENQUEUED: dispersion, scoring, weights, ICP, map update with the insert of the new walls, and the resample
// (decided on the device).  Then the host books the frame `lag` steps back (trace, pose, deferred errors) and returns, so the
// next call overlaps this frame's execution.  Every other entry point settles the frames in flight before it does anything,
// so pfslam_step + any getter behaves like the synchronous call of the reference.  A deferred error (kd_capacity exhausted,
// cell list overflow) is reported by the call that books the frame.
//
// The same four pieces make the single-GPU frame (pfslam_step) and the sharded frame (pfslam_shard_*: the caller's collectives
// sit between them); neither waits for the device anywhere.
//   frame_front    scan into its pinned slot, re-balance if due, first scan seeds the map, ICP fork, dispersion
//   frame_score    lane order, plan, scan-match, reduce + packed min / max keys (+ this shard's 16-byte record: its packed keys)
//   [single GPU: k_best_pose | sharded: all-gather of the records, k_weights_apply_sharded]  -> the frame's pose
//   frame_map_lists  rays, cell lists and their traversal on the aux stream (needs the pose only)
//   frame_tail     weights, sums + Neff on the GLOBAL weights, k_test_new (insert + header), gated resample, booking
static int frame_front(pfslam_handle *h, int frame, const float *scan_host, int *seeded)
{
    if (balance_due(h, frame) || h->kd_size == 0 || h->topo_in_step == 1) CHK(settle(h)); // these need the host's view of the map / the pose
    h->cur_seq = ++h->seq;
    h->cur_frame = frame;
    CHK(stage_scan(h, h->cur_seq, scan_host));
    if (!h->balance_external && !h->balance_done) CHK(balance_if_due(h, frame)); // (external: the caller has seen to it, pfslam_shard_balance_*)
    h->balance_done = false;
    *seeded = 0;
    if (h->kd_size == 0) { // first scan seeds the map (kernel.cu:1714-1717)
        HIPCHK(hipMemsetAsync(h->pose, 0, 16, h->stream));
        CHK(launch_map_update_device(h));
        CHK(seed_map_from_walls(h));
        *seeded = 1;
        return 0;
    }
    CHK(fork_icp(h)); // scan is queued, the pose is still last frame's: the ICP solve runs under the score kernel
    CHK(phase_begin(h));
    hipLaunchKernelGGL(k_motion, dim3((h->n + 255) / 256), dim3(256), 0, h->stream, h->x, h->y, h->th, h->w, h->wm, h->n,
                       frame, h->goff, h->trig);
    HIPCHK(hipGetLastError());
    CHK(phase_end(h, PF_T_MOTION));
    h->theta_bound += 0.1f;
    return 0;
}
// sums + Neff, insert + header, gated resample; then the frame is in flight and the host books the one `lag` steps back
static int frame_tail(pfslam_handle *h, bool fork)
{
    const int seq = h->cur_seq, frame = h->cur_frame;
    CHK(phase_end(h, PF_T_MEASURE));
    h->icp_delta_ready = false;
    // k_test_new inserts the new walls and writes the frame's header (Neff included: behind the sums)
    CHK(launch_map_update_device(h, seq, fork, fork ? 2 : 0));
    CHK(phase_end(h, PF_T_MAP));
    CHK(launch_resample(h, frame, /*gated=*/true));
    CHK(phase_end(h, PF_T_RESAMPLE));
    h->in_flight.push_back(pfslam_handle::Frame{seq, frame, 0, h->plan_valid || h->cells_valid});
    while ((int)h->in_flight.size() > (h->topo_in_step == 1 ? 0 : h->lag)) CHK(consume_frame(h));
    if (h->topo_in_step == 1) CHK(frame_topology(h, nullptr)); // //UpdateTopology(); //CheckLoopClosure(); (kernel.cu:1750-1751) when enabled
    return 0;
}

// a round-4 frame (KD or grid) behind round-5 frames: nothing of those may still be in flight -- their launches sit on four streams
// and are ordered by the frame ring, which the round-4 chain knows nothing about
static int leave_frame_v2(pfslam_handle *h)
{
    return h->pipe_live ? settle_staged(h) : 0;
}

// What pfslam_step and pfslam_shard_disperse do in front of a frame: the frames in flight are booked before a re-balance (and for handles
// with topology in the step), the re-balance itself (unless the caller has seen to it: pfslam_shard_balance_*), and the choice of the
// frame -- round-5 frame (pfslam_frame.hip.inc) whenever the pass is organised by lattice-cell rows.  *v2 = 0: the caller goes on with
// frame_front, which must not re-balance the re-balanced tree (*rebalanced, handed over immediately in front of that call).
static int frame_choice(pfslam_handle *h, int frame, int *v2, int *used, int *bpc, bool *rebalanced)
{
    *v2 = 0;
    *rebalanced = false;
    if (h->kd_size > 0 || !h->in_flight.empty()) {
        const bool due = balance_due(h, frame);
        if (due || h->topo_in_step == 1) CHK(settle(h));
        if (due && !h->balance_external && h->kd_size > 0) {
            CHK(balance_if_due(h, frame));
            *rebalanced = true;
        }
        if (h->kd_size > 0 && frame_v2_ok(h, used, bpc)) {
            *v2 = 1;
            return 0;
        }
    }
    return leave_frame_v2(h);
}

extern "C" int pfslam_step(pfslam_handle *h, int frame, const float *scan_host)
{
    if (!h || !scan_host) return fail("pfslam_step: bad argument");
    if (h->own_global) return fail("pfslam_step: sharded handles are stepped through pfslam_shard_* by the multi-GPU harness");
    HIPCHK(hipSetDevice(h->cfg.device));
    int v2 = 0, used = 0, bpc = 0;
    bool rebalanced = false;
    h->shard_call = false;
    CHK(frame_choice(h, frame, &v2, &used, &bpc, &rebalanced));
    if (v2) return frame_v2(h, frame, scan_host, used, bpc);
    int seeded = 0;
    h->balance_done = rebalanced; // (consumed and cleared by frame_front)
    CHK(frame_front(h, frame, scan_host, &seeded));
    if (seeded) return 0;
    const bool fork = h->timing < 2; // the map update on the aux stream, unless the phases are timed
    h->cells_async = fork;           // ... and with it the marking and the walks of the new lattice cells (kd_cells.hip.inc)
    h->score_on_aux = fork;          // ... and the scan-match kernel itself, when the frame's cell passes are asynchronous (launch_score)
    const int src = launch_score(h, /*fuse_minmax=*/true); // joins the aux stream before the reduce: the keys were reset there
    h->cells_async = h->score_on_aux = false;
    CHK(src);
    if (fork) {
        // The map update is the longer branch of the frame's tail and needs only the pose: best particle + ICP increment, one
        // tiny launch right behind the reduce.  Lists and traversal start on the aux stream while the weights are still summed.
        hipStream_t ss = h->scored_on_aux ? h->aux : h->stream;
        hipLaunchKernelGGL(k_best_pose, dim3(1), dim3(64), 0, ss, (const long long *)h->stats, h->x, h->y, h->th, h->n, h->start,
                           (const float *)h->icp_dbg, h->pose);
        HIPCHK(hipGetLastError());
        if (h->scored_on_aux) { // this stream goes on with the weights: it needs the scores, the keys and (host mirror) nothing else
            HIPCHK(hipEventRecord(h->ev_scored, h->aux));
            HIPCHK(hipStreamWaitEvent(h->stream, h->ev_scored, 0));
        }
        CHK(launch_map_update_device(h, h->cur_seq, true, /*part=*/1));
    }
    // weights are final for this frame: Neff now (the header and the resample gate read it); without the fork the same launch
    // adds the ICP increment to the best particle's pose
    if (h->n <= PF_SUM_TILE) {
        CHK(launch_weights_small(h, false, !fork, !fork));
    } else {
        CHK(launch_weights(h, false, !fork));
        CHK(launch_weight_sums_with_scan_front(h, !fork));
    }
    const int trc = frame_tail(h, fork);
    h->scored_on_aux = false;
    return trc;
}

extern "C" int pfslam_set_lag(pfslam_handle *h, int frames)
{
    if (!h || frames < 0 || frames > PF_MAX_LAG) return fail("pfslam_set_lag: 0 .. 2 frames");
    HIPCHK(hipSetDevice(h->cfg.device));
    CHK(settle(h));
    h->lag = frames;
    return 0;
}

// ---- the same frame for a multi-GPU caller (sharded.py, host/pfslam_mgpu.cpp) -------------------
// Particles are sharded, the map / scan / ICP / map update are replicated.  The caller's collectives sit between the calls;
// the schedule is FIXED -- three all-gathers in every frame, none of them data-dependent -- and, like pfslam_step, no call
// waits for the device: the resample is decided on the device on the gathered weights, its sources are read from the gathered
// pose blocks, and the frame is booked one step later from its pinned header.  The four calls are the four parts of the round-5 frame
// (pfslam_frame.hip.inc) -- the frame pfslam_step runs -- and every collective goes straight into one of the frame's own streams:
// pfslam_shard_stream names it (ask after the call in front of the collective; it is the handle's stream in one-stream frames).
//   pfslam_shard_disperse   scan, re-balance if due, (first scan: seed); dispersion + lane order of this shard; cells' passes; ICP solve
//   [all-gather buffer 16 -> 17, stream 0]  pose blocks [x | y | theta], 3 * stride floats per rank: on the particle stream, which has
//                                  nothing else to do until the reduce -- the collective runs UNDER the scan-match kernel
//   pfslam_shard_score      (job-wide |heading| maximum out of the gathered blocks;) scan-match, reduce -> this shard's packed keys (buffer 14)
//   [all-gather buffer 14 -> 15, stream 1]  16 bytes per rank, on the chain stream between the reduce and the walls: the one collective
//                                  on the frame's critical chain
//   pfslam_shard_weights    walls at the frame's pose (best particle of the whole job, read out of the gathered pose blocks, + ICP
//                           increment), insert, cell rows; weights of this shard from the job's min / max
//   [all-gather buffer 5 -> 10, stream 0]   weights, stride floats per rank, on the particle stream
//   pfslam_shard_finish     sums + Neff on the gathered weights, header, gated resample from the gathered pose blocks; the free cells'
//                           chain; booking
// A map the lattice-cell rows do not cover (frame_v2_ok) takes the staged chain instead -- same calls, same buffers, same collectives,
// all of them on the handle's stream (pfslam_shard_stream says so).
extern "C" int pfslam_shard_disperse(pfslam_handle *h, int frame, const float *scan_host, int *seeded)
{
    if (!h || !scan_host || !seeded) return fail("pfslam_shard_disperse: bad argument");
    HIPCHK(hipSetDevice(h->cfg.device));
    if (h->timing >= 2) return fail("pfslam_shard_disperse: per-phase timing (pfslam_set_timing 2) is for pfslam_step only");
    h->shard_stage = 0;
    h->shard_v2 = false;
    h->shard_call = true;
    *seeded = 0;
    int v2 = 0, used = 0, bpc = 0;
    bool rebalanced = false;
    CHK(frame_choice(h, frame, &v2, &used, &bpc, &rebalanced));
    if (v2) {
        CHK(frame_v2_begin(h, frame, scan_host, used, bpc, /*sharded=*/true));
        h->shard_v2 = true;
        h->shard_stage = 1;
        return 0;
    }
    h->balance_done = rebalanced; // (consumed and cleared by frame_front)
    CHK(frame_front(h, frame, scan_host, seeded));
    if (!*seeded) h->shard_stage = 1;
    return 0;
}
extern "C" int pfslam_shard_score(pfslam_handle *h)
{
    if (!h) return fail("null handle");
    if (h->shard_stage != 1) return fail("pfslam_shard_score: call pfslam_shard_disperse first (and skip the frame when it seeded the map)");
    HIPCHK(hipSetDevice(h->cfg.device));
    if (h->shard_v2) {
        CHK(frame_v2_score(h));
    } else {
        h->cells_async = true; // the sharded frame's map update always runs on the aux stream
        const int src = launch_score(h, /*fuse_minmax=*/true, nullptr, /*sharded=*/true);
        h->cells_async = false;
        CHK(src);
    }
    h->shard_stage = 2;
    return 0;
}
extern "C" int pfslam_shard_weights(pfslam_handle *h)
{
    if (!h) return fail("null handle");
    if (h->shard_stage != 2) return fail("pfslam_shard_weights: call pfslam_shard_score first");
    HIPCHK(hipSetDevice(h->cfg.device));
    if (h->shard_v2) {
        CHK(frame_v2_chain(h));
    } else {
        // launch_score joined the ICP solve (the aux stream also reset the keys there): its increment is ready.  The merged keys go where
        // the staged chain's header and resample expect the frame's keys (stats); the best particle's pose comes out of the gathered blocks,
        // whose all-gather sits in front of the scan-match kernel on this very stream.
        const bool multi = h->world > 1;
        hipLaunchKernelGGL(k_weights_apply_sharded, dim3((h->n + 255) / 256), dim3(256), 0, h->stream, h->w, h->wm, (const float *)h->fit,
                           h->n, h->goff, mirror_count(h), (const long long *)h->stats, multi ? (const long long *)h->gkeys : (const long long *)nullptr,
                           h->world, (const float *)h->gpose, h->stride, (long long *)h->stats, h->start, (const float *)h->icp_dbg, h->pose,
                           (unsigned long long *)nullptr);
        HIPCHK(hipGetLastError());
        h->icp_delta_ready = false;
        CHK(launch_map_update_device(h, h->cur_seq, true, /*part=*/1)); // needs the pose only
    }
    h->shard_stage = 3;
    return 0;
}
extern "C" int pfslam_shard_finish(pfslam_handle *h)
{
    if (!h) return fail("null handle");
    if (h->shard_stage != 3) return fail("pfslam_shard_finish: call pfslam_shard_weights first");
    HIPCHK(hipSetDevice(h->cfg.device));
    h->shard_stage = 0;
    if (h->shard_v2) return frame_v2_finish(h);
    CHK(launch_weight_sums_with_scan_front(h, false)); // on the gathered global weights
    return frame_tail(h, true);
}
// The stream a caller issues collective `which` of the frame being enqueued on (0 pose blocks, 1 keys, 2 weights): query it after the
// pfslam_shard_* call in front of that collective.  Stream order is all the ordering there is: the library has enqueued what the
// collective waits for in front of it and enqueues its consumers behind it.
extern "C" int pfslam_shard_stream(pfslam_handle *h, int which, void **hip_stream)
{
    if (!h || !hip_stream || which < 0 || which > 2) return fail("pfslam_shard_stream: bad argument");
    hipStream_t st = h->stream;
    if (h->shard_v2 && which == 1 && !h->fv.serial) st = h->aux;
    *hip_stream = (void *)st;
    return 0;
}

// The frame loop of particleFilter (kernel.cu:1702-1762) with the reference's 2-D stages in place of the KD
// ones: PFMotionUpdate, PFMeasurementUpdate (GPU branch, 307-339: robotPos = best particle), PFUpdateMap (GPU
// branch, 551-577), PFResample.  The reference defines these but ships the KD variants wired (SURVEY 3.3).
// One host sync per frame, for the resample decision.
extern "C" int pfslam_step_grid(pfslam_handle *h, int frame, const float *scan_host)
{
    if (!h || !scan_host) return fail("pfslam_step_grid: bad argument");
    if (h->own_global) return fail("pfslam_step_grid: sharded handles are stepped by the multi-GPU harness");
    HIPCHK(hipSetDevice(h->cfg.device));
    if (h->topo_in_step) CHK(settle(h));
    CHK(leave_frame_v2(h));
    // a preceding pfslam_step may have left its map update on the aux stream: it reads the masks, the pose, the counts and the
    // sums this frame is about to overwrite (and wipes the masks as its last reader)
    CHK(join_map(h));
    const int seq = ++h->seq;
    CHK(stage_scan(h, seq, scan_host));
    hipLaunchKernelGGL(k_motion, dim3((h->n + 255) / 256), dim3(256), 0, h->stream, h->x, h->y, h->th, h->w, h->wm, h->n, frame,
                       h->goff, h->trig);
    h->theta_bound += 0.1f;
    CHK(score_grid_launch(h, true)); // score + int min/max/argmax + weights + their sums; the best particle's pose lands in `start`
    HIPCHK(hipMemcpyAsync(h->pose, h->start, 12, hipMemcpyDeviceToDevice, h->stream));
    CHK(launch_update_map_grid(h));
    CHK(launch_header(h, seq, false));
    CHK(launch_resample(h, frame, /*gated=*/true)); // decided on the device, like the KD frame
    h->in_flight.push_back(pfslam_handle::Frame{seq, frame, 1});
    while ((int)h->in_flight.size() > (h->topo_in_step ? 0 : h->lag)) CHK(consume_frame(h));
    if (h->topo_in_step) CHK(frame_topology(h));
    return 0;
}
