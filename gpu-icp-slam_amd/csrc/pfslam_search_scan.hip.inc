// pfslam_search_scan.hip.inc -- pfslam_search_scan (correlative scan-to-scan search: pfslam_search's window scored against a distance field
// built from the end points of a reference scan instead of the map; the handle needs no map); the specification is in include/pfslam.h.
// Included by pfslam_hip.hip behind pfslam_search.hip.inc (same translation unit): it reuses SearchParams, search_box, k_search_ends,
// k_search_score and k_search_result as they are, and leaves the field in the layout k_search_score reads.  The entry point is a thin
// call into the family's one volume runner, search_volume (pfslam_search_cov.hip.inc), which launches this file's kernels for the field.
// tests/test_search_scan_kernel_text.py cuts the text between the two SEARCH-SCAN-KERNEL-TEXT marks out and runs it on the CPU.

// SEARCH-SCAN-KERNEL-TEXT-BEGIN
#define PF_SCAN_NO_POINT 0x7fc00000 /* pts[].x of a beam that gives no point (a NaN: a point never has one, it would have been skipped) */

// One thread per beam of the reference scan: step 1 of pfslam_register at the reference pose.  A beam out of range gives no point; the
// points are counted in the same pass (one atomic per wave: the compiler merges the lanes' adds).
__global__ __launch_bounds__(256) void k_scan_points(const float *__restrict__ ref, float rx, float ry, float rt, int nb, int trig,
                                                     float2 *__restrict__ pts, int *count)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nb) return;
    float wx, wy;
    pf::clean_lidar_scan(b, ref[b], rt, wx, wy, trig);
    float2 p;
    p.x = __int_as_float(PF_SCAN_NO_POINT);
    p.y = 0.0f;
    if (fabsf(wx) < PF_LIDAR_RANGE && fabsf(wy) < PF_LIDAR_RANGE) {
        p.x = rx + wx;
        p.y = ry + wy;
        atomicAdd(count, 1);
    }
    pts[b] = p;
}

// One thread per pair of cells of the box: every cell starts at qcap, the value of a cell no point is near.  The launch covers the `cap`
// cells the host bounds the box by; the threads behind the box leave at once.  Thread 0 writes the two spare cells (k_search_score).
__global__ __launch_bounds__(256) void k_scan_fill(SearchParams p, const int *__restrict__ box, uint16_t *__restrict__ field)
{
    const SearchBox B = search_box(box, p);
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id == 0) {
        field[p.cap] = 0;
        field[p.cap + 1] = (uint16_t)p.qcap;
    }
    const int cells = min(B.W * B.H, p.cap); // (W * H <= cap: the host's bound)
    const int c = 2 * id;
    if (c >= cells) return;
    if (c + 1 < cells)
        *(unsigned int *)(field + c) = (unsigned)p.qcap * 0x10001u; // (the buffer is 4-byte aligned and c is even)
    else
        field[c] = (uint16_t)p.qcap;
}

// q of one cell for one point: the specification's arithmetic.  d2 is finite or +inf here (a point and a lattice coordinate are finite).
__device__ __forceinline__ unsigned scan_q(float px, float py, int kx, int ky, const SearchParams &p)
{
    const float dx = px - (float)kx * p.res, dy = py - (float)ky * p.res;
    const float r = rintf(pf::fdiv(dx * dx + dy * dy, p.u));
    return r >= (float)p.qcap ? (unsigned)p.qcap : (unsigned)(int)r;
}

// The splat.  One wave per point: the point visits the (2R + 1)^2 cells around its own cell (cx, cy) = (rint(px / res), rint(py / res)),
// clipped to the box, and lowers each to its q.  An integer minimum is exact in any order, so the field does not depend on the schedule.
//   Why R = ceil(max_dist / res) + 2 is enough: a cell outside the neighbourhood has |kx - cx| >= R + 1 in one coordinate, so it is at
//   least (R + 0.5) res >= max_dist + 2.5 res from the point in that coordinate -- less the float rounding of px / res and (float)kx * res,
//   below a quarter of a cell inside +-2^20 cells -- and 16 (max_dist / res + 2)^2 > qcap + 1: its q saturates, which is what it holds.
// Sixteen-bit cells have no atomic minimum.  A lane therefore owns one aligned 32-bit word -- two adjacent cells of a row -- computes both
// q and lowers both halves with ONE compare-and-swap; the lanes of a wave take adjacent words of a row, so no two lanes of a wave ever
// meet in a word, a wave's request is one contiguous run of up to 256 bytes, and only different points near one cell retry.  A word that
// is already low enough (the usual case once a few beams have fallen into a cell) costs a plain load.  A half outside the point's
// neighbourhood, the row or the box is swapped for itself.
__global__ __launch_bounds__(256) void k_scan_splat(const float2 *__restrict__ pts, int nb, int R, SearchParams p, const int *__restrict__ box,
                                                    uint16_t *field)
{
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= nb) return;
    const SearchBox B = search_box(box, p);
    if (B.W <= 0 || B.H <= 0 || B.W * B.H > p.cap) return; // no searched beam has a cell: nothing reads the field
    const float2 pt = pts[b];
    const float fx = rintf(pf::fdiv(pt.x, p.res)), fy = rintf(pf::fdiv(pt.y, p.res));
    const float lim = (float)(PF_SEARCH_CELL_MAX + R);
    if (!(fabsf(fx) <= lim && fabsf(fy) <= lim)) return; // no point, a point that is not finite or one farther out than any box: qcap everywhere
    const int cx = (int)fx, cy = (int)fy;
    const int x_lo = max(cx - R, B.x0), x_hi = min(cx + R, B.x0 + B.W - 1);
    const int y_lo = max(cy - R, B.y0), y_hi = min(cy + R, B.y0 + B.H - 1);
    if (x_lo > x_hi || y_lo > y_hi) return;
    const int wpr = (x_hi - x_lo) / 2 + 2; // words a row's run of cells can touch
    const int items = (y_hi - y_lo + 1) * wpr;
    unsigned int *words = (unsigned int *)field;
    for (int t = lane; t < items; t += 64) {
        const int ky = y_lo + t / wpr;
        const int id0 = (ky - B.y0) * B.W + (x_lo - B.x0), id1 = id0 + (x_hi - x_lo); // the row's run of cells, inside [0, W H)
        const int w = (id0 >> 1) + t % wpr;
        if (w > (id1 >> 1)) continue;
        const int c0 = 2 * w, c1 = c0 + 1;
        const bool in0 = c0 >= id0, in1 = c1 <= id1;
        const unsigned q0 = in0 ? scan_q(pt.x, pt.y, x_lo + (c0 - id0), ky, p) : 0xffffu;
        const unsigned q1 = in1 ? scan_q(pt.x, pt.y, x_lo + (c1 - id0), ky, p) : 0xffffu;
        unsigned old = words[w];
        for (;;) {
            const unsigned lo = min(old & 0xffffu, q0), hi = min(old >> 16, q1);
            const unsigned want = (hi << 16) | lo;
            if (want == old) break;
            const unsigned seen = atomicCAS(&words[w], old, want);
            if (seen == old) break;
            old = seen;
        }
    }
}
// SEARCH-SCAN-KERNEL-TEXT-END

// The field of a call from a list of points: the box of search_box() filled with qcap, then the splat.  (A separate function taking a
// point list: a map's nodes are such a list too.)
static int scan_field_from_points(pfslam_handle *h, const float2 *pts, int npts, const SearchParams &p, float max_dist, const int *box, uint16_t *field)
{
    const int R = (int)ceilf(pf::fdiv(max_dist, p.res)) + 2; // (qcap <= 65535 bounds max_dist / res by 64.001: R <= 67)
    hipLaunchKernelGGL(k_scan_fill, dim3((unsigned)((p.cap / 2 + 1 + 255) / 256)), dim3(256), 0, h->stream, p, box, field);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_scan_splat, dim3((unsigned)((npts + 3) / 4)), dim3(256), 0, h->stream, pts, npts, R, p, box, field);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int pfslam_search_scan(pfslam_handle *h, const float *ref_scan_host, const float ref_pose[3], const float *scan_host, const float centre[3],
                                  const pfslam_search_opts *opts, float pose_out[3], float info[8], int32_t *scores)
{
    if (!h || !opts || !pose_out || !info) return fail("pfslam_search_scan: bad argument");
    if (!ref_scan_host) return fail("pfslam_search_scan: ref_scan_host must not be NULL");
    return search_volume(h, "pfslam_search_scan", PF_FORM_NO_MAP, ref_scan_host, ref_pose, scan_host, centre, opts, nullptr, pose_out, info, nullptr, scores);
}
