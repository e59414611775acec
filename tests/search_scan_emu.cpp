// The text of the pfslam_search_scan kernels (csrc/pfslam_search_scan.hip.inc behind the unchanged text of csrc/pfslam_search.hip.inc and
// what that reuses, cut out by tests/test_search_scan_kernel_text.py) run on the CPU behind tests/simt_shim.h: k_search_ends and
// k_search_score a thread per GPU thread; k_scan_points, k_scan_fill and k_scan_splat, whose threads meet nowhere but in atomics, one
// thread after the other.  Every buffer has exactly the size pfslam_search_scan requests, so that a sanitizer build sees any overrun.
// TEST INFRASTRUCTURE, not product code.
#include "simt_shim.h"
#include "kernel_text.inc"

// usage: search_scan_emu IN.bin OUT.bin
//   IN  = int32 {nb, trig, half_x, half_y, half_theta, stride, 0, 0}, float {cx, cy, ct, step_theta, max_dist, res, rx, ry, rt, 0, 0, 0},
//         ref[nb], scan[nb]
//   OUT = the 12 floats of k_search_result's `out`, int32 {box cells W, H, points, R}, then the score volume, one int32 per candidate
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
    launch_serial((nb + 255) / 256, 256, [&] { k_scan_points(ref.data(), fl[6], fl[7], fl[8], nb, trig, pts.data(), &count); });
    launch_threads(na, 256, [&] { k_search_ends(scan.data(), p, trig, ends.data(), nin.data(), box); });
    launch_serial((p.cap / 2 + 1 + 255) / 256, 256, [&] { k_scan_fill(p, box, field); });
    launch_serial((nb + 3) / 4, 256, [&] { k_scan_splat(pts.data(), nb, R, p, box, field); });
    const int chunks = (nx * ny + 63) / 64;
    launch_threads(na * chunks, 64, [&] { k_search_score(ends.data(), nin.data(), box, field, p, chunks, scores.data(), key); });
    launch_serial(1, 1, [&] { k_search_result(key, nin.data(), p, out.data()); });
    const SearchBox B = search_box(box, p);
    const int dims[4] = {B.W, B.H, count, R};
    f = fopen(argv[2], "wb");
    fwrite(out.data(), 4, out.size(), f);
    fwrite(dims, 4, 4, f);
    fwrite(scores.data(), 4, scores.size(), f);
    fclose(f);
    return 0;
}
