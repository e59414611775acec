// The text of the pfslam_search_cov kernels (csrc/pfslam_search_cov.hip.inc behind the unchanged text of pfslam_estimate's device
// functions, of csrc/pfslam_search.hip.inc and of csrc/pfslam_search_scan.hip.inc, cut out by tests/test_search_cov_kernel_text.py) run on
// the CPU behind tests/simt_shim.h.  The call is pfslam_search_scan_cov's: the scan form needs no tree.  Every buffer has exactly the size
// the entry point requests, so that a sanitizer build sees any overrun.  TEST INFRASTRUCTURE, not product code.
#include "simt_shim.h"
#include "kernel_text.inc"

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
    launch_serial((nb + 255) / 256, 256, [&] { k_scan_points(ref.data(), fl[6], fl[7], fl[8], nb, trig, pts.data(), &count); });
    launch_threads(na, 256, [&] { k_search_ends(scan.data(), p, trig, ends.data(), nin.data(), box); });
    launch_serial((p.cap / 2 + 1 + 255) / 256, 256, [&] { k_scan_fill(p, box, field); });
    launch_serial((nb + 3) / 4, 256, [&] { k_scan_splat(pts.data(), nb, R, p, box, field); });
    const int chunks = (nx * ny + 63) / 64;
    launch_threads(na * chunks, 64, [&] { k_search_score(ends.data(), nin.data(), box, field, p, chunks, scores.data(), key); });
    launch_serial(1, 1, [&] { k_search_result(key, nin.data(), p, out.data()); });
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
        launch_threads(1, PF_EST_WAVES * 64, [&] { k_cov_small(scores.data(), key, p, q, part.data(), cov.data()); });
    } else {
        launch_threads(nt, PF_EST_WAVES * 64, [&] { k_cov_moments(scores.data(), key, p, q, part.data(), nt); });
        launch_threads(nt, PF_EST_WAVES * 64, [&] { k_cov_centred(scores.data(), key, p, q, part.data(), part.data() + (size_t)5 * nt, nt); });
        launch_threads(1, 64, [&] { k_cov_final(part.data(), key, q, nt, cov.data()); });
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
