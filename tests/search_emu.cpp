// The text of the pfslam_search kernels (csrc/pfslam_search.hip.inc behind the text of csrc/pfslam_register.hip.inc it reuses, cut out by
// tests/test_search_kernel_text.py) run on the CPU behind tests/simt_shim.h: k_search_ends and k_search_score, which have barriers or
// shuffles, a thread per GPU thread; k_search_field, whose threads meet nowhere, one thread after the other.  Every buffer has exactly the
// size pfslam_search requests, so that a sanitizer build sees any overrun.  TEST INFRASTRUCTURE, not product code.
#include "simt_shim.h"
#include "kernel_text.inc"

// usage: search_emu IN.bin OUT.bin
//   IN  = int32 {n_nodes, planar, nb, trig, half_x, half_y, half_theta, stride}, float {cx, cy, ct, step_theta, max_dist, res, 0, 0},
//         hot[n] (16 B), z[n], parent[n], w[n], scan[nb]
//   OUT = the 12 floats of k_search_result's `out`, int32 {box cells W, H, 0, 0}, then the score volume, one int32 per candidate
int main(int argc, char **argv) {
    if (argc < 3) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const auto hd = rd<int>(f, 8);
    const auto fl = rd<float>(f, 8);
    const int n = hd[0], planar = hd[1], nb = hd[2], trig = hd[3];
    const auto hot = rd<uint4>(f, n);
    const auto z = rd<float>(f, n);
    const auto parent = rd<int>(f, n);
    const auto w = rd<float>(f, n);
    const auto scan = rd<float>(f, nb);
    fclose(f);
    const pf::KdView tree{hot.data(), z.data(), parent.data(), w.data(), planar};
    // what every entry point derives from its arguments: the library's own search_derive (csrc/pfslam_search.hip.inc), cut out with the kernels
    SearchParams p;
    SearchWhy why;
    const SearchRefusal no = search_derive(fl[5], nb, &fl[0], hd[4], hd[5], hd[6], hd[7], fl[3], fl[4], &p, &why);
    if (no != SEARCH_FITS) return no == SEARCH_QCAP ? 5 : 6;
    const int nx = 2 * p.hx + 1, ny = 2 * p.hy + 1, na = 2 * p.ht + 1;
    const size_t cand = (size_t)nx * ny * na;
    // exact sizes: the sanitizer sees any overrun
    std::vector<uint16_t> field((size_t)p.cap + 2, 0xdead);
    std::vector<int2> ends((size_t)na * nb, int2{7, 7});
    std::vector<int> nin((size_t)na, -7), scores(cand, -7);
    unsigned long long state[3];
    memset(state, 0xff, sizeof(state));
    unsigned long long *key = state;
    int *box = (int *)(state + 1);
    std::vector<float> out(PF_SEARCH_OUT, -1.0f);
    launch_threads(na, 256, [&] { k_search_ends(scan.data(), p, trig, ends.data(), nin.data(), box); });
    launch_serial((p.cap + 255) / 256, 256, [&] { k_search_field(tree, p, box, field.data()); }); // (no barrier, no shuffle: the threads of a workgroup one after the other)
    const int chunks = (nx * ny + 63) / 64;
    launch_threads(na * chunks, 64, [&] { k_search_score(ends.data(), nin.data(), box, field.data(), p, chunks, scores.data(), key); });
    launch_serial(1, 1, [&] { k_search_result(key, nin.data(), p, out.data()); });
    const SearchBox B = search_box(box, p);
    const int dims[4] = {B.W, B.H, 0, 0};
    f = fopen(argv[2], "wb");
    fwrite(out.data(), 4, out.size(), f);
    fwrite(dims, 4, 4, f);
    fwrite(scores.data(), 4, scores.size(), f);
    fclose(f);
    return 0;
}
