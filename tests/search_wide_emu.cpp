// The text of the pfslam_search_wide kernels (csrc/pfslam_search_wide.hip.inc behind the text of csrc/pfslam_search.hip.inc and
// csrc/pfslam_register.hip.inc it reuses, cut out by tests/test_search_wide_kernel_text.py) run on the CPU behind tests/simt_shim.h, every
// buffer at the exact size pfslam_search_wide requests so that a sanitizer build sees any overrun.  The host's descent (batches of a
// quarter of a frontier buffer, depth first) is restated below, statement for statement.  TEST INFRASTRUCTURE, not product code.
#include "simt_shim.h"
#include "kernel_text.inc"

// usage: search_wide_emu IN.bin OUT.bin
//   IN  = int32 {n_nodes, planar, nb, trig, half_x, half_y, half_theta, stride, frontier nodes, 0}, float {cx, cy, ct, step_theta, max_dist, res, 0, 0},
//         hot[n] (16 B), z[n], parent[n], w[n], scan[nb]
//   OUT = the 12 floats of k_search_result's `out`, then the eight int64 of `stats`
int main(int argc, char **argv) {
    if (argc < 3) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const auto hd = rd<int>(f, 10);
    const auto fl = rd<float>(f, 8);
    const int n_nodes = hd[0], planar = hd[1], nb = hd[2], trig = hd[3], room = hd[8];
    const auto hot = rd<uint4>(f, n_nodes);
    const auto z = rd<float>(f, n_nodes);
    const auto parent = rd<int>(f, n_nodes);
    const auto w = rd<float>(f, n_nodes);
    const auto scan = rd<float>(f, nb);
    fclose(f);
    if (room < 4) return 7;
    const pf::KdView tree{hot.data(), z.data(), parent.data(), w.data(), planar};
    // what every entry point derives from its arguments: the library's own search_derive (csrc/pfslam_search.hip.inc), cut out with the kernels
    SearchParams p;
    SearchWhy why;
    const SearchRefusal no = search_derive(fl[5], nb, &fl[0], hd[4], hd[5], hd[6], hd[7], fl[3], fl[4], &p, &why);
    if (no != SEARCH_FITS) return no == SEARCH_QCAP ? 5 : 6;
    const long long nx = 2LL * p.hx + 1, ny = 2LL * p.hy + 1, na = 2LL * p.ht + 1;
    int top = 0;
    while (top < PF_WIDE_MAX_LEVEL && (1LL << top) < std::max(nx, ny)) top++;
    const long long n_top = na * (((nx - 1) >> top) + 1) * (((ny - 1) >> top) + 1);
    const size_t level = (size_t)p.cap + 2;
    // exact sizes: the sanitizer sees any overrun
    std::vector<uint16_t> field(level * (size_t)(top + 1), 0xdead);
    std::vector<int2> ends((size_t)na * nb, int2{7, 7});
    std::vector<int> nin((size_t)na, -7), nodes_buf((size_t)room * (size_t)(top + 1), -7), lb((size_t)room, -7);
    unsigned long long state[4];
    memset(state, 0xff, 24);
    unsigned long long *key = state;
    int *box = (int *)(state + 1);
    int *count = (int *)(state + 3);
    std::vector<float> out(PF_SEARCH_OUT, -1.0f);
    launch_threads((int)na, 256, [&] { k_search_ends(scan.data(), p, trig, ends.data(), nin.data(), box); });
    const int cell_blocks = (p.cap + 255) / 256;
    launch_serial(cell_blocks, 256, [&] { k_search_field(tree, p, box, field.data()); }); // (no barrier, no shuffle: the threads of a workgroup one after the other)
    for (int L = 1; L <= top; L++)
        launch_serial(cell_blocks, 256, [&] { k_wide_pyramid(box, p, (1 << (L - 1)) * p.stride, field.data() + level * (size_t)(L - 1), field.data() + level * (size_t)L); });
    long long have[PF_WIDE_MAX_LEVEL + 1] = {0}, done[PF_WIDE_MAX_LEVEL + 1] = {0};
    long long bounded = 0, scored = 0, batches = 0;
    have[top] = n_top;
    for (int L = top;;) {
        if (done[L] >= have[L]) {
            if (L == top) break;
            L++;
            continue;
        }
        const int n = (int)std::min<long long>(have[L] - done[L], L ? std::max(room / 4, 1) : room);
        int *nodes = nodes_buf.data() + (size_t)room * (size_t)L;
        if (L == top) {
            launch_serial((n + 255) / 256, 256, [&] { k_wide_top(p, L, done[L], n, nodes); });
        } else {
            nodes += done[L];
        }
        done[L] += n;
        batches++;
        (L ? bounded : scored) += n;
        const uint16_t *fL = field.data() + level * (size_t)L;
        if (L) launch_threads(n, 64, [&] { k_wide_score<false>(nodes, ends.data(), nin.data(), box, field.data(), fL, p, lb.data(), key); });
        else launch_threads(n, 64, [&] { k_wide_score<true>(nodes, ends.data(), nin.data(), box, field.data(), fL, p, lb.data(), key); });
        if (L == 0) continue;
        *count = 0;
        launch_threads((n + 255) / 256, 256, [&] { k_wide_expand(nodes, lb.data(), n, L, p, key, nodes_buf.data() + (size_t)room * (size_t)(L - 1), count); });
        const int kids = *count;
        if (kids < 0 || kids > 4 * n) return 8;
        if (kids) {
            L--;
            have[L] = kids;
            done[L] = 0;
        }
    }
    launch_serial(1, 1, [&] { k_search_result(key, nin.data(), p, out.data()); });
    const SearchBox B = search_box(box, p);
    const long long stats[8] = {state[0] == ~0ull ? -1 : (long long)(state[0] & 0xffffffffull), nx * ny * na, bounded, scored, top, batches, (long long)B.W * B.H, 0};
    f = fopen(argv[2], "wb");
    fwrite(out.data(), 4, out.size(), f);
    fwrite(stats, 8, 8, f);
    fclose(f);
    return 0;
}
