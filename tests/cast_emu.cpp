// The text of the pfslam_cast kernels (csrc/pfslam_cast.hip.inc, cut out by tests/test_cast_kernel_text.py) run on the CPU behind
// tests/simt_shim.h: k_cast_box, k_cast_count and k_cast_rays, which have shuffles, a thread per GPU thread; k_cast_splat and
// k_cast_expand, whose threads meet nowhere but in atomics, one thread after the other.  Every buffer has exactly the size the entry points
// request, so that a sanitizer build sees any overrun.  TEST INFRASTRUCTURE, not product code.
#include "simt_shim.h"
#include "kernel_text.inc"

// usage: cast_emu IN.bin OUT.bin
//   IN  = int32 {nb, trig, m, nodes, inflate, skip_cells, 0, 0}, float {res_x, res_y, max_range, w_min, no_hit, 0, 0, 0},
//         nodes x {x, y, z, w}, m x {x, y, theta}
//   OUT = int64 stats[8] of pfslam_cast, m * nb ranges, m * nb x 2 cells; the same two arrays and an int32 hit count of the plain walk
//         (k_cast_rays<false>); then pfslam_map_raster's W * H bytes
int main(int argc, char **argv) {
    if (argc < 3) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const auto hd = rd<int>(f, 8);
    const auto fl = rd<float>(f, 8);
    const int nb = hd[0], m = hd[2], nn = hd[3];
    const auto nodes = rd<float>(f, (size_t)nn * 4);
    const auto poses = rd<float>(f, (size_t)m * 3);
    fclose(f);
    CastParams p;
    p.res_x = fl[0]; p.res_y = fl[1]; p.max_range = fl[2]; p.w_min = fl[3]; p.no_hit = fl[4];
    p.inflate = hd[4]; p.skip = hd[5]; p.nb = nb; p.trig = hd[1];
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
    launch_threads(nblk, 256, [&] { k_cast_box(hot.data(), w.data(), nn, p, st.data()); });
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
        launch_serial(nblk, 256, [&] { k_cast_splat(hot.data(), w.data(), nn, p, B, tiles.data()); });
        launch_threads((int)((ntiles + 255) / 256), 256, [&] { k_cast_count(tiles.data(), (int)ntiles, st.data()); });
    }
    const int rays = m * nb;
    std::vector<float> ranges((size_t)rays, -7.0f);
    std::vector<int> cells((size_t)2 * rays, -7);
    std::vector<float> ranges_plain((size_t)rays, -7.0f);
    std::vector<int> cells_plain((size_t)2 * rays, -7);
    launch_threads((rays + 255) / 256, 256, [&] { k_cast_rays<false>(poses.data(), rays, p, B, tiles.data(), ranges_plain.data(), cells_plain.data(), st.data()); });
    const int hits_plain = st[6];
    st[6] = 0;
    launch_threads((rays + 255) / 256, 256, [&] { k_cast_rays<true>(poses.data(), rays, p, B, tiles.data(), ranges.data(), cells.data(), st.data()); });
    const size_t ncell = (size_t)B.W * B.H;
    std::vector<uint8_t> occ(ncell, 7);
    if (ncell) launch_serial((int)((ncell + 255) / 256), 256, [&] { k_cast_expand(tiles.data(), B, occ.data()); });
    const int64_t stats[8] = {rays, st[6], st[4], st[5], B.x0, B.y0, B.W, B.H};
    f = fopen(argv[2], "wb");
    fwrite(stats, 8, 8, f);
    fwrite(ranges.data(), 4, ranges.size(), f);
    fwrite(cells.data(), 4, cells.size(), f);
    fwrite(ranges_plain.data(), 4, ranges_plain.size(), f);
    fwrite(cells_plain.data(), 4, cells_plain.size(), f);
    fwrite(&hits_plain, 4, 1, f);
    fwrite(occ.data(), 1, occ.size(), f);
    fclose(f);
    return 0;
}
