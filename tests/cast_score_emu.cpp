// The text of the pfslam_cast_score kernel (csrc/pfslam_cast_score.hip.inc) behind that of the cast kernels it stands on
// (csrc/pfslam_cast.hip.inc), cut out by tests/test_cast_score_kernel_text.py, run on the CPU behind tests/simt_shim.h.  Every buffer has
// exactly the size the entry point requests, so that a sanitizer build sees any overrun.  TEST INFRASTRUCTURE, not product code.
#include "simt_shim.h"
#include "kernel_text.inc"

// usage: cast_score_emu IN.bin OUT.bin
//   IN  = int32 {nb, trig, m, nodes, inflate, skip_cells, soa, stride, count_miss, qcap, want_classes, 0},
//         float {res_x, res_y, max_range, w_min, tol, u, z_min, z_max}, nodes x {x, y, z, w},
//         the poses: m x {x, y, theta} (soa 0), or the block [x | y | theta] of 3 * stride floats (soa 1, stride >= m), nb scan ranges
//   OUT = for the jumping walk (k_cast_score<true>), then for the plain walk: int64 stats[8] of pfslam_cast_score, m x 8 rows,
//         m * nb class bytes (only with want_classes)
int main(int argc, char **argv) {
    if (argc < 3) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const auto hd = rd<int>(f, 12);
    const auto fl = rd<float>(f, 8);
    const int nb = hd[0], m = hd[2], nn = hd[3], soa = hd[6], stride = hd[7], want_classes = hd[10];
    if (soa && stride < m) return 3;
    const auto nodes = rd<float>(f, (size_t)nn * 4);
    const auto poses = rd<float>(f, soa ? (size_t)3 * stride : (size_t)3 * m);
    const auto scan = rd<float>(f, (size_t)nb);
    fclose(f);
    CastParams p;
    p.res_x = fl[0]; p.res_y = fl[1]; p.max_range = fl[2]; p.w_min = fl[3]; p.no_hit = 0.0f;
    p.inflate = hd[4]; p.skip = hd[5]; p.nb = nb; p.trig = hd[1];
    CastScoreParams s;
    s.tol = fl[4]; s.u = fl[5]; s.z_min = fl[6]; s.z_max = fl[7];
    s.qcap = hd[9]; s.count_miss = hd[8];
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
    // what pfslam_cast_score does: the pose list through (base, base + 1, base + 2) and stride 3, the particle block through its three
    // arrays and stride 1
    const float *px = poses.data(), *py = soa ? px + stride : px + 1, *pth = soa ? px + 2 * stride : px + 2;
    const int ps = soa ? 1 : 3;
    const size_t rays = (size_t)m * nb;
    const int blocks = (int)((rays + 255) / 256);
    f = fopen(argv[2], "wb");
    for (int jump = 1; jump >= 0; jump--) {
        std::vector<int> rows((size_t)m * PF_CAST_SCORE_ROW, 0); // (the entry point clears them)
        std::vector<uint8_t> classes(want_classes ? rays : 0, 7);
        uint8_t *cl = want_classes ? classes.data() : nullptr;
        if (jump) launch_threads(blocks, 256, [&] { k_cast_score<true>(px, py, pth, ps, scan.data(), (int)rays, p, s, B, tiles.data(), rows.data(), cl); });
        else launch_threads(blocks, 256, [&] { k_cast_score<false>(px, py, pth, ps, scan.data(), (int)rays, p, s, B, tiles.data(), rows.data(), cl); });
        // as the entry point does: the hits leave the rows for stats[1], the cost takes their place
        int64_t hits = 0;
        for (int r = 0; r < m; r++) {
            int *row = &rows[(size_t)r * PF_CAST_SCORE_ROW];
            hits += row[7];
            row[7] = row[5] + (s.count_miss ? s.qcap * row[4] : 0);
        }
        const int64_t stats[8] = {(int64_t)rays, hits, st[4], st[5], B.x0, B.y0, B.W, B.H};
        fwrite(stats, 8, 8, f);
        fwrite(rows.data(), 4, rows.size(), f);
        fwrite(classes.data(), 1, classes.size(), f);
    }
    fclose(f);
    return 0;
}
