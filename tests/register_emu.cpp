// The text of the pfslam_nearest / pfslam_register kernels (csrc/pfslam_register.hip.inc, with wave_sum_canonical and the svd3 block of
// csrc/pfslam_stages.hip.inc it reuses, cut out by tests/test_register_kernel_text.py) run on the CPU behind tests/simt_shim.h, every
// buffer at its exact size so that a sanitizer build sees any overrun.  TEST INFRASTRUCTURE, not product code.
#include "simt_shim.h"
#include "kernel_text.inc"

// usage: register_emu IN.bin OUT.bin
//   IN  = int32 {n_nodes, planar, nb, nq, use_start, trig, 0, 0}, hot[n] (16 B), z[n], parent[n], w[n], scan[nb], queries[nq * 3],
//         the eight 32-bit words of pfslam_register_opts, start[3]
//   OUT = nb > 0: the 12 + 8 * max_iters floats of k_register's `out`; then nq > 0: best[nq] (int32), d2[nq], visits[nq] (uint32)
int main(int argc, char **argv) {
    if (argc < 3) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const auto hd = rd<int>(f, 8);
    const int n = hd[0], planar = hd[1], nb = hd[2], nq = hd[3], use_start = hd[4], trig = hd[5];
    const auto hot = rd<uint4>(f, n);
    const auto z = rd<float>(f, n);
    const auto parent = rd<int>(f, n);
    const auto w = rd<float>(f, n);
    const auto scan = rd<float>(f, nb);
    const auto q = rd<float>(f, (size_t)nq * 3);
    RegOpts o;
    if (fread(&o, sizeof(o), 1, f) != 1) return 2;
    const auto start = rd<float>(f, 3);
    fclose(f);
    const pf::KdView tree{hot.data(), z.data(), parent.data(), w.data(), planar};
    f = fopen(argv[2], "wb");
    if (nb > 0) {
        std::vector<float4> tar(nb), cor(nb);                     // exact sizes: the sanitizer sees any overrun
        std::vector<float> out((size_t)PF_REG_OUT_HEAD + 8 * (size_t)o.max_iters, -1.0f), pose(start.begin(), start.end());
        pose.push_back(0.0f);
        if (planar)
            launch_threads(1, 1024, [&] { k_register<true>(scan.data(), nb, pose.data(), start[0], start[1], start[2], use_start, tree, o, trig, tar.data(), cor.data(), out.data()); });
        else
            launch_threads(1, 1024, [&] { k_register<false>(scan.data(), nb, pose.data(), start[0], start[1], start[2], use_start, tree, o, trig, tar.data(), cor.data(), out.data()); });
        fwrite(out.data(), 4, out.size(), f);
    }
    if (nq > 0) {
        std::vector<int> best(nq, -7);
        std::vector<float> d2(nq, -1.0f);
        std::vector<unsigned> visits(nq, 0);
        launch_serial((nq + 255) / 256, 256, [&] { k_nearest(q.data(), nq, tree, best.data(), d2.data()); });   // (no barrier in k_nearest)
        for (int i = 0; i < nq; i++) {                           // the counting instantiation of the same search: node evaluations per query
            float d;
            const int bi = pf::kd_nearest_exact<true>(tree, q[3 * i], q[3 * i + 1], q[3 * i + 2], &d, &visits[i]);
            if (bi != best[i]) { fprintf(stderr, "counting search disagrees at query %d\n", i); return 3; }
        }
        fwrite(best.data(), 4, nq, f); fwrite(d2.data(), 4, nq, f); fwrite(visits.data(), 4, nq, f);
    }
    fclose(f);
    return 0;
}
