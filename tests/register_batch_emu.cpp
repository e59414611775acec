// The text of the pfslam_register_batch kernel (csrc/pfslam_register_batch.hip.inc behind the text of csrc/pfslam_register.hip.inc it
// reuses, cut out by tests/test_register_batch_kernel_text.py) run on the CPU behind tests/simt_shim.h: the DYNAMIC LDS is a heap buffer
// of exactly the bytes the launch requests, every other buffer has its exact size, so that a sanitizer build sees any overrun.  The
// workgroups of a launch run one after the other.  TEST INFRASTRUCTURE, not product code.
#include "simt_shim.h"
#include "kernel_text.inc"

// usage: register_batch_emu IN.bin OUT.bin
//   IN  = int32 {n_nodes, planar, nb, m, threads (256 or 1024), trig, 0, 0}, hot[n] (16 B), z[n], parent[n], w[n], scan[nb],
//         the eight 32-bit words of pfslam_register_opts, starts[m * 3]
//   OUT = the m x 12 floats of k_register_batch's `out`
int main(int argc, char **argv) {
    if (argc < 3) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const auto hd = rd<int>(f, 8);
    const int n = hd[0], planar = hd[1], nb = hd[2], m = hd[3], nt = hd[4], trig = hd[5];
    const auto hot = rd<uint4>(f, n);
    const auto z = rd<float>(f, n);
    const auto parent = rd<int>(f, n);
    const auto w = rd<float>(f, n);
    const auto scan = rd<float>(f, nb);
    RegOpts o;
    if (fread(&o, sizeof(o), 1, f) != 1) return 2;
    const auto starts = rd<float>(f, (size_t)m * 3);
    fclose(f);
    if (nt != 256 && nt != 1024) return 4;
    const pf::KdView tree{hot.data(), z.data(), parent.data(), w.data(), planar};
    std::vector<float> out((size_t)PF_REGB_OUT * m, -1.0f);   // exact sizes: the sanitizer sees any overrun
    const size_t lds = (size_t)nb * 8 * sizeof(float);       // what pfslam_register_batch requests
    for (int row = 0; row < m; row++) {
        g_dyn_lds = (float *)malloc(lds);                      // (a fresh, uninitialised buffer per workgroup, as on the device)
        auto go = [&](auto kern) { launch_threads(1, nt, [&] { kern(scan.data(), nb, starts.data(), tree, o, trig, out.data()); }, row); };
        if (planar && nt == 256) go(k_register_batch<true, 256>);
        else if (planar) go(k_register_batch<true, 1024>);
        else if (nt == 256) go(k_register_batch<false, 256>);
        else go(k_register_batch<false, 1024>);
        free(g_dyn_lds);
    }
    f = fopen(argv[2], "wb");
    fwrite(out.data(), 4, out.size(), f);
    fclose(f);
    return 0;
}
