// The text of the pfslam_estimate kernels (csrc/pfslam_stages.hip.inc, cut out by tests/test_estimate_kernel_text.py) run on the CPU behind
// tests/simt_shim.h, the buffers at their exact sizes so that a sanitizer build sees any overrun.  TEST INFRASTRUCTURE, not product code.
#include "simt_shim.h"
#include "kernel_text.inc"

// usage: estimate_emu GN WORLD IN.bin OUT.bin   IN = gw[world * stride] then gpose[world][3][stride] as float32, OUT = the 16 floats
int main(int argc, char **argv) {
    const int gn = atoi(argv[1]), world = atoi(argv[2]);
    const int stride = (gn + world - 1) / world;
    std::vector<float> gw((size_t)world * stride), gpose((size_t)world * 3 * stride);   // exact sizes: the sanitizer sees any overrun
    FILE *f = fopen(argv[3], "rb");
    if (fread(gw.data(), 4, gw.size(), f) != gw.size() || fread(gpose.data(), 4, gpose.size(), f) != gpose.size()) return 2;
    fclose(f);
    const int nt = (gn + PF_SUM_TILE - 1) / PF_SUM_TILE;
    std::vector<float> scratch((size_t)11 * nt + 16, -1.0f);
    float *part = scratch.data(), *res = part + (size_t)11 * nt;
    if (nt == 1) {
        launch_threads(1, 384, [&] { k_estimate_small(gw.data(), gpose.data(), stride, gn, part, res); });
    } else {
        launch_threads(nt, 384, [&] { k_estimate_moments(gw.data(), gpose.data(), stride, gn, part, nt); });
        launch_threads(nt, 384, [&] { k_estimate_centred(gw.data(), gpose.data(), stride, gn, part, part + (size_t)5 * nt, nt); });
        launch_threads(1, 64, [&] { k_estimate_final(part, nt, gn, res); });
    }
    f = fopen(argv[4], "wb"); fwrite(res, 4, 16, f); fclose(f);
    return 0;
}
