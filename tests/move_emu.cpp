// The text of pfslam_move_particles' kernel (csrc/pfslam_move.hip.inc, cut out by tests/test_move_kernel_text.py) run on the CPU behind
// tests/simt_shim.h, the buffers at their exact sizes so that a sanitizer build sees any overrun.  TEST INFRASTRUCTURE, not product code.
#include "simt_shim.h"
#include "kernel_text.inc"

// usage: move_emu N GOFF FRAME TRIG IN.bin OUT.bin   IN = MoveParams (10 floats), pose[3], cloud[8], x[N], y[N], theta[N] as float32;
//                                                    OUT = pose[3], cloud[8], x[N], y[N], theta[N]
//        move_emu zmax STATE OUT.bin                 OUT = normal(STATE, 0, 1) in the specification's form and in the device library's
int main(int argc, char **argv) {
    if (argc == 4 && strcmp(argv[1], "zmax") == 0) {
        uint32_t a = (uint32_t)strtoul(argv[2], nullptr, 10), b = a;
        const float z[2] = {pf::normal(a, 0.0f, 1.0f, false), pf::normal(b, 0.0f, 1.0f, true)};
        FILE *f = fopen(argv[3], "wb"); fwrite(z, 4, 2, f); fclose(f);
        return 0;
    }
    const int n = atoi(argv[1]), goff = atoi(argv[2]), frame = atoi(argv[3]), trig = atoi(argv[4]);
    FILE *f = fopen(argv[5], "rb");
    std::vector<float> mp = rd<float>(f, 10), pose = rd<float>(f, 3), cloud = rd<float>(f, 8);
    std::vector<float> x = rd<float>(f, n), y = rd<float>(f, n), th = rd<float>(f, n);   // exact sizes: the sanitizer sees any overrun
    fclose(f);
    static_assert(sizeof(MoveParams) == 40, "MoveParams is ten floats");
    MoveParams m;
    memcpy(&m, mp.data(), sizeof(m));
    launch_serial((n + 255) / 256, 256, [&] { k_move(x.data(), y.data(), th.data(), n, m, frame, goff, trig, pose.data(), cloud.data()); });
    f = fopen(argv[6], "wb");
    fwrite(pose.data(), 4, 3, f); fwrite(cloud.data(), 4, 8, f);
    fwrite(x.data(), 4, n, f); fwrite(y.data(), 4, n, f); fwrite(th.data(), 4, n, f);
    fclose(f);
    return 0;
}
