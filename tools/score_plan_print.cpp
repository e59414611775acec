// tools/score_plan_print.cpp -- the chunk plan of the round-5 frame's scan-match launch (csrc/score_plan.h), printed.
//   g++ -std=c++17 -O1 -I gpu-icp-slam_amd/csrc [-DPF_TAPER_SLOTS=.. -DPF_TAPER_DIV=..] tools/score_plan_print.cpp -o score_plan_print
//   score_plan_print N [BEAMS [LARGEST_WEIGHT]]
#include "score_plan.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    if (argc < 2) return fprintf(stderr, "usage: %s particles [beams [largest |weight|]]\n", argv[0]), 2;
    const int n = atoi(argv[1]), nb = argc > 2 ? atoi(argv[2]) : 1081;
    const float w = argc > 3 ? (float)atof(argv[3]) : 113.0f;
    const pf::ScorePlan p = pf::score_plan(n, nb, w, true);
    const int groups = (n + 63) / 64;
    printf("taper slots %d div %d | %d particles (%d groups) x %d beams, |w| <= %g: target %d waves, %d chunks -> %d waves%s%s\n  sizes:", PF_TAPER_SLOTS,
           PF_TAPER_DIV, n, groups, nb, (double)w, pf::score_plan_target(n), p.used, groups * p.used, p.tapered ? "" : " (uniform)", p.p16_ok ? "" : " (not a round-5 frame)");
    for (int k = 0; k < p.used;) { // run-length: "26 x 37" = 37 chunks of 26 beams
        int r = k;
        while (r < p.used && p.starts[(size_t)r + 1] - p.starts[(size_t)r] == p.starts[(size_t)k + 1] - p.starts[(size_t)k]) r++;
        printf(" %d x %d,", p.starts[(size_t)k + 1] - p.starts[(size_t)k], r - k);
        k = r;
    }
    printf("\n");
    return 0;
}
