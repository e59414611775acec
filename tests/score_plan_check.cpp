// score_plan_check.cpp -- tests/test_score_plan.py's stand-alone checker of csrc/score_plan.h (built with -fsanitize=address,undefined).
// TEST INFRASTRUCTURE, not product code.
//   score_plan_check              every property below over the particle, beam and weight counts of the test; exit status 0 = all hold
//   score_plan_check n nb w       prints the plan: "used bpc tapered p16_ok chunks" and the starts
#include "score_plan.h"

#include <cstdio>
#include <cstdlib>
#include <set>

static int g_failed = 0;
#define EXPECT(cond, ...)                                   \
    do {                                                    \
        if (!(cond)) {                                      \
            if (g_failed++ < 20) {                          \
                fprintf(stderr, "FAILED %s: ", #cond);      \
                fprintf(stderr, __VA_ARGS__);               \
                fprintf(stderr, "\n");                      \
            }                                               \
        }                                                   \
    } while (0)

// The uniform plan as every launch cut its beams before the taper, restated (not included) from the parent's score_chunks, launch_score
// and frame_v2_ok: target waves, chunks per group, beams per chunk, chunks used.
static void uniform_restated(int n, int nb, int *target, int *chunks, int *bpc, int *used)
{
    const int groups = (n + 63) / 64;
    int t = groups * 160;
    if (t > 65536) t = 65536;
    if (t < 24576) t = 24576;
    int c = (t + groups - 1) / groups;
    if (c > nb) c = nb;
    if (c < 1) c = 1;
    *target = t;
    *chunks = c;
    *bpc = (nb + c - 1) / c;
    *used = (nb + *bpc - 1) / *bpc;
}

static void check(int n, int nb, float w)
{
    const pf::ScorePlan p = pf::score_plan(n, nb, w, true);
    int target, chunks, ubpc, uused;
    uniform_restated(n, nb, &target, &chunks, &ubpc, &uused);
    const int groups = (n + 63) / 64;
#define AT "n %d nb %d w %g: used %d bpc %d tapered %d", n, nb, (double)w, p.used, p.bpc, (int)p.tapered
    EXPECT(p.used >= 1 && (int)p.starts.size() == p.used + 1, AT);
    if (p.used < 1 || (int)p.starts.size() != p.used + 1) return;
    EXPECT(p.starts[0] == 0 && p.starts[(size_t)p.used] == nb, AT);
    int largest = 0;
    for (int k = 0; k < p.used; k++) {
        const int size = p.starts[(size_t)k + 1] - p.starts[(size_t)k];
        EXPECT(size >= 1, AT);                                                                        // starts strictly increase
        if (k > 0) EXPECT(size <= p.starts[(size_t)k] - p.starts[(size_t)k - 1], AT);                 // sizes never increase
        largest = std::max(largest, size);
    }
    EXPECT(p.used <= nb, AT);
    EXPECT(largest == p.bpc, AT);
    // the 16-bit bound, or "not a round-5 frame"
    const bool fits = (float)largest * w <= 32767.0f;
    EXPECT(p.p16_ok == (fits && p.used >= 2), AT);
    // below the threshold: today's plan exactly
    const bool long_chunks = ubpc >= 8;
    if (!long_chunks) {
        EXPECT(!p.tapered && p.bpc == ubpc && p.used == uused, AT);
        for (int k = 0; k <= p.used; k++) EXPECT(p.starts[(size_t)k] == std::min(nb, k * ubpc), AT);
    }
    // waves = groups x used against the target.  "Whenever nb allows it" is made precise here:
    //   upper bound, 1.25 x target: always, unless the 16-bit bound asks for chunks shorter than the uniform plan's (then the map's
    //     weights decide the chunk count, not the target)
    //   lower bound, target: whenever the chunks are not all of one size.  A uniform plan reaches ceil(target / groups) chunks only where nb
    //     divides into that many (bpc = ceil(nb / chunks) rounds up, used = ceil(nb / bpc) comes out smaller -- 1081 beams in 120 chunks:
    //     bpc 10, used 109), and it is required to be today's plan, so there the bound holds where used == chunks
    const long long waves = (long long)groups * p.used;
    const bool weight_bound = long_chunks && (float)ubpc * w > 32767.0f;
    if (!weight_bound) EXPECT(4 * waves <= 5LL * target, AT);
    if (p.tapered || p.used == (target + groups - 1) / groups) EXPECT(waves >= target, AT);
    if (p.tapered) EXPECT(p.used >= uused, AT);
    // long chunks and the taper switched off: today's plan too, unless the 16-bit bound shortens the chunks
    if (long_chunks && !weight_bound) {
        const pf::ScorePlan q = pf::score_plan(n, nb, w, true, /*taper_slots=*/0);
        EXPECT(!q.tapered && q.bpc == ubpc && q.used == uused, AT);
    }
    // other map weights: one chunk
    const pf::ScorePlan o = pf::score_plan(n, nb, w, false);
    EXPECT(o.used == 1 && o.bpc == nb && !o.tapered && !o.p16_ok && o.starts.size() == 2 && o.starts[0] == 0 && o.starts[1] == nb, AT);
    EXPECT(pf::score_plan_chunks(n, nb, true) == chunks && pf::score_plan_chunks(n, nb, false) == 1, AT);
#undef AT
}

int main(int argc, char **argv)
{
    if (argc == 4) {
        const pf::ScorePlan p = pf::score_plan(atoi(argv[1]), atoi(argv[2]), (float)atof(argv[3]), true);
        printf("%d %d %d %d %d\n", p.used, p.bpc, (int)p.tapered, (int)p.p16_ok, p.chunks);
        for (int s : p.starts) printf("%d ", s);
        printf("\n");
        return 0;
    }
    std::set<int> ns;
    for (int n = 1; n < 4200; n++) ns.insert(n);
    for (int n = 4200; n <= 200000; n += 61) ns.insert(n);
    for (int n = 31040; n <= 31110; n++) ns.insert(n);
    for (int n : {26214, 26215, 32000, 40000, 65536, 65537, 100000, 199999, 200000}) ns.insert(n);
    const int nbs[] = {1, 2, 63, 64, 65, 1081, 4096};
    const float ws[] = {1.0f, 113.0f, 3000.0f, 40000.0f};
    long long plans = 0;
    for (int n : ns)
        for (int nb : nbs)
            for (float w : ws) {
                check(n, nb, w);
                plans++;
            }
    // the taper is really there where the flagship runs
    for (int n : {32000, 40000, 65537, 100000}) {
        const pf::ScorePlan p = pf::score_plan(n, 1081, 113.0f, true);
        EXPECT(p.tapered && p.used >= 2 && p.starts[1] - p.starts[0] > p.starts[(size_t)p.used] - p.starts[(size_t)p.used - 1],
               "n %d: used %d bpc %d tapered %d", n, p.used, p.bpc, (int)p.tapered);
    }
    printf("%lld plans checked, %d failed, taper slots %d div %d\n", plans, g_failed, PF_TAPER_SLOTS, PF_TAPER_DIV);
    return g_failed ? 1 : 0;
}
