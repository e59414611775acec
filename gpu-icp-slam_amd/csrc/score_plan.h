// score_plan.h -- how a scoring pass cuts its beams into chunks (one wave per 64 particles and chunk).  Pure host code, no HIP:
// the library's launches (score_chunks, frame_v2_ok) and tests/test_score_plan.py's stand-alone checker both include it.
#pragma once

#include <algorithm>
#include <vector>

// The taper of the round-5 frame's scan-match launch: the last rows of chunks the dispatcher hands out shrink, so that the waves still
// running when it has run dry are short ones.  With 42 equal chunks of 26 beams at 100 k particles (65 646 waves on 8192 wave slots, groups
// fastest) the last-indexed wave started 69 us before the last wave ended, a whole wave's duration (54 us) and more; with the last ten rows
// shrinking to 4 beams (47 chunks: 37 of 26 / 25, then 23 22 18 17 15 13 10 8 6 4) that tail is 42 us, the kernel 0.400 -> 0.390 ms and the
// frame 0.5280 -> 0.5125 ms, every run of five against every run of five of the parent (profiles/chunk_taper_ab.txt; 40 k particles: chunks
// of 11 beams, nothing to gain and nothing lost).  The price is five more waves per group, i.e. five more prologues on 1081 beams.  The
// partials are 16-bit integers: any order of adding them is exact, so the scores are the same bits.  Other (SLOTS, DIV) pairs -- 8192 .. 24576,
// 3 .. 6 -- came out within 0.3 % of these and were not told apart by five runs each.
//   PF_TAPER_SLOTS  rows that shrink, as waves: rows = PF_TAPER_SLOTS / groups, at least 4 (16384 = two rounds of the 8192 wave slots); 0: no taper
//   PF_TAPER_DIV    the smallest chunk is 1 / PF_TAPER_DIV of the largest, at least 2 beams
#ifndef PF_TAPER_SLOTS
#define PF_TAPER_SLOTS 16384
#endif
#ifndef PF_TAPER_DIV
#define PF_TAPER_DIV 6
#endif
#define PF_TAPER_MIN_BPC 8 /* uniform chunks shorter than this stay as they are (1081 beams: below ~27 k particles) */
#define PF_P16_MAX 32767.0f /* a chunk's partial sum is stored as a 16-bit integer: beams x largest |weight| must fit */

namespace pf {

struct ScorePlan {
    int chunks = 1;          // what the target asks for: the stage-level launches cut nb into this many uniform chunks themselves
    int bpc = 0, used = 0;   // largest chunk, number of chunks
    bool tapered = false;    // false: chunk k is [k bpc, min(nb, (k + 1) bpc)), today's uniform plan -- starts says the same
    bool p16_ok = false;     // more than one chunk of integer partials and bpc x w_absmax <= 32767: fit for the round-5 frame
    std::vector<int> starts; // used + 1 entries, starts[0] = 0, starts[used] = nb
};

// The uniform plan's target: ~8 rounds of the 8192 wave slots (256 CUs x 32), fine-grained enough that the tail of the last round is
// small (measured: 16 k waves 3.33 ms, 128 k waves 2.9-3.0 ms at 100 k particles); down to one beam per chunk for small N.
// (round 5: 65 536 -- 42 chunks of 26 beams at 100 k particles.  A wave's prologue, the fp64 sincos of its 64 headings, is ~10 % of a
// 13-beam chunk, and the reduce reads half the partials: frame 0.530 -> 0.520 ms in an A/B on one box; 32 768: 0.538, 262 144: 0.569)
// Below ~40 k particles fewer, longer waves win (a wave's prologue and the launch's ramp against the beams it scores): ~160 chunks per
// group between 24 576 and 65 536 waves (profiles/r05_sweep_waves.txt: 10 k particles 0.218 -> 0.209 ms per frame, 20 k 0.2493 -> 0.2478,
// 1 k / 4 k unchanged within noise)
inline int score_plan_target(int n)
{
    const int groups = (n + 63) / 64;
    return std::max(24576, std::min(65536, groups * 160));
}
// ... and the number of uniform chunks it asks for (what a stage-level launch cuts nb into: bpc = ceil(nb / chunks), used = ceil(nb / bpc)).
// Beam-chunk partials added afterwards equal the reference's sequential beam-order float sum only when every term is an
// integer and no partial sum can pass 2^24 (any map the SLAM step builds: 0 / -100 initial, -1 / +4 steps, clamp +-113; upload_tree
// holds an uploaded map to n_beams x largest |weight| <= 2^24).  A map uploaded through pfslam_set_map with other weights is scored
// in one chunk: slower, but kernEvaluateParticlesKD's own summation order.
inline int score_plan_chunks_for(int target, int groups, int nb)
{
    if (groups < 1 || nb < 1) return 1;
    const int chunks = (target + groups - 1) / groups;
    return std::max(1, std::min(chunks, nb)); // small particle counts go down to one beam per wave
}
inline int score_plan_chunks(int n, int nb, bool integral_w)
{
    return integral_w ? score_plan_chunks_for(score_plan_target(n), (n + 63) / 64, nb) : 1;
}

inline ScorePlan score_plan(int n, int nb, float w_absmax, bool integral_w, int taper_slots = PF_TAPER_SLOTS, int taper_div = PF_TAPER_DIV)
{
    ScorePlan p;
    const int groups = (n + 63) / 64;
    if (n < 1 || nb < 1) return p;
    const int chunks = score_plan_chunks(n, nb, integral_w);
    p.chunks = chunks;
    p.bpc = (nb + chunks - 1) / chunks;
    p.used = (nb + p.bpc - 1) / p.bpc;
    auto uniform = [&]() {
        p.tapered = false;
        p.starts.resize((size_t)p.used + 1);
        for (int k = 0; k <= p.used; k++) p.starts[k] = (int)std::min<long long>(nb, (long long)k * p.bpc);
        p.p16_ok = integral_w && p.used >= 2 && (float)p.bpc * w_absmax <= PF_P16_MAX;
    };
    uniform();
    if (!integral_w || p.bpc < PF_TAPER_MIN_BPC) return p;
    // Long chunks.  The largest one the 16-bit partials allow (a map uploaded with large weights: more, shorter chunks instead of
    // another kind of frame) ...
    int body = p.bpc;
    if ((float)body * w_absmax > PF_P16_MAX) body = (int)std::min((float)body, PF_P16_MAX / w_absmax);
    if (body < 1) return p; // (p16_ok is false: one beam is too much)
    while (body > 1 && (float)body * w_absmax > PF_P16_MAX) body--;
    // ... and the last T rows shrink from it to S beams, T <= half the rows
    const int S = std::max(2, body / std::max(1, taper_div));
    int T = taper_slots > 0 && body >= PF_TAPER_MIN_BPC ? std::max(4, taper_slots / groups) : 0;
    T = std::min(T, (nb / body) / 2);
    if (T < 2) T = 0;
    if (T == 0 && body == p.bpc) return p; // today's plan
    // Row weights: body for a full row, t[i] for the i-th shrinking one (S for the last).  The rows share nb beams in proportion,
    // by rounding the running sum; sorted, the sizes never increase.  Enough full rows that none is longer than body
    // (total weight >= nb) and that the launch has the target's waves.
    std::vector<int> w;
    long long W = 0;
    for (int i = 1; i <= T; i++) {
        const int t = body - ((body - S) * i + T / 2) / T;
        w.push_back(t);
        W += t;
    }
    const int U = std::max((int)((nb - W + body - 1) / body), chunks - T);
    W += (long long)U * body;
    const int R = U + T;
    if (U < 1 || R > nb) return p;
    std::vector<int> size((size_t)R);
    long long acc = 0, prev = 0;
    for (int k = 0; k < R; k++) {
        acc += k < U ? body : w[(size_t)(k - U)];
        const long long cut = (acc * nb + W / 2) / W;
        size[(size_t)k] = (int)(cut - prev);
        prev = cut;
    }
    std::sort(size.begin(), size.end(), [](int a, int b) { return a > b; });
    if (size.back() < 1 || size.front() > body || prev != nb) return p; // (cannot happen for the sizes above; the uniform plan is always right)
    p.bpc = size.front();
    p.used = R;
    p.tapered = true;
    p.starts.assign((size_t)R + 1, 0);
    for (int k = 0; k < R; k++) p.starts[(size_t)k + 1] = p.starts[(size_t)k] + size[(size_t)k];
    p.p16_ok = R >= 2 && (float)p.bpc * w_absmax <= PF_P16_MAX;
    return p;
}

} // namespace pf
