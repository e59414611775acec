// replay_main.cpp -- headless counterpart of the reference's main loop (main.cpp:47-96, 175-229):
//   pfslam_replay <scene.txt> <lidar.f32|.mat> [frames] [grid] [loop] [resampler=N] [estimate=1] [register=K] [multistart=K] [search=1|2|3] [odometry=1|2] [cast=1] [castscore=1] [export=PREFIX]
//     grid           the 2-D occupancy-grid stages instead of the point-cloud ones
//     loop           UpdateTopology + CheckLoopClosure at the end of every frame (kernel.cu:1750-1751, commented out in
//                    the reference's shipped step); loop-closure proposals are printed per frame
//     resampler=N    PFResample's draw (pfslamSetResampler): 0 the reference's seeding (default), 1 per-particle seeds, 2 systematic
//     estimate=1     a second line per frame: the cloud's weighted mean pose, the six covariance entries (xx xy xt yy yt tt) and Neff
//                    (pfslamPoseEstimate), as decimals and as float bits
//     register=K     a further line per frame: the pose pfslamRegister reaches from the frame's pose in at most K iterations (the frame's scan
//                    against the frame's map; the filter is not changed), its status and iteration count, as decimals and as float bits
//     multistart=K   a further line per frame: pfslamRegisterBatch from the nine starts frame's pose + (dx, dy, 0), dx, dy in {-0.1, 0, 0.1} m
//                    (row = 3 * index of dx + index of dy), at most K iterations each: the row it picks and that row's pose, as decimals
//                    and as float bits ("best -1" and no pose when no run completed an iteration)
//     search=1       a further line per frame: pfslamSearch with the default window around the frame's pose: the candidate it picks and
//                    that candidate's pose, as decimals and as float bits
//     search=2       instead a line "search_wide ..." per frame: pfslamSearchWide over +-20 m and a full turn (+-3.14159 rad) around the
//                    frame's pose, in the same form
//     search=3       instead the lines "search_best <frame> <row> index <k> pose ... bits ..." per frame, one per row: pfslamSearchBest over the
//                    same window, eight rows wanted ("search_best <frame> none" when the call fails or finds no row)
//     odometry=1     lidar-only odometry: before every frame after the first, pfslamSearchScan of the new scan against the previous scan at
//                    the previous frame's pose (the default window around it); a line "odometry <frame> index <k> delta <dx dy dtheta> bits
//                    <3 hex words of the winning pose>" and pfslamShiftParticles with that delta before the step ("odometry <frame> none"
//                    and no shift when the call fails or no heading has an in-range beam)
//     odometry=2     instead the motion model: pfslamSearchScanCov of the same two scans (the library's default sigma) and
//                    pfslamMoveParticles(frame, delta, cov + 3, the previous pose's heading) with the floors res / sqrt(12) and
//                    step_theta / sqrt(12) of the search's lattice; a line "odometry <frame> index <k> delta <dx dy dtheta> sd <the square
//                    roots of the covariance's three diagonal entries> bits <3 hex words of the winning pose>" ("odometry <frame> none" and
//                    no move when a call fails or no heading has an in-range beam)
//     cast=1         a further line per frame: "cast <frame> hits <n> agree <k>": pfslamCastScan from the frame's pose through the frame's map,
//                    the beams that hit, and the beams whose cast range is within 0.1 m of the scan's ("cast <frame> none" when the call fails or
//                    the scan does not have the filter's 1081 beams)
//     castscore=1    a further line per frame: "castscore <frame> valid <n> agree <a> through <t> short <s> miss <m> cost <c>": pfslamCastScore of
//                    the frame's pose, the frame's scan against the frame's map ("castscore <frame> none" when the call fails)
//     export=PREFIX  after the last frame: the map as the reference's viewer filters it (KD nodes with w > -100,
//                    main.cpp:269-284) and the occupancy grid -> PREFIX.kd.bin / .kd.csv / .grid.i8 / .grid.pgm
// iteration 0: Free + Init; then particleFilter(pbo=NULL, ++iteration, lidar) until the scans run out.
// Prints one line per frame (pose, map size) and the mean step time.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "kernel.h"

int main(int argc, char **argv)
{
    if (argc < 3) {
        printf("Usage: %s SCENEFILE.txt LIDARFILE.f32|.mat [frames] [grid] [loop] [resampler=N] [estimate=1] [register=K] [multistart=K] [search=1|2|3] [odometry=1|2] [cast=1] [castscore=1] [export=PREFIX]\n", argv[0]);
        return 1;
    }
    Scene *scene = new Scene(argv[1]);
    Lidar *lidar = new Lidar(argv[2]);
    size_t last = lidar->scans.size() - 1;
    bool loop = false, estimate = false;
    int register_iters = 0, multistart_iters = 0, search = 0;
    int odometry = 0;
    bool cast = false, castscore = false;
    std::string export_prefix;
    for (int i = 3; i < argc; i++) {
        if (strcmp(argv[i], "grid") == 0) pfslamUseGridMap(true);
        else if (strcmp(argv[i], "loop") == 0) loop = true;
        else if (strncmp(argv[i], "resampler=", 10) == 0) pfslamSetResampler(atoi(argv[i] + 10));
        else if (strncmp(argv[i], "estimate=", 9) == 0) estimate = atoi(argv[i] + 9) != 0;
        else if (strncmp(argv[i], "register=", 9) == 0) register_iters = atoi(argv[i] + 9);
        else if (strncmp(argv[i], "multistart=", 11) == 0) multistart_iters = atoi(argv[i] + 11);
        else if (strncmp(argv[i], "search=", 7) == 0) search = atoi(argv[i] + 7);
        else if (strncmp(argv[i], "odometry=", 9) == 0) odometry = atoi(argv[i] + 9);
        else if (strncmp(argv[i], "cast=", 5) == 0) cast = atoi(argv[i] + 5) != 0;
        else if (strncmp(argv[i], "castscore=", 10) == 0) castscore = atoi(argv[i] + 10) != 0;
        else if (strncmp(argv[i], "export=", 7) == 0) export_prefix = argv[i] + 7;
        else if (atoi(argv[i]) > 0) last = std::min(last, (size_t)atoi(argv[i]));
    }
    particleFilterFree();
    particleFilterInit(scene);
    pfslamUseTopology(loop);
    double total_ms = 0;
    size_t iteration = 0, proposals = 0;
    glm::vec3 last_pose(0.0f);
    while (iteration < last) {
        iteration++;
        if (odometry == 2 && iteration > 1) {
            glm::vec3 r;
            int index = -1;
            float cov[16];
            bool moved = false;
            if (pfslamSearchScanCov(lidar->scans[iteration - 1].data(), last_pose, 0.2f, r, cov, &index, lidar->scans[iteration].data()) && index >= 0) {
                const glm::vec3 d(r.x - last_pose.x, r.y - last_pose.y, r.z - last_pose.z);
                float res = 0.025f; // pfslam_default_config
                if (!scene->maps.empty()) res = scene->maps[0].resolution.x;
                const float step_theta = 0.0125f; // pfslam_search_default_opts
                if (pfslamMoveParticles((int)iteration, d, cov + 3, last_pose.z, res / sqrtf(12.0f), step_theta / sqrtf(12.0f))) {
                    unsigned int b[3];
                    memcpy(&b[0], &r.x, 4); memcpy(&b[1], &r.y, 4); memcpy(&b[2], &r.z, 4);
                    printf("odometry %zu index %d delta %.6f %.6f %.6f sd %.6f %.6f %.6f bits %08x %08x %08x\n", iteration, index, d.x, d.y, d.z,
                           sqrtf(cov[3]), sqrtf(cov[6]), sqrtf(cov[8]), b[0], b[1], b[2]);
                    moved = true;
                }
            }
            if (!moved) printf("odometry %zu none\n", iteration);
        } else if (odometry && iteration > 1) {
            glm::vec3 r;
            int index = -1;
            if (pfslamSearchScan(lidar->scans[iteration - 1].data(), last_pose, r, &index, lidar->scans[iteration].data()) && index >= 0) {
                const glm::vec3 d(r.x - last_pose.x, r.y - last_pose.y, r.z - last_pose.z);
                unsigned int b[3];
                memcpy(&b[0], &r.x, 4); memcpy(&b[1], &r.y, 4); memcpy(&b[2], &r.z, 4);
                printf("odometry %zu index %d delta %.6f %.6f %.6f bits %08x %08x %08x\n", iteration, index, d.x, d.y, d.z, b[0], b[1], b[2]);
                pfslamShiftParticles(d);
            } else {
                printf("odometry %zu none\n", iteration);
            }
        }
        auto t0 = std::chrono::steady_clock::now();
        particleFilter(nullptr, (int)iteration, lidar);
        Particle *p; MAP_TYPE *map; KDTree::Node *kd; int np, nkd; glm::vec3 pos;
        getPCData(&p, &map, &kd, &np, &nkd, pos);
        total_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        unsigned int bx, by, bt;
        memcpy(&bx, &pos.x, 4); memcpy(&by, &pos.y, 4); memcpy(&bt, &pos.z, 4);
        last_pose = pos;
        printf("frame %zu pose %.6f %.6f %.6f bits %08x %08x %08x particles %d kd %d", iteration, pos.x, pos.y, pos.z, bx, by, bt, np, nkd);
        if (loop) {
            const auto pairs = pfslamLoopClosures();
            proposals += pairs.size();
            printf(" closures %zu", pairs.size());
            for (size_t k = 0; k < pairs.size() && k < 8; k++) printf(" (%d,%d)", pairs[k].first, pairs[k].second);
        }
        printf("\n");
        if (estimate) {
            glm::vec3 m;
            float c[9], neff = 0.0f;
            if (pfslamPoseEstimate(m, c, &neff)) {
                const float v[10] = {m.x, m.y, m.z, c[0], c[1], c[2], c[4], c[5], c[8], neff};
                printf("estimate %zu mean %.6f %.6f %.6f cov %.6e %.6e %.6e %.6e %.6e %.6e neff %.3f bits", iteration, v[0], v[1], v[2], v[3], v[4], v[5],
                       v[6], v[7], v[8], v[9]);
                for (int k = 0; k < 10; k++) {
                    unsigned int b;
                    memcpy(&b, &v[k], 4);
                    printf(" %08x", b);
                }
                printf("\n");
            } else {
                printf("estimate %zu none\n", iteration);
            }
        }
        if (register_iters > 0) {
            glm::vec3 r;
            int status = 0, iters = 0;
            if (pfslamRegister(pos, register_iters, r, &status, &iters)) {
                unsigned int b[3];
                memcpy(&b[0], &r.x, 4); memcpy(&b[1], &r.y, 4); memcpy(&b[2], &r.z, 4);
                printf("register %zu pose %.6f %.6f %.6f status %d iterations %d bits %08x %08x %08x\n", iteration, r.x, r.y, r.z, status, iters, b[0], b[1], b[2]);
            } else {
                printf("register %zu none\n", iteration);
            }
        }
        if (multistart_iters > 0) {
            const float off[3] = {-0.1f, 0.0f, 0.1f};
            glm::vec3 starts[9], poses[9];
            for (int a = 0; a < 3; a++)
                for (int b = 0; b < 3; b++) starts[3 * a + b] = glm::vec3(pos.x + off[a], pos.y + off[b], pos.z);
            int best = -1;
            if (!pfslamRegisterBatch(starts, 9, multistart_iters, poses, nullptr, &best)) {
                printf("multistart %zu none\n", iteration);
            } else if (best < 0) {
                printf("multistart %zu best -1\n", iteration);
            } else {
                const glm::vec3 r = poses[best];
                unsigned int b[3];
                memcpy(&b[0], &r.x, 4); memcpy(&b[1], &r.y, 4); memcpy(&b[2], &r.z, 4);
                printf("multistart %zu best %d pose %.6f %.6f %.6f bits %08x %08x %08x\n", iteration, best, r.x, r.y, r.z, b[0], b[1], b[2]);
            }
        }
        if (search == 1) {
            glm::vec3 r;
            int index = -1;
            if (pfslamSearch(pos, r, &index)) {
                unsigned int b[3];
                memcpy(&b[0], &r.x, 4); memcpy(&b[1], &r.y, 4); memcpy(&b[2], &r.z, 4);
                printf("search %zu index %d pose %.6f %.6f %.6f bits %08x %08x %08x\n", iteration, index, r.x, r.y, r.z, b[0], b[1], b[2]);
            } else {
                printf("search %zu none\n", iteration);
            }
        }
        if (search == 2) {
            glm::vec3 r;
            long long index = -1;
            if (pfslamSearchWide(pos, 20.0f, 3.14159f, r, &index)) {
                unsigned int b[3];
                memcpy(&b[0], &r.x, 4); memcpy(&b[1], &r.y, 4); memcpy(&b[2], &r.z, 4);
                printf("search_wide %zu index %lld pose %.6f %.6f %.6f bits %08x %08x %08x\n", iteration, index, r.x, r.y, r.z, b[0], b[1], b[2]);
            } else {
                printf("search_wide %zu none\n", iteration);
            }
        }
        if (search == 3) {
            glm::vec3 r[8];
            long long index[8];
            const int found = pfslamSearchBest(pos, 20.0f, 3.14159f, 8, r, index);
            for (int n = 0; n < found; n++) {
                unsigned int b[3];
                memcpy(&b[0], &r[n].x, 4); memcpy(&b[1], &r[n].y, 4); memcpy(&b[2], &r[n].z, 4);
                printf("search_best %zu %d index %lld pose %.6f %.6f %.6f bits %08x %08x %08x\n", iteration, n, index[n], r[n].x, r[n].y, r[n].z, b[0], b[1], b[2]);
            }
            if (found <= 0) printf("search_best %zu none\n", iteration);
        }
        if (cast) {
            std::vector<float> expected(lidar->scans[iteration].size());
            int hits = 0;
            if (expected.size() == 1081 && pfslamCastScan(pos, expected.data(), &hits)) {
                int agree = 0;
                for (size_t b = 0; b < expected.size(); b++) agree += fabsf(expected[b] - lidar->scans[iteration][b]) <= 0.1f ? 1 : 0;
                printf("cast %zu hits %d agree %d\n", iteration, hits, agree);
            } else {
                printf("cast %zu none\n", iteration);
            }
        }
        if (castscore) {
            int row[8];
            if (pfslamCastScore(&pos, 1, row, nullptr))
                printf("castscore %zu valid %d agree %d through %d short %d miss %d cost %d\n", iteration, row[0], row[1], row[2], row[3], row[4], row[7]);
            else
                printf("castscore %zu none\n", iteration);
        }
    }
    printf("mean step+readback %.3f ms over %zu frames\n", iteration ? total_ms / iteration : 0.0, iteration);
    if (loop) printf("loop-closure proposals %zu\n", proposals);
    if (!export_prefix.empty()) printf("exported %d map points to %s.*\n", pfslamExportMap(export_prefix.c_str()), export_prefix.c_str());
    particleFilterFree();
    delete lidar;
    delete scene;
    return 0;
}
