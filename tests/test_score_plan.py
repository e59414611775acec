"""csrc/score_plan.h, the chunk plan of a scoring pass, checked on the CPU: tests/score_plan_check.cpp includes the header, is built as a
stand-alone program with -fsanitize=address,undefined and run; Python never loads it.

For every particle count below 4200, and above that in steps of 61 up to 200 000 with 26 214, 31 040 .. 31 110, 40 000, 65 536, 65 537 and
100 000 among them, for 1, 2, 63, 64, 65, 1081 and 4096 beams and a largest |weight| of 1, 113, 3000 and 40000, the program checks that
  * the starts increase strictly from 0 to the beam count, the sizes never increase, there are no more chunks than beams;
  * the largest chunk x the largest |weight| fits 32767, or the plan says that it is not fit for the round-5 frame (p16_ok);
  * waves = groups x chunks is at most 1.25 x the target -- unless the 16-bit bound asks for shorter chunks than the target's, then the map's
    weights decide -- and at least the target where the chunks are not all of one size; a uniform plan is required to be the plan from
    before the taper, whose ceil(nb / ceil(nb / chunks)) reaches `chunks` only where the beam count divides that way, so there the lower
    bound is asked for where it does;
  * below the threshold (uniform chunks of fewer than 8 beams) the plan is the uniform one from before the taper, restated in the
    checker and again below; with the taper switched off it is that plan above the threshold too;
  * the taper is there (first chunk longer than the last) at 32 000, 40 000, 65 537 and 100 000 particles, 1081 beams, |weight| 113.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpu-icp-slam_amd", "csrc")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("score_plan") / "score_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-I", CSRC,
                           os.path.join(ROOT, "tests", "score_plan_check.cpp"), "-o", exe])
    return exe


def plan(checker, n, nb, w):
    out = subprocess.run([checker, str(n), str(nb), str(w)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    head, starts = out.stdout.splitlines()[:2]
    used, bpc, tapered, p16_ok, chunks = [int(v) for v in head.split()]
    return {"used": used, "bpc": bpc, "tapered": bool(tapered), "p16_ok": bool(p16_ok), "chunks": chunks, "starts": [int(v) for v in starts.split()]}


def uniform(n, nb):
    """the plan from before the taper: (bpc, used)"""
    groups = (n + 63) // 64
    target = max(24576, min(65536, groups * 160))
    chunks = max(1, min((target + groups - 1) // groups, nb))
    bpc = (nb + chunks - 1) // chunks
    return bpc, (nb + bpc - 1) // bpc


def test_every_plan_holds_its_properties(checker):
    out = subprocess.run([checker], capture_output=True, text=True)
    print(out.stdout[-500:])
    assert out.returncode == 0 and " 0 failed" in out.stdout, out.stdout[-1000:] + out.stderr[-4000:]


@pytest.mark.parametrize("n", [1, 64, 65, 1000, 4608, 5825, 10000, 20000, 26214])
def test_short_chunks_stay_uniform(checker, n):
    for nb in (1, 65, 1081, 4096):
        p = plan(checker, n, nb, 113)
        bpc, used = uniform(n, nb)
        if bpc < 8:
            assert not p["tapered"] and (p["bpc"], p["used"]) == (bpc, used), (n, nb, p)
            assert p["starts"] == [min(nb, k * bpc) for k in range(used + 1)]


@pytest.mark.parametrize("n", [32000, 40000, 65537, 100000])
def test_the_taper_is_active_where_chunks_are_long(checker, n):
    p = plan(checker, n, 1081, 113)
    sizes = [b - a for a, b in zip(p["starts"], p["starts"][1:])]
    print(n, p["used"], sizes)
    assert uniform(n, 1081)[0] >= 8
    assert p["tapered"] and p["p16_ok"] and sizes[0] > sizes[-1] and sizes == sorted(sizes, reverse=True) and sum(sizes) == 1081
    assert sizes[0] <= uniform(n, 1081)[0] and sizes[-1] >= 1


def test_large_weights_shorten_the_chunks_instead_of_leaving_the_frame(checker):
    """100 000 particles on a map whose weights reach 3000: at most 10 beams per chunk (10 x 3000 <= 32767 < 11 x 3000)"""
    p = plan(checker, 100000, 1081, 3000)
    assert p["p16_ok"] and p["bpc"] == 10 and p["used"] >= 109, p
    assert not plan(checker, 100000, 1081, 40000)["p16_ok"]
