"""The pfslam_estimate kernels' own text, run on the CPU (no GPU needed): tests/estimate_emu.cpp compiles the kernels cut out of
csrc/pfslam_stages.hip.inc behind a small SIMT shim (a thread per GPU thread, barriers for __syncthreads and the wave shuffles) with
-ffp-contract=off like the library, under AddressSanitizer and UBSan with every buffer at its exact size.  Unsharded and rank-major sharded
layouts must give the restatement's 16 floats bit for bit (tests/estimate_ref.py), which also shows that no index leaves a buffer and that
every thread reaches every barrier.  What it cannot show is the GPU's arithmetic and memory model: tests/test_gpu_estimate.py does."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import estimate_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gpu-icp-slam_amd", "csrc", "pfslam_stages.hip.inc")
CASES = [(1, 1, "zeros"), (64, 1, "zeros"), (65, 2, "zeros"), (4096, 3, "zeros"), (4097, 2, "one"), (4097, 1, "zeros"), (5000, 3, "zeros"),
         (8193, 3, "zeros")]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile the kernel text for the CPU")
    d = tmp_path_factory.mktemp("estimate_emu")
    src = open(SRC).read()
    cuts = [("template <typename F>\n__device__ __forceinline__ float wave_sum_canonical", "// float <-> order-preserving signed int"),
            ("#define PF_EST_WAVES", 'extern "C" int pfslam_estimate')]
    text = ""
    for first, last in cuts:
        assert src.count(first) == 1 and last in src, "the kernel text has moved: %r" % first
        text += src[src.index(first):src.index(last, src.index(first))]
    assert "k_estimate_small" in text and "k_estimate_centred" in text
    (d / "estimate_kernel_text.inc").write_text(text)
    shutil.copy(os.path.join(ROOT, "tests", "estimate_emu.cpp"), str(d / "estimate_emu.cpp"))
    exe = str(d / "estimate_emu")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-pthread", str(d / "estimate_emu.cpp"), "-o", exe])
    return d, exe


@pytest.mark.parametrize("n,world,weights", CASES)
def test_kernel_text_on_the_cpu_equals_the_restatement(emu, n, world, weights):
    d, exe = emu
    x, y, t, w = E.cloud(n, weights)
    stride = (n + world - 1) // world
    gw = np.zeros(world * stride, np.float32)
    gw[:n] = w
    gpose = np.zeros((world, 3, stride), np.float32)          # buffer 17: rank-major blocks [x | y | theta], the last one padded
    for r in range(world):
        lo, hi = r * stride, min((r + 1) * stride, n)
        gpose[r, 0, :hi - lo], gpose[r, 1, :hi - lo], gpose[r, 2, :hi - lo] = x[lo:hi], y[lo:hi], t[lo:hi]
    fin, fout = str(d / ("in_%d_%d.bin" % (n, world))), str(d / ("out_%d_%d.bin" % (n, world)))
    with open(fin, "wb") as f:
        f.write(gw.tobytes())
        f.write(gpose.tobytes())
    r = subprocess.run([exe, str(n), str(world), fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    got, want = np.fromfile(fout, np.float32), E.estimate16(x, y, t, w)
    assert (got.view(np.int32) == want.view(np.int32)).all(), (got.tolist(), want.tolist())
