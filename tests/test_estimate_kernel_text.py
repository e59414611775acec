"""The pfslam_estimate kernels' own text, run on the CPU (no GPU needed): tests/estimate_emu.cpp compiles the kernels cut out of
csrc/pfslam_stages.hip.inc behind a small SIMT shim (a thread per GPU thread, barriers for __syncthreads and the wave shuffles) with
-ffp-contract=off like the library, under AddressSanitizer and UBSan with every buffer at its exact size.  Unsharded and rank-major sharded
layouts must give the restatement's 16 floats bit for bit (tests/estimate_ref.py), which also shows that no index leaves a buffer and that
every thread reaches every barrier.  What it cannot show is the GPU's arithmetic and memory model: tests/test_gpu_estimate.py does."""

import numpy as np
import pytest

import kernel_text as KT
import estimate_ref as E

CASES = [(1, 1, "zeros"), (64, 1, "zeros"), (65, 2, "zeros"), (4096, 3, "zeros"), (4097, 2, "one"), (4097, 1, "zeros"), (5000, 3, "zeros"),
         (8193, 3, "zeros")]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return KT.build(tmp_path_factory, "estimate", ("k_estimate_small", "k_estimate_centred"), ("PF_SUM_TILE",))


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
    KT.run(exe, n, world, fin, fout)
    got, want = np.fromfile(fout, np.float32), E.estimate16(x, y, t, w)
    assert (got.view(np.int32) == want.view(np.int32)).all(), (got.tolist(), want.tolist())
