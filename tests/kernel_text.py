"""What the tests/test_*_kernel_text.py share (TEST INFRASTRUCTURE, a plain module): the table of the sections of kernel text that are cut
out of csrc/ between comment marks, what each needs in front of it, and the one recipe that compiles a tests/*_emu.cpp over such text
behind tests/simt_shim.h as a stand-alone program under AddressSanitizer and UBSan, with -ffp-contract=off like the library."""
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpu-icp-slam_amd", "csrc")
# section: (file under csrc/, STEM of its marks "// STEM-KERNEL-TEXT-BEGIN" and "-END", the sections its text needs in front of it).
# The table is in the one order in which the text compiles: text() emits what a feature needs in this order.
SECTIONS = {
    "wave_sum": ("pfslam_stages.hip.inc", "WAVE-SUM", ()),
    "svd3": ("pfslam_stages.hip.inc", "SVD3", ()),
    "estimate_device": ("pfslam_stages.hip.inc", "ESTIMATE-DEVICE", ("wave_sum",)),
    "estimate": ("pfslam_stages.hip.inc", "ESTIMATE", ("estimate_device",)),
    "register": ("pfslam_register.hip.inc", "REGISTER", ("wave_sum", "svd3")),
    "register_batch": ("pfslam_register_batch.hip.inc", "REGISTER-BATCH", ("register",)),
    "search": ("pfslam_search.hip.inc", "SEARCH", ("register",)),
    "search_scan": ("pfslam_search_scan.hip.inc", "SEARCH-SCAN", ("search",)),
    "search_cov": ("pfslam_search_cov.hip.inc", "SEARCH-COV", ("estimate_device", "search_scan")),
    "search_wide": ("pfslam_search_wide.hip.inc", "SEARCH-WIDE", ("search",)),
    "search_best": ("pfslam_search_best.hip.inc", "SEARCH-BEST", ("search_wide",)),
    "cast": ("pfslam_cast.hip.inc", "CAST", ()),
    "cast_score": ("pfslam_cast_score.hip.inc", "CAST-SCORE", ("cast",)),
}


def clangxx():
    """clang++ (kd_device.h uses ext_vector_type): the one hipcc drives, or any on the path."""
    cands = [shutil.which("clang++")]
    try:
        hipcc = importlib.import_module("gpu-icp-slam_amd.build").hipcc()
        rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
        cands = [os.path.join(rocm, "lib", "llvm", "bin", "clang++"), os.path.join(rocm, "llvm", "bin", "clang++")] + cands
    except Exception:
        pass
    for c in cands:
        if c and os.path.exists(c):
            return c
    return None


def section(name):
    """The text of one section: from its begin mark up to its end mark, each of which must occur exactly once."""
    fname, stem, _ = SECTIONS[name]
    src = open(os.path.join(CSRC, fname)).read()
    first, last = "// %s-KERNEL-TEXT-BEGIN" % stem, "// %s-KERNEL-TEXT-END" % stem
    assert src.count(first) == 1 and src.count(last) == 1, "the kernel text has moved: %r in %s" % (first, fname)
    assert src.index(first) < src.index(last)
    return src[src.index(first):src.index(last)]


def text(feature):
    """The section `feature` behind everything it needs, directly or not."""
    need, todo = set(), [feature]
    while todo:
        name = todo.pop()
        if name not in need:
            need.add(name)
            todo += SECTIONS[name][2]
    return "".join(section(name) for name in SECTIONS if name in need)


def defines(names):
    """The #define lines of csrc/pfslam_hip.hip for these names."""
    main = open(os.path.join(CSRC, "pfslam_hip.hip")).read()
    return "".join(re.search(r"^#define %s .*$" % name, main, re.M).group(0) + "\n" for name in names)


def build(tmp_path_factory, feature, names, define=()):
    """Compile tests/<feature>_emu.cpp over the kernel text of `feature`, in which every one of `names` must occur, and the #define lines
    `define`.  Returns (directory, executable)."""
    cxx = clangxx()
    if cxx is None:
        pytest.fail("clang++ is needed to compile the kernel text for the CPU")
    d = tmp_path_factory.mktemp(feature + "_emu")
    cut = text(feature)
    for name in names:
        assert name in cut, "%s is not in the kernel text of %s" % (name, feature)
    (d / "kernel_text.inc").write_text(cut)
    (d / "kernel_defines.inc").write_text(defines(define))
    os.makedirs(str(d / "hip"))
    (d / "hip" / "hip_runtime.h").write_text("// (tests/simt_shim.h stands in for the HIP runtime's declarations)\n")
    emu = feature + "_emu.cpp"
    for src in (os.path.join(CSRC, "pf_math.h"), os.path.join(CSRC, "kd_device.h"), os.path.join(ROOT, "tests", "simt_shim.h"),
                os.path.join(ROOT, "tests", emu)):
        shutil.copy(src, str(d))
    exe = str(d / (feature + "_emu"))
    subprocess.check_call([cxx, "-std=c++20", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wno-unknown-attributes", "-pthread", "-I", str(d), str(d / emu), "-o", exe])
    return d, exe


def run(exe, *args):
    """Run an emulator to the end: exit status 0, or the tail of what it (or a sanitizer) wrote to stderr."""
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def device_arrays(tree):
    """The four device arrays of a map as pfslam_set_map lays them out (csrc/kd_device.h): hot records, z (a planar z level's true left
    child as int bits), parents, weights; and the planar flag."""
    n = len(tree)
    planar = int(not (tree["z"] != 0).any())
    left = tree["left"].copy()
    z = tree["z"].astype(np.float32).copy()
    if planar:
        zl = tree["axis"] == 2
        z.view(np.int32)[zl] = tree["left"][zl]
        left[zl] = tree["right"][zl]
    hot = np.zeros((n, 4), np.uint32)
    hot[:, 0] = tree["x"].astype(np.float32).view(np.uint32)
    hot[:, 1] = tree["y"].astype(np.float32).view(np.uint32)
    hot[:, 2] = (left.astype(np.int64) & 0x3fffffff).astype(np.uint32) | (tree["axis"].astype(np.uint32) << 30)
    hot[:, 3] = tree["right"].astype(np.int32).view(np.uint32)
    return hot, z, tree["parent"].astype(np.int32), tree["w"].astype(np.float32), planar


def poses_of(m, seed=3):
    """m poses inside the 40 m map, the first the one the cast tests cast from."""
    rng = np.random.RandomState(seed)
    p = np.concatenate([rng.uniform(-15, 15, (m, 2)), rng.uniform(-3.2, 3.2, (m, 1))], axis=1).astype(np.float32)
    p[0] = (0.5, 0.3, 0.1)
    return p
