"""csrc/xai_conv_walk.h and libxai_conv.so without a GPU.  The planner header is built alone by the host compiler
(tests/conv_walk_main.cpp: it needs nothing of HIP), once plainly and once with -fsanitize=address,undefined -- that stand-alone
program is the sanitizer run of the planner -- and both are asked the same cases; the expected plans are tests/conv_walk_restated.py's.
Then the header of the library at 1.0 with the literal argument types of its two entries, and every refusal K78 and K79 make before
any HIP call.  What holds for every library alike (the record, the exports, the loader, build()'s version check) is
tests/test_cpu_abi_libs.py's, for the key conv."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import conv_walk_restated as R

from abi_libs import built, declared, exported_elsewhere
from conftest import PKG, ROOT

HEADER = os.path.join(ROOT, "include", "xai_conv.h")
ENTRIES = ["xai_conv1x1_bwd_data_f32", "xai_conv1x1_bwd_data_simple_f32"]
_p, _i = C.c_void_p, C.c_int

# (K, S): layer4's own (128 blocks over 19 and over 3, remainders 14 and 2), one partial sum, five blocks over three, fewer blocks
# than partial sums (1 and 2 over 3), blocks = partial sums, the most partial sums there can be, and no remainder
SHAPES = ((2048, 19), (2048, 3), (2048, 1), (80, 3), (16, 3), (32, 3), (48, 3), (16, 1), (2048, 32), (512, 4))
CASES = [(K, S, m, g, o, z) for (K, S) in SHAPES for m, g, o, z in itertools.product((0, 1), (0, 1), (0, 1), (0, 1))]
REFUSED = [(0, 1, 0, 0, 0, 0), (8, 1, 0, 0, 0, 0), (24, 1, 0, 0, 0, 0), (-16, 1, 0, 0, 0, 0), (2048, 0, 0, 0, 0, 0), (2048, 33, 0, 0, 0, 0),
           (2048, -1, 0, 0, 0, 0), (2048, 3, 2, 0, 0, 0), (2048, 3, -1, 0, 0, 0), (2048, 3, 0, 2, 0, 0), (2048, 3, 0, 0, 2, 0)]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    path = tmp_path_factory.mktemp("conv_walk_" + request.param) / "conv_walk"
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + extra + ["-I" + os.path.join(PKG, "csrc"),
                                                                                os.path.join(ROOT, "tests", "conv_walk_main.cpp"), "-o", str(path)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(path)


def _run(exe, mode, args=()):
    r = subprocess.run([exe, mode] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr              # a sanitizer report ends the program with a non-zero status
    return r.stdout.splitlines()


def test_the_restatement_lists_every_block_once_and_sizes_the_partial_sums_by_both_rules():
    for K, S in SHAPES:
        nb = K // 16
        q, r = divmod(nb, S)
        for m in (0, 1):
            asc = R.parts(K, S, m, R.ASCENDING)
            assert sorted(b for p in asc for b in p) == list(range(nb))                      # every K-block exactly once
            assert [len(p) for p in asc] == [q + (s < r) for s in range(S)]                  # the remainder in front
            assert all(p == sorted(p) for p in asc)                                          # ascending inside a partial sum
            assert R.parts(K, S, m, R.DESCENDING) == asc[::-1]
        assert [b for p in R.parts(K, S, R.CONTIGUOUS, 0) for b in p] == list(range(nb))     # contiguous: one run after the other
        assert all(b % S == s for s, p in enumerate(R.parts(K, S, R.ROUND_ROBIN, 0)) for b in p)
    assert [len(p) for p in R.parts(2048, 3, 0, 0)] == [43, 43, 42] and R.parts(2048, 3, 0, 0)[1][0] == 43
    assert R.parts(2048, 3, 1, 0)[2][:3] == [2, 5, 8] and [len(p) for p in R.parts(2048, 19, 1, 0)] == [7] * 14 + [6] * 5
    assert R.parts(80, 3, 0, 0) == [[0, 1], [2, 3], [4]] and R.parts(80, 3, 1, 0) == [[0, 3], [1, 4], [2]]
    assert R.parts(16, 3, 0, 0) == [[0], [], []] and R.parts(32, 3, 1, 1) == [[], [1], [0]]


def test_the_planner_is_the_restatement(exe):
    lines = iter(_run(exe, "plan", [v for c in CASES for v in c]))
    for K, S, m, g, o, z in CASES:
        assert next(lines).split() == ["ok", str(S), str(g), str(z)], (K, S, m, g, o, z)
        want = R.parts(K, S, m, o)
        for blocks in want:
            head, _, listed = next(lines).partition(":")
            first, step, count = (int(v) for v in head.split())
            assert [int(v) for v in listed.split()] == blocks and count == len(blocks), (K, S, m, o, blocks)
            assert not blocks or (first == blocks[0] and step == (S if m == R.ROUND_ROBIN else 1))
    assert next(lines, None) is None


def test_the_planner_refuses_what_it_cannot_walk_and_leaves_the_plan_untouched(exe):
    assert _run(exe, "plan", [v for c in REFUSED for v in c]) == ["refused"] * len(REFUSED)       # (exit status 3: *w was written)


def test_the_two_k_groupings_and_their_slab_rows(exe):
    lines = [[int(v) for v in l.split()] for l in _run(exe, "group")]
    assert lines[0] == list(range(16)) == lines[1]                                            # consecutive fours: k = 4m + q, in place
    assert lines[2] == [0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15]                 # stride 4: k = m + 4q
    for g, (ks, rows) in enumerate((lines[0:2], lines[2:4])):
        assert ks == [R.k_of(g, m, q) for m in range(4) for q in range(4)]
        assert [rows[k] for k in ks] == list(range(16))                                       # row(k(m, q)) = 4m + q


def test_the_emulation_and_the_bound_on_a_small_sum():
    rng = np.random.default_rng(0)
    gy, w = rng.standard_normal((80, 5)).astype(np.float32), rng.standard_normal((80, 3)).astype(np.float32)
    exact = w.astype(np.float64).T @ gy.astype(np.float64)
    abs_sum = np.abs(w.astype(np.float64)).T @ np.abs(gy.astype(np.float64))
    seen = set()
    for walk in [(S, m, g, o, z) for S in (1, 3) for m, g, o, z in itertools.product((0, 1), (0, 1), (0, 1), (0, 1))]:
        got = R.emulate(gy, w, walk)
        assert got.dtype == np.float32 and (np.abs(got - exact) <= R.bound(80, walk[0], walk[1], walk[3], abs_sum)).all()
        seen.add(got.tobytes())
    assert len(seen) > 4                                                                      # the walks are different sums


def test_the_header_parses_at_1_0_with_these_argument_types():
    from xai_engine import _lib
    rec = _lib.LIBRARIES["conv"]
    text = open(HEADER).read()
    args, ret, version = _lib.parse_header(text, rec.defines)
    assert version == (rec.version, rec.minor) == (1, 0)
    assert sorted(args) == declared(HEADER) == sorted(ENTRIES + ["xai_conv_version", "xai_conv_version_minor"])
    assert args == rec.signatures and all(t is _i for t in ret.values())
    assert args["xai_conv1x1_bwd_data_f32"] == [_p, _p] + [_i] * 10 + [_p, _p]
    assert args["xai_conv1x1_bwd_data_simple_f32"] == [_p, _p] + [_i] * 9 + [_p, _p]
    make = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert "conv/conv1x1_bwd_kernels.hip" in make and os.path.exists(os.path.join(PKG, "csrc", "conv", "conv1x1_bwd_kernels.hip"))
    db = subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-pnq"], capture_output=True, text=True).stdout
    rule = next(line for line in db.splitlines() if line.startswith("build/conv/conv1x1_bwd_kernels.o:"))
    assert "../../include/xai_conv.h" in rule and "xai_conv_walk.h" in rule


def test_k78_and_k79_check_their_arguments_without_a_gpu():
    from xai_engine import _lib
    built("conv")
    lib = _lib.load("conv")
    p = 4096                                              # non-null, aligned, never dereferenced: every call below is refused
    NULL, SHAPE, UNSUPPORTED = -1, -2, -3

    def fast(gy=p, w=p, N=2, K=32, C=8, HW=49, S=3, m=0, g=0, o=0, z=0, tile=0, gx=p):
        return lib.xai_conv1x1_bwd_data_f32(gy, w, N, K, C, HW, S, m, g, o, z, tile, gx, None)

    def simple(gy=p, w=p, N=2, K=32, C=8, HW=49, S=3, m=0, g=0, o=0, z=0, gx=p):
        return lib.xai_conv1x1_bwd_data_simple_f32(gy, w, N, K, C, HW, S, m, g, o, z, gx, None)
    for f in (fast, simple):
        assert f(gy=None) == NULL and f(w=None) == NULL and f(gx=None) == NULL
        assert f(gy=p + 2) == SHAPE and f(w=p + 1) == SHAPE and f(gx=p + 3) == SHAPE
        assert f(N=0) == SHAPE and f(C=0) == SHAPE and f(HW=0) == SHAPE and f(K=0) == SHAPE
        assert f(K=24) == SHAPE and f(K=8) == SHAPE and f(K=40) == SHAPE                      # K % 16 != 0
        assert f(S=0) == SHAPE and f(S=33) == SHAPE and f(m=2) == SHAPE and f(g=2) == SHAPE and f(o=2) == SHAPE
        assert f(N=50000, HW=50000) == UNSUPPORTED and f(N=1 << 20, K=2048, HW=49) == UNSUPPORTED
        assert f(N=1 << 20, K=16, C=4096, HW=49) == UNSUPPORTED
    assert fast(tile=16) == SHAPE and fast(tile=48) == SHAPE and fast(tile=-1) == SHAPE


def test_no_other_library_exports_a_conv_name():
    """the prefixes of this library's own names; xai_convw_ is the sibling's (tests/test_cpu_conv_wide.py)"""
    assert not [(o, n) for o, n in exported_elsewhere("conv") if n.startswith(("xai_conv_", "xai_conv1x1_"))]
