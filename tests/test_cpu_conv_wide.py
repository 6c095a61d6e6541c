"""The staggered-start planner of csrc/xai_conv_walk.h and libxai_convw.so without a GPU.  The planner is built alone by the host
compiler (tests/conv_stagger_main.cpp: it needs nothing of HIP), once plainly and once with -fsanitize=address,undefined -- that
stand-alone program is the sanitizer run of the planner -- and both are asked the same cases; the expected plans and chains are
tests/conv_stagger_restated.py's.  Then the header of the library at 1.0 with the literal argument types of its two entries and every
refusal K80 and K81 make before any HIP call.  What holds for every library alike (the record, the exports, the loader, build()'s
version check) is tests/test_cpu_abi_libs.py's, for the key convw."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import conv_stagger_restated as S

from abi_libs import built, declared, exported_elsewhere
from conftest import PKG, ROOT

HEADER = os.path.join(ROOT, "include", "xai_convw.h")
ENTRIES = ["xai_convw_bwd_data_f32", "xai_convw_bwd_data_simple_f32"]
_p, _i = C.c_void_p, C.c_int

# (K, depth, tile, axis, n, stride): the GEMM kernels of the probe (MT32x32x64 at K = 512 and 1024, MT64x64x32 at K = 128 and 64, both
# SU32_SUS256), no stagger, a stride of one iteration, of four, one below an iteration, fewer iterations than n at every halving,
# one iteration, and the other axis
CASES = [(512, 64, 32, 0, 32, 256), (1024, 64, 32, 0, 32, 256), (128, 32, 64, 0, 32, 256), (64, 32, 64, 0, 32, 256), (512, 64, 64, 0, 0, 0),
         (80, 16, 32, 0, 32, 64), (256, 16, 32, 0, 8, 256), (256, 64, 16, 0, 32, 128), (96, 32, 48, 0, 4, 256), (48, 16, 16, 1, 2, 0),
         (16, 16, 16, 0, 32, 256), (2048, 16, 128, 1, 32, 64), (192, 64, 32, 0, 1, 256)]
REFUSED = [(0, 16, 16, 0, 0, 0), (8, 16, 16, 0, 0, 0), (24, 16, 16, 0, 0, 0), (64, 0, 16, 0, 0, 0), (64, 24, 16, 0, 0, 0), (64, 48, 16, 0, 0, 0),
           (64, 128, 16, 0, 0, 0), (64, 16, 0, 0, 0, 0), (64, 16, 8, 0, 0, 0), (64, 16, 24, 0, 0, 0), (64, 16, 16, 2, 0, 0), (64, 16, 16, -1, 0, 0),
           (64, 16, 16, 0, 3, 0), (64, 16, 16, 0, -2, 0), (64, 16, 16, 0, 12, 64), (64, 16, 16, 0, 4, -64)]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    path = tmp_path_factory.mktemp("conv_stagger_" + request.param) / "conv_stagger"
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + extra + ["-I" + os.path.join(PKG, "csrc"),
                                                                                os.path.join(ROOT, "tests", "conv_stagger_main.cpp"), "-o", str(path)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(path)


def _run(exe, mode, args=()):
    r = subprocess.run([exe, mode] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr              # a sanitizer report ends the program with a non-zero status
    return r.stdout.splitlines()


def test_the_restatement_starts_every_tile_inside_the_loop_and_takes_every_block_once():
    assert S.plan(512, 64, 32, 0, 32, 256) == (32, 4, 32, 0, 7, 0) and S.plan(1024, 64, 32, 0, 32, 256) == (64, 4, 32, 0, 15, 0)
    assert S.plan(128, 32, 64, 0, 32, 256) == (8, 2, 64, 0, 1, 1) and S.plan(64, 32, 64, 0, 32, 256) == (4, 2, 64, 0, 0, 0)
    assert S.plan(192, 64, 32, 0, 1, 256)[4:] == (0, 0) and S.plan(512, 64, 64, 0, 0, 0)[4:] == (0, 0)
    for case in CASES:
        p = S.plan(*case)
        blocks, per_iter, tile, _, mask, shift = p
        assert (mask + 1) & mask == 0 and ((mask << shift) + 1) * per_iter <= blocks          # the last start is an iteration of the loop
        starts = set()
        for at in range(0, 40 * tile, 16):
            chain = S.chain(p, at)
            assert sorted(chain) == list(range(blocks)) and chain[0] % per_iter == 0          # every K-block once, from an iteration's first
            assert all((b - a) % blocks == 1 for a, b in zip(chain, chain[1:]))               # ascending, one wrap
            assert chain == S.chain(p, at - at % tile)                                        # one start per tile
            starts.add(chain[0])
        assert len(starts) == mask + 1
    assert S.chain(S.plan(512, 64, 32, 0, 32, 256), 100)[:2] == [12, 13] and S.chain(S.plan(128, 32, 64, 0, 32, 256), 64)[0] == 4


def test_the_planner_is_the_restatement(exe):
    lines = _run(exe, "plan", [v for c in CASES for v in c])
    assert lines == ["ok " + " ".join(str(v) for v in S.plan(*c)) for c in CASES]
    for case in CASES:
        p = S.plan(*case)
        for at in (0, 16, p[2] - 16, p[2], 3 * p[2] + 16, 33 * p[2]):
            assert _run(exe, "chain", list(case) + [at]) == [" ".join(str(b) for b in S.chain(p, at)) + " "], (case, at)


def test_the_planner_refuses_what_it_cannot_plan_and_leaves_the_plan_untouched(exe):
    assert all(S.plan(*c) is None for c in REFUSED)
    assert _run(exe, "plan", [v for c in REFUSED for v in c]) == ["refused"] * len(REFUSED)       # (exit status 3: *st was written)


def test_the_emulation_and_the_bound_on_a_small_sum():
    rng = np.random.default_rng(0)
    gy, w = rng.standard_normal((80, 40)).astype(np.float32), rng.standard_normal((80, 35)).astype(np.float32)
    exact = w.astype(np.float64).T @ gy.astype(np.float64)
    abs_sum = np.abs(w.astype(np.float64)).T @ np.abs(gy.astype(np.float64))
    seen = set()
    for g, z, axis, su in itertools.product((0, 1), (0, 1), (0, 1), (0, 4)):
        got = S.emulate(gy, w, g, z, S.plan(80, 16, 16, axis, su, 64))
        assert got.dtype == np.float32 and (np.abs(got - exact) <= S.bound(80, abs_sum)).all()
        seen.add(got.tobytes())
    assert len(seen) >= 6                                                                     # the starts and groupings are different sums


def test_the_header_parses_at_1_0_with_these_argument_types():
    from xai_engine import _lib
    rec = _lib.LIBRARIES["convw"]
    text = open(HEADER).read()
    args, ret, version = _lib.parse_header(text, rec.defines)
    assert version == (rec.version, rec.minor) == (1, 0)
    assert sorted(args) == declared(HEADER) == sorted(ENTRIES + ["xai_convw_version", "xai_convw_version_minor"])
    assert args == rec.signatures and all(t is _i for t in ret.values())
    for name in ENTRIES:
        assert args[name] == [_p, _p] + [_i] * 11 + [_p, _p]
    make = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert "conv/conv1x1_bwd_wide_kernels.hip" in make and os.path.exists(os.path.join(PKG, "csrc", "conv", "conv1x1_bwd_wide_kernels.hip"))
    db = subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-pnq"], capture_output=True, text=True).stdout
    rule = next(line for line in db.splitlines() if line.startswith("build/conv/conv1x1_bwd_wide_kernels.o:"))
    assert "../../include/xai_convw.h" in rule and "xai_conv_walk.h" in rule


def test_k80_and_k81_check_their_arguments_without_a_gpu():
    from xai_engine import _lib
    built("convw")
    lib = _lib.load("convw")
    p = 4096                                              # non-null, aligned, never dereferenced: every call below is refused
    NULL, SHAPE, UNSUPPORTED = -1, -2, -3

    def call(entry, gy=p, w=p, N=2, K=64, C=8, HW=100, g=0, z=0, depth=16, tile=32, axis=0, su=0, stride=0, gx=p):
        return getattr(lib, entry)(gy, w, N, K, C, HW, g, z, depth, tile, axis, su, stride, gx, None)
    for entry in ENTRIES:
        def f(**kw):
            return call(entry, **kw)
        assert f(gy=None) == NULL and f(w=None) == NULL and f(gx=None) == NULL
        assert f(gy=p + 2) == SHAPE and f(w=p + 1) == SHAPE and f(gx=p + 3) == SHAPE
        assert f(N=0) == SHAPE and f(C=0) == SHAPE and f(HW=0) == SHAPE and f(K=0) == SHAPE
        assert f(K=24) == SHAPE and f(K=8) == SHAPE and f(K=40) == SHAPE                      # K % 16 != 0
        assert f(g=2) == SHAPE and f(g=-1) == SHAPE and f(axis=2) == SHAPE
        assert f(depth=0) == SHAPE and f(depth=24) == SHAPE and f(depth=48) == SHAPE and f(depth=128) == SHAPE
        assert f(tile=0) == SHAPE and f(tile=8) == SHAPE and f(tile=40) == SHAPE
        assert f(su=3) == SHAPE and f(su=-4) == SHAPE and f(su=4, stride=-1) == SHAPE
        assert f(N=65536) == UNSUPPORTED and f(K=1 << 20, HW=4096) == UNSUPPORTED and f(C=1 << 20, HW=4096) == UNSUPPORTED
    fast = ENTRIES[0]
    assert call(fast, su=4, stride=64, axis=1) == UNSUPPORTED and call(fast, su=4, stride=64, tile=16) == UNSUPPORTED
    assert call(fast, su=4, stride=64, tile=48) == UNSUPPORTED
    assert call(ENTRIES[1], C=16 * 65535 + 1, HW=16) == UNSUPPORTED


def test_no_other_library_exports_a_convw_name():
    assert not [(o, n) for o, n in exported_elsewhere("convw") if n.startswith("xai_convw")]
