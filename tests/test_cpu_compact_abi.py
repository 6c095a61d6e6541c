"""libxai_compact.so and include/xai_hip_compact.h without a GPU: the header read at 1.0 with the literal argument types of its four
entries, the build rule, and every refusal K62-K64 make before any HIP call.  What holds for every library alike (the record, the
exports, the loader) is in tests/test_cpu_abi_libs.py."""
import ctypes as C
import os
import re
import subprocess

from abi_libs import built, declared
from conftest import PKG, ROOT

HEADER = os.path.join(ROOT, "include", "xai_hip_compact.h")
ENTRIES = ["xai_bn_relu_bwd_bcast_f32", "xai_bn_relu_bwd_compact_f32", "xai_bn_relu_fwd_cnhw_f32", "xai_stride_gather_cnhw_f32"]
_p, _i, _f = C.c_void_p, C.c_int, C.c_float


def test_the_header_parses_at_1_0_with_these_argument_types():
    from xai_engine import _lib
    rec = _lib.LIBRARIES["compact"]
    text = open(HEADER).read()
    args, ret, version = _lib.parse_header(text, rec.defines)
    assert version == (rec.version, rec.minor) == (1, 0)
    assert sorted(args) == declared(HEADER) == sorted(ENTRIES + ["xai_compact_version", "xai_compact_version_minor"])
    assert args == rec.signatures and all(t is _i for t in ret.values())
    assert args["xai_stride_gather_cnhw_f32"] == [_p, _i, _i, _i, _i, _i, _p, _p]
    assert args["xai_bn_relu_fwd_cnhw_f32"] == [_p] * 6 + [_f] + [_p] * 4 + [_f, _i, _i, _i, _i, _p, _p, _p]
    assert args["xai_bn_relu_bwd_compact_f32"] == [_p, _p, _p, _i, _i, _p, _p, _p, _f, _p, _p, _f, _i, _i, _i, _i, _i, _p, _p, _i, _p]
    assert args["xai_bn_relu_bwd_bcast_f32"] == [_p, _p, _p, _i, _f, _f, _p, _p, _p, _p, _f, _p, _p, _f, _i, _i, _i, _i, _i, _p, _p, _p]
    listed = text[text.index(" *   0 = "):text.index("#define XAI_COMPACT_VERSION")]
    assert sorted(re.findall(r"xai_[a-z0-9_]+", listed)) == ENTRIES
    for name in ENTRIES:                                  # every entry names what it replaces and the reference lines behind it
        at = text.index("int " + name + "(")
        comment = text[text.rfind("/*", 0, at):at]
        assert re.search(r"replaces\s", comment) and re.search(r"(saliencyMethods|evaluatePerturbation)\.py:\d+", comment), name


def test_the_makefile_builds_it_and_rebuilds_it_when_its_header_or_the_shared_device_header_changes():
    make = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert "SRCS_compact := bnrelu_compact_kernels.hip" in make and "xai_bn_device.h" in make
    db = subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-pnq"], capture_output=True, text=True).stdout
    rule = next(line for line in db.splitlines() if line.startswith("build/bnrelu_compact_kernels.o:"))
    assert "../../include/xai_hip_compact.h" in rule and "xai_bn_device.h" in rule and "xai_bn_index.h" in rule


def test_k62_to_k64_check_their_arguments_without_a_gpu():
    from xai_engine import _lib
    built("compact")
    lib = _lib.load("compact")
    p = 4096                                              # non-null, 16-byte aligned, never dereferenced: every call below is refused
    NULL, SHAPE, UNSUPPORTED = -1, -2, -3
    gather = lib.xai_stride_gather_cnhw_f32
    assert gather(None, 1, 1, 4, 4, 2, p, None) == NULL and gather(p, 1, 1, 4, 4, 2, None, None) == NULL
    assert gather(p, 0, 1, 4, 4, 2, p, None) == SHAPE and gather(p, 1, 1, 4, 4, 0, p, None) == SHAPE
    assert gather(p, 65536, 65536, 4, 4, 2, p, None) == UNSUPPORTED

    def fwd(x=p, idt=p, w=p, y=p, mask=p, w2=None, b2=None, N=1, C=2, HW=4, variant=9):
        return lib.xai_bn_relu_fwd_cnhw_f32(x, idt, w, p, p, p, 1e-5, w2, b2, p, p, 1e-5, variant, N, C, HW, y, mask, None)
    assert fwd(x=None) == NULL and fwd(idt=None) == NULL and fwd(w=None) == NULL and fwd(y=None) == NULL and fwd(w2=p) == NULL
    assert fwd(N=0) == SHAPE and fwd(variant=16) == SHAPE and fwd(mask=12) == SHAPE and fwd(N=65536, C=65536) == UNSUPPORTED

    def bwd(gy=p, gy2=None, gc=None, W=2, s=2, mask=p, w=p, gx=p, w2=None, v2=None, gid=None, cnhw=0, N=1, C=2, HW=4):
        return lib.xai_bn_relu_bwd_compact_f32(gy, gy2, gc, W, s, mask, w, p, 1e-5, w2, v2, 1e-5, 9, 0, N, C, HW, gx, gid, cnhw, None)
    assert bwd(gy=None) == NULL and bwd(mask=None) == NULL and bwd(w=None) == NULL and bwd(gx=None) == NULL
    assert bwd(w2=p) == NULL and bwd(w2=p, gid=p) == NULL and bwd(cnhw=1) == NULL
    assert bwd(gy2=p, gc=p) == SHAPE and bwd(gc=p, W=3) == SHAPE and bwd(gc=p, s=0) == SHAPE and bwd(gc=p, W=0) == SHAPE
    assert bwd(C=0) == SHAPE and bwd(mask=12) == SHAPE

    def bcast(go=p, fc=p, t=p, classes=3, mask=p, gx=p, N=1):
        return lib.xai_bn_relu_bwd_bcast_f32(go, fc, t, classes, 0.25, 0.0, None, mask, p, p, 1e-5, None, None, 0.0, 9, 0, N, 2, 4, gx, None, None)
    assert bcast(go=None) == NULL and bcast(fc=None) == NULL and bcast(t=None) == NULL and bcast(mask=None) == NULL and bcast(gx=None) == NULL
    assert bcast(classes=0) == SHAPE and bcast(N=0) == SHAPE
