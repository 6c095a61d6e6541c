"""xai_engine/_lib.py binds the C ABI from include/xai_hip.h itself (parse_header): the ctypes lists it derives from a synthetic
header that uses every type the binding knows, what it refuses, and literal pins of mixed-type entries of the real header."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from test_cpu_host import _lib_path

_p, _i, _l, _f, _d, _z = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double, C.c_size_t

SYNTHETIC = """
/* a comment with a ; and a prototype in it: int xai_not_declared(unsigned n); */
#ifndef XAI_HIP_H
#define XAI_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef void* xai_stream_t; /* hipStream_t */
#define XAI_ABI_VERSION 7
#define XAI_ABI_MINOR 42
#define XAI_E_NULL (-1)   /* not a version */
int xai_version(void);
const char* xai_strerror(int code);
size_t xai_some_bytes(int n, int64_t m);
/* every scalar type */
int xai_scalars_f32(int a, int64_t b, float c, double d,
                    size_t e,   xai_stream_t stream);
/* every pointer spelling */
int xai_pointers_f64(const float* a, float* b, double* c, const float* const* d, const void* e, void* f, const int32_t* g, int32_t* h,
                     const int64_t* i, int64_t* j, const uint64_t* k, uint64_t* l, const uint8_t* m, uint8_t* n, xai_stream_t s);
int xai_ranks_i32(const int32_t* rank, xai_stream_t stream);
int xai_packs_u64(uint64_t* bits, xai_stream_t stream);
int xai_max_features(void);
#ifdef __cplusplus
}
#endif
#endif
"""


@pytest.fixture(scope="module")
def L():
    from xai_engine import _lib
    return _lib


def test_synthetic_header_gives_these_ctypes_lists(L):
    args, ret, version = L.parse_header(SYNTHETIC)
    assert version == (7, 42)
    assert args == {"xai_version": [], "xai_strerror": [_i], "xai_some_bytes": [_i, _l], "xai_scalars_f32": [_i, _l, _f, _d, _z, _p],
                    "xai_pointers_f64": [_p] * 15, "xai_ranks_i32": [_p, _p], "xai_packs_u64": [_p, _p], "xai_max_features": []}
    assert ret == {"xai_version": _i, "xai_strerror": C.c_char_p, "xai_some_bytes": _z, "xai_scalars_f32": _i, "xai_pointers_f64": _i,
                   "xai_ranks_i32": _i, "xai_packs_u64": _i, "xai_max_features": _i}


def _with(extra, drop=None):
    text = SYNTHETIC if drop is None else SYNTHETIC.replace(drop, "")
    assert text != SYNTHETIC or drop is None
    return text.replace("int xai_max_features(void);", "int xai_max_features(void);\n" + extra)


@pytest.mark.parametrize("text, quoted", [
    (_with("int xai_count(unsigned n);"), "int xai_count(unsigned n)"),
    (_with("int xai_walk_f32(int (*visit)(int), xai_stream_t stream);"), "int xai_walk_f32(int (*visit)(int), xai_stream_t stream)"),
    (_with("struct xai_pair { int a; int b; };"), "struct xai_pair { int a"),
    (_with("int xai_version(void);"), "int xai_version(void)"),
    (_with("#define XAI_TWO_LINES(a) \\\n  ((a) + 1)"), "#define XAI_TWO_LINES(a) \\"),
    (_with("int xai_no_stream_f32(const float* x, int n);"), "int xai_no_stream_f32(const float* x, int n)"),
    # the rest of "nothing falls through to a default type"
    (_with("int xai_late_f32(xai_stream_t stream, int n);"), "int xai_late_f32(xai_stream_t stream, int n)"),
    (_with("int xai_twice_f32(xai_stream_t a, xai_stream_t b);"), "int xai_twice_f32(xai_stream_t a, xai_stream_t b)"),
    (_with("int xai_stream_bytes(xai_stream_t stream);"), "int xai_stream_bytes(xai_stream_t stream)"),
    (_with("size_t xai_sized_f32(xai_stream_t stream);"), "size_t xai_sized_f32(xai_stream_t stream)"),
    (_with("size_t xai_sized_f64(int n);"), "size_t xai_sized_f64(int n)"),
    (_with("int xai_unnamed(int);"), "int xai_unnamed(int)"),
    (_with("int xai_chars(const char* s);"), "int xai_chars(const char* s)"),
    (_with("float xai_ratio(int n);"), "float xai_ratio(int n)"),
    (_with("int other_name(int n);"), "int other_name(int n)"),
    (_with("int xai_left_over(int n)"), "int xai_left_over(int n)"),
    # and a header without its frame
    (_with("", drop="#define XAI_ABI_MINOR 42\n"), "XAI_ABI_MINOR"),
    (_with("#define XAI_ABI_MINOR 43"), "#define XAI_ABI_MINOR 43"),
    (_with("", drop="typedef void* xai_stream_t; /* hipStream_t */\n"), "typedef void* xai_stream_t"),
    (_with("", drop='extern "C" {\n'), 'extern "C"'),
])
def test_parser_refuses_and_quotes_the_statement(L, text, quoted):
    with pytest.raises(L.XaiHipError) as e:
        L.parse_header(text)
    assert quoted in str(e.value), str(e.value)


def test_literal_pins_on_the_real_header(L):
    S = L.SIGNATURES
    assert len(S) == 64 and os.path.samefile(L.HEADER_PATH, os.path.join(ROOT, "include", "xai_hip.h"))
    assert S["xai_gig_step_f32"] == [_p, _p, _p, _i, _l, _i, _f, _d, _p, _p, _p, _p, _p]
    assert S["xai_rise_accum_f64"][9] is _d and S["xai_rise_accum_f64"].count(_d) == 1
    assert S["xai_gradcam_f32"][9] is _z and S["xai_gradcam_f32"].count(_z) == 1
    assert S["xai_lime_max_features"] == [] and S["xai_version"] == []
    args, ret, _ = L.parse_header(open(L.HEADER_PATH).read())
    assert args == S
    assert ret["xai_strerror"] is C.c_char_p
    sized = sorted(n for n, t in ret.items() if t is _z)
    assert sized == ["xai_attn_head_importance_workspace_bytes", "xai_bn_gate_mask_bytes", "xai_gradcam_workspace_bytes",
                     "xai_rank_workspace_bytes", "xai_xrai_workspace_bytes"] == sorted(n for n in S if n.endswith("_bytes"))
    assert all(t is _i for n, t in ret.items() if n != "xai_strerror" and n not in sized)
    _lib_path()
    lib = L.load()                                       # and that is what the loaded functions carry
    assert lib.xai_strerror.restype is C.c_char_p and lib.xai_bn_gate_mask_bytes.restype is _z
    assert list(lib.xai_gig_step_f32.argtypes) == S["xai_gig_step_f32"] and lib.xai_gig_step_f32.restype is _i


def test_version_numbers_are_the_headers_defines(L, monkeypatch, tmp_path):
    hdr = open(os.path.join(ROOT, "include", "xai_hip.h")).read()
    assert L.ABI_VERSION == int(re.search(r"^#define XAI_ABI_VERSION (\d+)$", hdr, flags=re.M).group(1))
    assert L.ABI_MINOR == int(re.search(r"^#define XAI_ABI_MINOR (\d+)$", hdr, flags=re.M).group(1))
    assert (L.ABI_VERSION, L.ABI_MINOR) == L.parse_header(hdr)[2]
    # read once at import, from the record's header_path; a header that is absent or does not parse is an error that names the path
    for name, text in (("absent.h", None), ("broken.h", hdr.replace("int xai_version(void);", "long xai_version(void);"))):
        path = tmp_path / name
        if text is not None:
            path.write_text(text)
        monkeypatch.setattr(L.LIBRARIES["hip"], "header_path", str(path))
        with pytest.raises(L.XaiHipError, match=name):
            L.LIBRARIES["hip"].read_header()
