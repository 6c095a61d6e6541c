"""GradientShap without a GPU: the harness row's place and the CLI, the extension library (include/xai_hip_ext.h bound by the
strict header reader, its exports, its version pair, the two kernels' argument checks made before any HIP call), the frozen main
library beside it, the NumPy draws, the refusals, and the restatement (tests/gshap_restated.py) against the closed form of the
method on a linear classifier -- not against captum, which is on neither machine (parity with captum itself is unpinned)."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import gshap_restated as R
from abi_libs import built, declared, exported, exported_elsewhere
from conftest import PKG, ROOT
from helpers import TinyNet

EXT_HEADER = os.path.join(ROOT, "include", "xai_hip_ext.h")
_p, _i, _l = C.c_void_p, C.c_int, C.c_int64


# ------------------------------------------------------------------------------------------------ the harness row and the CLI
def test_gs_is_a_cnn_attribution_between_lime_and_sg_and_in_the_cli():
    from xai_engine.sweep import CNN_ATTR_FUNCS, TRANS_ATTR_FUNCS
    from xai_engine.evaluate_perturbation import build_parser
    i = CNN_ATTR_FUNCS.index("gs")
    assert CNN_ATTR_FUNCS[i - 1] == "lime" and CNN_ATTR_FUNCS[i + 1] == "sg" and "gs" not in TRANS_ATTR_FUNCS
    # what the rows before it pin still holds
    j = CNN_ATTR_FUNCS.index("xrai")
    assert CNN_ATTR_FUNCS[j - 1] == "sg" and CNN_ATTR_FUNCS[j + 1] == "gc"
    assert CNN_ATTR_FUNCS[-5:] == ("gc", "gbp", "ggc", "fa", "occ")
    assert len(CNN_ATTR_FUNCS) == len(set(CNN_ATTR_FUNCS)) == 16             # the reference's dispatch, :99-176
    assert " gs," in build_parser().format_help()


def test_driver_and_class_carry_the_stated_parameter_names():
    from xai_engine import gshap
    p = inspect.signature(gshap.gradient_shap_batch).parameters
    assert list(p) == ["x", "model", "targets", "baselines", "n_samples", "stdevs", "want_attr", "want_map", "pass_images", "streams",
                       "graphs", "draws"]
    assert [p[k].default for k in list(p)[4:]] == [5, 0.0, True, False, None, 1, True, None]
    p = inspect.signature(gshap.GradientShap.attribute).parameters
    assert list(p) == ["self", "inputs", "baselines", "n_samples", "stdevs", "target"]
    assert (p["n_samples"].default, p["stdevs"].default, p["target"].default) == (5, 0.0, None)
    assert list(inspect.signature(gshap.GradientShap.__init__).parameters) == ["self", "model"]
    assert set(gshap.GSHAP_COUNTS) == {"captures", "captures_refused", "replayed", "eager"}


def test_engine_refuses_the_cpu_and_bad_arguments_before_any_buffer_is_made():
    from xai_engine import XaiHipError, gshap
    from xai_engine import kernels as K
    x, net, base = torch.zeros(2, 3, 8, 8), TinyNet().eval(), torch.zeros(1, 3, 8, 8)
    with pytest.raises(XaiHipError):
        gshap.gradient_shap_batch(x, net, 0, base)
    with pytest.raises(XaiHipError):
        gshap.GradientShap(net).attribute(x, base, target=0)
    with pytest.raises(NotImplementedError):
        gshap.gradient_shap_batch((x, x), net, 0, base)
    with pytest.raises(XaiHipError):
        K.gshap_scale(x, base, torch.zeros(10), torch.zeros(10, dtype=torch.int64), 5)
    with pytest.raises(XaiHipError):
        K.gshap_finish(torch.zeros(10, 3, 8, 8), x, base, torch.zeros(10, dtype=torch.int64), 5)
    # past the device check the argument checks come before any buffer or graph: on a box without a GPU a tensor class that
    # claims to be a device tensor stands in for one
    class FakeCuda(torch.Tensor):
        is_cuda = True

    def dev_t(*shape):
        return torch.zeros(*shape, device="cuda") if torch.cuda.is_available() else torch.zeros(*shape).as_subclass(FakeCuda)
    fx, fb = dev_t(2, 3, 8, 8), dev_t(1, 3, 8, 8)
    for bad_base in (dev_t(1, 3, 8, 9), dev_t(3, 8, 8), dev_t(0, 3, 8, 8), dev_t(1, 1, 8, 8)):
        with pytest.raises(ValueError, match="baselines must be"):
            gshap.gradient_shap_batch(fx, net, 0, bad_base)
    with pytest.raises(XaiHipError, match="baselines"):
        gshap.gradient_shap_batch(fx, net, 0, torch.zeros(1, 3, 8, 8))               # a CPU baseline
    for n in (0, -3):
        with pytest.raises(ValueError, match="n_samples"):
            gshap.gradient_shap_batch(fx, net, 0, fb, n_samples=n)
    with pytest.raises(ValueError, match="nothing to return"):
        gshap.gradient_shap_batch(fx, net, 0, fb, want_attr=False)
    with pytest.raises(NotImplementedError, match="stdevs"):
        gshap.gradient_shap_batch(fx, net, 0, fb, stdevs=(0.1,))
    with pytest.raises(NotImplementedError):
        gshap.GradientShap(net).attribute(fx, fb)                                     # target=None
    assert gshap._PASSES.entries() == {}


# ------------------------------------------------------------------------------------------------ the extension library
def test_extension_header_parses_with_the_strict_reader_and_the_table_equals_the_parse():
    from xai_engine import _lib
    rec = _lib.LIBRARIES["ext"]
    assert os.path.samefile(rec.header_path, EXT_HEADER)
    text = open(EXT_HEADER).read()
    args, ret, version = _lib.parse_header(text, rec.defines)
    assert args == rec.signatures and sorted(args) == declared(EXT_HEADER)
    assert version == (rec.version, rec.minor)
    assert rec.version == int(re.search(r"^#define XAI_EXT_VERSION (\d+)$", text, flags=re.M).group(1))
    assert rec.minor == int(re.search(r"^#define XAI_EXT_MINOR (\d+)$", text, flags=re.M).group(1))
    assert args["xai_ext_version"] == [] and args["xai_ext_version_minor"] == []
    assert args["xai_gshap_scale_f32"] == [_p, _p, _p, _p, _i, _i, _l, _i, _i, _p, _p]
    assert args["xai_gshap_finish_f32"] == [_p, _p, _p, _p, _i, _i, _i, _l, _i, _i, _p, _p, _p]
    assert all(t is _i for t in ret.values())
    # the two headers do not share a name, and the main table is the main header's alone
    assert not set(args) & set(_lib.SIGNATURES)
    # every launch entry cites the line it replaces
    for name in args:
        if name.endswith("_f32"):
            at = text.index(name + "(")
            assert "evaluatePerturbation.py:164-167" in text[text.rfind("/*", 0, at):at], name


def test_the_default_of_parse_header_is_the_main_headers_pair():
    from xai_engine import _lib
    assert inspect.signature(_lib.parse_header).parameters["defines"].default == ("XAI_ABI_VERSION", "XAI_ABI_MINOR")
    main = open(_lib.HEADER_PATH).read()
    assert _lib.parse_header(main) == _lib.parse_header(main, _lib.ABI_DEFINES)
    assert _lib.parse_header(main)[0] == _lib.SIGNATURES
    with pytest.raises(_lib.XaiHipError, match="XAI_EXT_MINOR"):
        _lib.parse_header(main, _lib.LIBRARIES["ext"].defines)       # the pair asked for is the pair required
    with pytest.raises(_lib.XaiHipError, match="XAI_ABI_MINOR"):
        _lib.parse_header(open(EXT_HEADER).read())


def _ext_with(extra, drop=None):
    text = open(EXT_HEADER).read()
    if drop is not None:
        assert drop in text
        text = text.replace(drop, "")
    anchor = "int xai_ext_version_minor(void);"
    assert anchor in text
    return text.replace(anchor, anchor + "\n" + extra)


@pytest.mark.parametrize("text, quoted", [
    (lambda: _ext_with("int xai_count(unsigned n);"), "int xai_count(unsigned n)"),
    (lambda: _ext_with("struct xai_pair { int a; int b; };"), "struct xai_pair { int a"),
    (lambda: _ext_with("int xai_ext_version(void);"), "int xai_ext_version(void)"),
    (lambda: _ext_with("#define XAI_TWO_LINES(a) \\\n  ((a) + 1)"), "#define XAI_TWO_LINES(a) \\"),
    (lambda: _ext_with("int xai_no_stream_f32(const float* x, int n);"), "int xai_no_stream_f32(const float* x, int n)"),
    (lambda: _ext_with("int xai_late_f32(xai_stream_t stream, int n);"), "int xai_late_f32(xai_stream_t stream, int n)"),
    (lambda: _ext_with("int xai_stream_bytes(xai_stream_t stream);"), "int xai_stream_bytes(xai_stream_t stream)"),
    (lambda: _ext_with("float xai_ratio(int n);"), "float xai_ratio(int n)"),
    (lambda: _ext_with("int other_name(int n);"), "int other_name(int n)"),
    (lambda: _ext_with("int xai_left_over(int n)"), "int xai_left_over(int n)"),
    (lambda: _ext_with("", drop="#define XAI_EXT_MINOR 0\n"), "XAI_EXT_MINOR"),
    (lambda: _ext_with("#define XAI_EXT_MINOR 43"), "#define XAI_EXT_MINOR 43"),
    (lambda: _ext_with("", drop="typedef void* xai_stream_t; /* hipStream_t; the same typedef as xai_hip.h's */\n"), "typedef void* xai_stream_t"),
    (lambda: _ext_with("", drop='extern "C" {\n'), 'extern "C"'),
])
def test_reader_refuses_a_broken_extension_header_and_quotes_the_statement(text, quoted):
    from xai_engine import _lib
    with pytest.raises(_lib.XaiHipError) as e:
        _lib.parse_header(text(), _lib.LIBRARIES["ext"].defines)
    assert quoted in str(e.value), str(e.value)


def test_extension_library_exports_exactly_its_header_and_the_main_library_still_its_64():
    from xai_engine import _lib, LIB_PATH
    assert exported(built("ext")) == declared(EXT_HEADER) == sorted(_lib.LIBRARIES["ext"].signatures)
    main = exported(LIB_PATH)
    assert main == declared(os.path.join(ROOT, "include", "xai_hip.h")) and len(main) == 64
    assert not [(o, n) for o, n in exported_elsewhere("ext") if "gshap" in n or "_ext_" in n]         # nor any of the others
    assert (_lib.ABI_VERSION, _lib.ABI_MINOR) == (1, 11)


def test_both_kernels_check_their_arguments_without_a_gpu():
    from xai_engine import _lib
    built("ext")
    lib = _lib.load("ext")
    p = 16                               # a non-NULL pointer that is never dereferenced: validation comes first

    def scale(x=p, base=p, alpha=p, idx=p, out=p, rows=10, n=5, E=147, nb=1, per_row=0):
        return lib.xai_gshap_scale_f32(x, base, alpha, idx, rows, n, E, nb, per_row, out, None)
    assert scale(x=None) == -1 and scale(base=None) == -1 and scale(alpha=None) == -1 and scale(idx=None) == -1 and scale(out=None) == -1
    assert scale(rows=0) == -2 and scale(n=0) == -2 and scale(E=0) == -2 and scale(nb=0) == -2 and scale(rows=-5) == -2
    assert scale(rows=7) == -2                                                    # no multiple of n_samples

    def finish(g=p, x=p, base=p, idx=p, attr=p, out=p, B=2, n=5, Cc=3, HW=49, nb=1, per_row=0):
        return lib.xai_gshap_finish_f32(g, x, base, idx, B, n, Cc, HW, nb, per_row, attr, out, None)
    assert finish(g=None) == -1 and finish(x=None) == -1 and finish(base=None) == -1 and finish(idx=None) == -1
    assert finish(attr=None, out=None) == -1
    assert finish(B=0) == -2 and finish(n=0) == -2 and finish(Cc=0) == -2 and finish(HW=0) == -2 and finish(nb=-1) == -2
    # the codes are the main header's, the texts come from xai_strerror
    assert b"NULL" in _lib.load().xai_strerror(scale(x=None))
    with pytest.raises(_lib.XaiHipError, match="xai_gshap_scale_f32 failed with code -1: required pointer is NULL"):
        _lib.check(scale(x=None), "xai_gshap_scale_f32")


# ------------------------------------------------------------------------------------------------ the draws
@pytest.mark.parametrize("n_base, n, B", [(1, 5, 1), (3, 5, 2)])
def test_draw_is_captums_two_numpy_calls_in_order(n_base, n, B):
    from xai_engine import gshap
    np.random.seed(0)
    want_idx = np.random.choice(n_base, n * B)
    want_alpha = np.random.uniform(0, 1, n * B).astype(np.float32)
    after = np.random.get_state()
    np.random.seed(0)
    idx, alpha = gshap.draw(n_base, n * B)
    assert idx.dtype == want_idx.dtype and alpha.dtype == np.float32
    assert np.array_equal(idx, want_idx) and np.array_equal(alpha, want_alpha)
    now = np.random.get_state()
    assert now[0] == after[0] and np.array_equal(now[1], after[1]) and now[2:] == after[2:]      # the state is where the two calls leave it
    if (n_base, n, B) == (1, 5, 1):
        assert np.array_equal(alpha[:2], np.float32([0.5488135, 0.71518934])) and not idx.any()
    else:
        assert idx.tolist() == [0, 1, 0, 1, 1, 2, 0, 2, 0, 0]
    np.random.seed(0)
    r_idx, r_alpha = R.draw(n_base, n * B)                                          # and the restatement draws the same
    assert np.array_equal(r_idx, want_idx) and np.array_equal(r_alpha, want_alpha) and r_alpha.dtype == np.float32


def test_draws_given_by_the_caller_are_checked_on_the_host():
    from xai_engine import gshap
    idx, alpha = gshap._upload_draws(([0, 2, 1, 1], [0.0, 0.25, 0.5, 1.0]), 3, 4, "cpu")
    assert idx.dtype == torch.int64 and idx.tolist() == [0, 2, 1, 1] and alpha.dtype == torch.float32 and alpha.tolist() == [0.0, 0.25, 0.5, 1.0]
    for bad in (([0, 3, 1, 1], [0.0] * 4), ([0, -1, 1, 1], [0.0] * 4), ([0, 1, 1], [0.0] * 4), ([0.0, 1.0, 1.0, 1.0], [0.0] * 4),
                ([0, 1, 1, 1], [0.0] * 3)):
        with pytest.raises(ValueError):
            gshap._upload_draws(bad, 3, 4, "cpu")


# ------------------------------------------------------------------------------------------------ the restatement vs the closed form
def _linear(C_, H, W, classes, seed):
    g = torch.Generator().manual_seed(seed)
    lin = torch.nn.Linear(C_ * H * W, classes, bias=True)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(lin.weight.shape, generator=g))
        lin.bias.copy_(torch.randn(classes, generator=g))
    return torch.nn.Sequential(torch.nn.Flatten(), lin).double().eval()


def test_restatement_on_a_linear_classifier_is_x_minus_the_mean_baseline_times_the_class_row():
    """logits = W . flatten(x) + c: the gradient at every interpolant is W[t], so the attribution is (x - mean of the chosen
    baselines) * W[t] whatever the coefficients are."""
    B, n, N_b = 2, 5, 3
    model = _linear(3, 6, 5, 7, seed=0)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 3, 6, 5, generator=g, dtype=torch.float64)
    base = torch.randn(N_b, 3, 6, 5, generator=g, dtype=torch.float64) + 0.5
    t = torch.tensor([4, 1])
    np.random.seed(0)
    state = np.random.get_state()
    idx, _ = R.draw(N_b, n * B)
    np.random.set_state(state)
    for pass_images in (None, 1):
        np.random.set_state(state)
        got = R.gradient_shap(model, x, t, base, n_samples=n, pass_images=pass_images)
        Wt = model[1].weight.detach()[t].view(B, 3, 6, 5)
        b_bar = base[torch.from_numpy(idx)].view(B, n, 3, 6, 5).mean(1)
        want = (x - b_bar) * Wt
        assert float((got - want).abs().max()) <= 1e-6 * float(want.abs().max())
        # ... and that is no `grad` or `inp_x_grad` row: with a baseline that is not zero it is off by more than a tenth of its size
        assert float((got - x * Wt).abs().max()) > 0.1 * float(got.abs().max())
    # the draws= override gives the same as the NumPy state it stands for
    np.random.set_state(state)
    draws = R.draw(N_b, n * B)
    again = R.gradient_shap(model, x, t, base, n_samples=n, draws=draws)
    assert torch.equal(again, got)
    m = R.harness_map(got[0])
    assert m.shape == (6, 5) and np.array_equal(m, ((got[0][0] + got[0][1]) + got[0][2]).abs().numpy())


def test_restatement_in_fp32_on_a_relu_classifier_depends_on_the_coefficients_and_draws_no_noise_at_zero():
    torch.manual_seed(0)
    net = TinyNet().eval()
    g = torch.Generator().manual_seed(2)
    x, base, t = torch.randn(2, 3, 8, 8, generator=g), torch.randn(1, 3, 8, 8, generator=g), torch.tensor([3, 8])
    idx = np.zeros(10, np.int64)
    a1 = np.linspace(0.05, 0.95, 10).astype(np.float32)
    before = torch.get_rng_state()
    one = R.gradient_shap(net, x, t, base, draws=(idx, a1))
    assert torch.equal(torch.get_rng_state(), before)                               # stdevs == 0: nothing drawn from torch
    two = R.gradient_shap(net, x, t, base, draws=(idx, a1[::-1].copy()))
    assert one.dtype == torch.float32 and one.shape == x.shape and not torch.equal(one, two)
    cut = R.gradient_shap(net, x, t, base, draws=(idx, a1), pass_images=1)                         # rows are independent
    assert float((cut - one).abs().max()) <= 1e-5 * float(one.abs().max())
    noisy = R.gradient_shap(net, x, t, base, stdevs=0.1, draws=(idx, a1))
    assert not torch.equal(torch.get_rng_state(), before) and not torch.equal(noisy, one)
    # the mean: from +0, so a pixel whose terms are all -0 gives +0; a true division
    term = torch.full((5, 1), -0.0)
    assert torch.equal(R.sample_mean(term, 5).view(torch.int32), torch.zeros(1, 1, dtype=torch.int32))
    v = torch.tensor([[0.1], [0.2], [0.3], [0.4], [0.7]])
    want = np.float32(np.float32(np.float32(np.float32(np.float32(0.1) + np.float32(0.2)) + np.float32(0.3)) + np.float32(0.4)) + np.float32(0.7))
    assert float(R.sample_mean(v, 5)) == float(np.float32(want / np.float32(5)))


# ------------------------------------------------------------------------------------------------ captum
CAPTUM = textwrap.dedent("""
    import sys
    sys.path.insert(0, sys.argv[2]); sys.path.insert(0, sys.argv[1])
    import captum.attr
    before = dict(vars(captum.attr))
    import xai_engine.gshap as gs
    import xai_engine.guided
    assert captum.attr.GradientShap.WHO == "captum"                                  # not asked: untouched
    assert gs.patch_captum() is before["GradientShap"]
    from captum.attr import GradientShap, GuidedBackprop
    assert GradientShap is gs.GradientShap and GuidedBackprop.WHO == "captum"
    changed = sorted(k for k, v in vars(captum.attr).items() if before.get(k) is not v)
    assert changed == ["GradientShap"], changed
    assert gs.patch_captum() is gs.GradientShap
    print("captum ok")
""")


def test_patch_captum_rebinds_exactly_the_one_name(tmp_path):
    pkg = tmp_path / "site" / "captum" / "attr"
    pkg.mkdir(parents=True)
    (tmp_path / "site" / "captum" / "__init__.py").write_text("")
    (pkg / "__init__.py").write_text("".join(f"class {n}: WHO = 'captum'\n" for n in ("GradientShap", "GuidedBackprop", "LayerGradCam")))
    env = {k: v for k, v in os.environ.items() if k not in ("PYTHONPATH", "XAI_PATCH_CAPTUM")}
    r = subprocess.run([sys.executable, "-c", CAPTUM, PKG, str(tmp_path / "site")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "captum ok" in r.stdout, r.stdout + r.stderr
    from xai_engine import gshap
    try:
        import captum  # noqa: F401
    except ImportError:
        assert gshap.patch_captum() is None
