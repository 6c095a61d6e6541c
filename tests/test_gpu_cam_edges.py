"""K3 (csrc/cam_kernels.hip: gradcam_kernel<PPL>, gradcam_finish_kernel, bilinear_up_kernel) on the MI355X against
tests/cam_restated.py at its edges.

Grad-CAM is held bit for bit to cam_fp32 -- the order the kernel file's header states: channels {wave, wave + 16, ...} ascending per
wave, the butterfly, a true division, wave partials in wave order, slice partials in slice order -- on N(0, 1) data, and element
for element to int64 results on integer data that is exact in any order; the same output lies inside cam_bound around cam64 and
inside the project's 1e-5.  The bilinear kernel is held bit for bit to bilinear_fp32 and inside bilinear_bound around the fp64
interpolation at exact coordinates.  Every output and the workspace live between guard words that must come back untouched, and
every input is read back after the call.  The shrinking cells pin the kernel as PLAIN bilinear; what the reference computes for a
shrinking axis (antialiased) is xai_engine.kernels.resize_bilinear's business, held to torch's CPU op here."""
import copy

import numpy as np
import pytest
import torch

import cam_restated as R
from conftest import BAR, check
from test_cpu_cam import inside, torch_antialiased, torch_plain
from test_gpu_masker_edges import In, Out, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AGAINST = "fp64 restatement"
F32 = np.float32


@pytest.fixture(scope="module")
def K():
    from xai_engine import kernels
    from xai_engine import load_library
    load_library()
    return kernels


@pytest.fixture(scope="module")
def lib(K):
    return __import__("xai_engine")._lib.load()


def run_cam(K, lib, act, grad, relu, ws_mode="full"):
    """xai_gradcam_f32 -> (B, h, w) fp32.  cam and the workspace sit between guard words, checked after the call, as are the
    inputs.  ws_mode: "full" (the workspace xai_gradcam_workspace_bytes asks for), "short" (the same buffer, declared one byte
    short: it must not be written) or "none" (a null pointer)."""
    B, C, h, w = act.shape
    nbytes = lib.xai_gradcam_workspace_bytes(B, C, h, w)
    assert nbytes == 4 * R.workspace_floats(B, C, h * w)
    a, g, out = In(act), In(grad), Out(B * h * w)
    ws = Out(nbytes // 4) if nbytes and ws_mode != "none" else None
    K._call("xai_gradcam_f32", torch.device(DEV), a.ptr, g.ptr, B, C, h, w, int(relu), out.ptr, ws.ptr if ws else None,
            nbytes - 1 if ws_mode == "short" else nbytes)
    got = out.get().view(F32).reshape(B, h, w).copy()
    if ws is not None:
        ws.get()                                           # the words around the workspace
        assert ws_mode == "full" or ws.untouched(), "a workspace declared too small was written"
    a.unchanged(), g.unchanged()
    return got


def held_to_the_restatement(name, got, act, grad, relu, have_ws=True):
    """bits of cam_fp32; inside cam_bound around cam64 (the fraction goes to the ledger at 1.0); the project's norm at 1e-5"""
    same_bits(got, R.cam_fp32(act, grad, relu, have_ws=have_ws), name)
    want = R.cam64(act, grad, relu)
    ratio = inside(got, want, R.cam_bound(act, grad, have_ws=have_ws))
    print(f"{name}: {ratio:.4f} of the derived bound")
    check(name + "/bound", ratio, 0, 1.0, against=AGAINST, absolute=True)
    check(name, got, want, BAR, against=AGAINST)
    if relu:
        raw = R.cam_fp32(act, grad, False, have_ws=have_ws)
        assert (got >= 0).all() and (got.view(np.int32)[raw <= 0] == 0).all(), "a clamped output is not +0.0"


@pytest.mark.parametrize("cell", R.cam_cells(), ids=R.cam_name)
def test_gradcam_cell_has_the_bits_of_the_restatement(K, lib, cell):
    exact = R.exact_case(*cell)
    act, grad = R.normal_case(*cell)
    for relu in (0, 1):
        got = run_cam(K, lib, exact[0], exact[1], relu)
        want = np.maximum(exact[3], 0) if relu else exact[3]
        assert (got == np.rint(got)).all(), "integer data came back with a fraction"
        np.testing.assert_array_equal(got.astype(np.int64), want, err_msg=f"{cell} relu{relu}: integer data")
        held_to_the_restatement(f"cam_edges/cam/{R.cam_name(cell)}/relu{relu}", run_cam(K, lib, act, grad, relu), act, grad, relu)


def test_gradcam_without_enough_workspace_takes_one_slice(K, lib):
    """C = 256 at B = 1 is four slices with the workspace; with a null workspace, or one declared a byte short, the whole image
    goes to one workgroup: the bits of cam_fp32(have_ws=False), which differ from the sliced ones, and nothing written to the
    buffer that was too small."""
    cell = (1, 256, 7, 9)
    assert R.slices_for(1, 256) == (4, 64) and R.slices_for(1, 256, have_ws=False) == (1, 256)
    act, grad = R.normal_case(*cell)
    exact = R.exact_case(*cell)
    assert (R.cam_fp32(act, grad, False).view(np.int32) != R.cam_fp32(act, grad, False, have_ws=False).view(np.int32)).any()
    for mode in ("none", "short", "full"):
        for relu in (0, 1):
            got = run_cam(K, lib, exact[0], exact[1], relu, ws_mode=mode)
            np.testing.assert_array_equal(got.astype(np.int64), np.maximum(exact[3], 0) if relu else exact[3], err_msg=mode)
        held_to_the_restatement(f"cam_edges/cam_no_workspace/{mode}", run_cam(K, lib, act, grad, 0, ws_mode=mode), act, grad, 0,
                                have_ws=mode == "full")
        same_bits(run_cam(K, lib, act, grad, 1, ws_mode=mode), R.cam_fp32(act, grad, True, have_ws=mode == "full"), (mode, "relu"))


def run_bilinear(K, src, H, W, mult, take_abs):
    B, h, w = src.shape
    s, out = In(src), Out(B * H * W)
    K._call("xai_bilinear_up_f32", torch.device(DEV), s.ptr, B, h, w, H, W, float(mult), int(take_abs), out.ptr)
    got = out.get().view(F32).reshape(B, H, W).copy()
    s.unchanged()
    return got


@pytest.mark.parametrize("cell", R.bilinear_cells(), ids=R.bilinear_name)
def test_bilinear_cell_has_the_bits_of_the_restatement(K, cell):
    """... shrinking cells included: the kernel is plain bilinear whatever the sizes.  Identity size: src * mult bit for bit.
    h = 1 (w = 1): the rows (columns) whose vertical (horizontal) weight is 0 are bitwise equal and the others within two blend
    roundings of them -- R.degenerate_axis_holds says why "all bitwise equal" is not a property of this arithmetic."""
    B, h, w, H, W, mult, take_abs = cell
    name = f"cam_edges/bilinear/{R.bilinear_name(cell)}"
    src = R.bilinear_case(cell)
    got = run_bilinear(K, src, H, W, mult, take_abs)
    same_bits(got, R.bilinear_fp32(src, H, W, mult, take_abs), name)
    want = mult * R.bilinear64(src, H, W)
    want = np.abs(want) if take_abs else want
    ratio = inside(got, want, R.bilinear_bound(src, H, W, mult))
    print(f"{name}: {ratio:.4f} of the derived bound")
    check(name + "/bound", ratio, 0, 1.0, against=AGAINST, absolute=True)
    check(name, got, want, BAR, against=AGAINST)
    if (h, w) == (H, W):
        same_bits(got, np.abs(src * F32(mult)) if take_abs else src * F32(mult), (name, "identity"))
    if h == 1:
        assert R.degenerate_axis_holds(src, got, 1, mult)
    if w == 1:
        assert R.degenerate_axis_holds(src, got, 2, mult)
    if take_abs:
        assert (got >= 0).all()
    if (h, w, H, W) in R.SHRINKING and mult == 1.0 and not take_abs:
        plain = torch_plain(src, H, W)
        name = f"cam_edges/bilinear_plain_vs_torch/{R.bilinear_name(cell)}"
        ratio = inside(got, plain.astype(np.float64), R.bilinear_bound(src, H, W))
        print(f"{name}: {ratio:.4f} of the derived bound")
        check(name + "/bound", ratio, 0, 1.0, against="torch cpu, antialias=False", absolute=True)
        check(name, got, plain, BAR, against="torch cpu, antialias=False")
        assert np.abs(got - torch_antialiased(src, H, W)).max() > 0.1       # ... and not the reference's resize


def test_resize_bilinear_is_k3_until_an_axis_shrinks_and_the_antialiased_resize_beyond(K):
    """kernels.resize_bilinear: the bits of bilinear_up where no axis shrinks; the reference's antialiased resize (torch's CPU
    kernel) at the project's bar on the shrinking cells, times the scale, with |.|."""
    for h, w, H, W in R.BILINEAR_SHAPES:
        src = R.bilinear_case((3, h, w, H, W))
        dev = torch.from_numpy(src).to(DEV)
        got = K.resize_bilinear(dev, H, W, scale=3.0, take_abs=True).cpu().numpy()
        if (h, w, H, W) in R.SHRINKS:
            check(f"cam_edges/resize_antialiased/{h}x{w}_to_{H}x{W}", got, np.abs(torch_antialiased(src, H, W) * F32(3)), BAR,
                  against="torch cpu, antialias=True")
        else:
            assert H >= h and W >= w
            same_bits(got, K.bilinear_up(dev, H, W, scale=3.0, take_abs=True).cpu().numpy(), (h, w, H, W))
            same_bits(got, R.bilinear_fp32(src, H, W, 3.0, True), (h, w, H, W))


def test_ablation_maps_follow_the_reference_when_the_sample_grid_is_finer_than_the_image(K):
    """ablation._harness_map with a g x g sample grid of the caller's choosing: g = 6 onto 4 x 5 is |sum_c Resize-antialias| as the
    CPU computes it, for one shared plane (scale 3, abs) and for three separate ones; g = 2 onto 4 x 5 keeps the bits of K3."""
    from xai_engine.ablation import _harness_map
    rng = np.random.default_rng(21)
    fine, coarse = rng.standard_normal((2, 3, 6, 6)).astype(F32), rng.standard_normal((2, 3, 2, 2)).astype(F32)
    dev = torch.from_numpy(fine).to(DEV)
    aa = torch_antialiased(fine.reshape(6, 6, 6), 4, 5).reshape(2, 3, 4, 5)
    check("cam_edges/ablation_map/shared", _harness_map(dev, 4, 5, True).cpu().numpy(), np.abs(aa[:, 0] * F32(3)), BAR,
          against="torch cpu, antialias=True")
    check("cam_edges/ablation_map/per_channel", _harness_map(dev, 4, 5, False).cpu().numpy(), np.abs((aa[:, 0] + aa[:, 1]) + aa[:, 2]), BAR,
          against="torch cpu, antialias=True")
    dev = torch.from_numpy(coarse).to(DEV)
    same_bits(_harness_map(dev, 4, 5, True).cpu().numpy(), R.bilinear_fp32(coarse[:, 0], 4, 5, 3.0, True), "shared, up-sampling")
    up = R.bilinear_fp32(coarse.reshape(6, 2, 2), 4, 5).reshape(2, 3, 4, 5)
    same_bits(_harness_map(dev, 4, 5, False).cpu().numpy(), np.abs((up[:, 0] + up[:, 1]) + up[:, 2]), "per channel, up-sampling")


def test_a_layer_larger_than_the_map_is_resized_as_the_reference_resizes_it():
    """gradcam_saliency on an 8 x 8 layer with out_hw = (4, 5): |channels * Resize-antialias(cam)| as the CPU computes it from the
    CPU's own activations and gradients, eager and as a hipGraph replay (CapturedGradCam.step calls the same function); the plain
    bilinear of K3 is 0.1 and more of the map's maximum away."""
    from oracle import gradcam as ogc
    from xai_engine import gradcam as gc
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, padding=1), torch.nn.ReLU(), torch.nn.AdaptiveAvgPool2d(2), torch.nn.Flatten(),
                              torch.nn.Linear(32, 5)).eval()
    for p in net.parameters():
        p.requires_grad_(False)
    gnet = copy.deepcopy(net).to(DEV)
    out_hw, target = (4, 5), 3

    def reference(x):
        act, grad = ogc.layer_act_and_grad(net, net[0], x, target)
        assert act.shape == (2, 8, 8, 8)
        cam = ogc.cam_reduce(act, grad, relu=True)
        assert cam.max() > 0
        return np.abs(torch_antialiased(cam, *out_hw) * F32(3)), np.abs(ogc.bilinear_up(cam, *out_hw) * F32(3))

    xs = [torch.randn(2, 3, 8, 8, generator=torch.Generator().manual_seed(s)) for s in (1, 2)]
    want, plain = reference(xs[0])
    assert np.abs(want - plain).max() > 0.1 * want.max()
    eager = gc.gradcam_saliency(gnet, gnet[0], xs[0].to(DEV), target, out_hw)
    assert eager.shape == (2, 4, 5)
    check("cam_edges/shrinking_layer/eager", eager.cpu().numpy(), want, BAR, against="cpu, antialias=True")
    before = dict(gc.GRADCAM_COUNTS)
    first = gc.gradcam_saliency(gnet, gnet[0], xs[0].to(DEV), target, out_hw, graphs=True)
    second = gc.gradcam_saliency(gnet, gnet[0], xs[1].to(DEV), target, out_hw, graphs=True)
    assert gc.GRADCAM_COUNTS["captures"] == before["captures"] + 1 and gc.GRADCAM_COUNTS["replayed"] == before["replayed"] + 2, \
        [e.refused for _, e in gc._PASSES.entries().values()]
    check("cam_edges/shrinking_layer/graphs", first.cpu().numpy(), want, BAR, against="cpu, antialias=True")
    check("cam_edges/shrinking_layer/graphs_second_input", second.cpu().numpy(), reference(xs[1])[0], BAR, against="cpu, antialias=True")
