"""Device SLIC on the MI355X: K65-K68 (include/xai_hip_slic.h) and xai_engine/slic.py against the NumPy restatement of the header's
contract (tests/slic_restated.py), which tests/test_cpu_slic.py and the fixture's generator hold to scikit-image 0.18.3's binary.

Everything is exact: the contract fixes the order of every operation, so labels, components and counts are compared as integers and the
centres as bytes, after every iteration, in float32 and float64."""
import functools

import numpy as np
import pytest
import torch

import slic_restated as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TAGS = ["mda", "ragged", "colour", "wide", "one"]
DTYPES = {"f32": np.float32, "f64": np.float64}
# H, W, n_segments: odd, ragged, whole tiles; s441 has step 3 and S = 441 clusters, so K65 lists them in two passes of 256
SEEDED = {"s17": (17, 20, 6), "s37": (37, 53, 12), "s64": (64, 64, 16), "s441": (64, 64, 455)}


@pytest.fixture(scope="module")
def K():
    from xai_engine import kernels
    return kernels


@pytest.fixture(scope="module")
def S():
    from xai_engine import slic
    return slic


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("slic.npz")


def smoothed(seed, H, W, passes):
    """tests/golden/make_golden_slic.py's image generator"""
    img = np.random.RandomState(seed).uniform(size=(H, W, 3))
    for _ in range(passes):
        p = np.pad(img, ((1, 1), (1, 1), (0, 0)), mode="edge")
        img = sum(p[i:i + H, j:j + W] for i in range(3) for j in range(3)) / 9.0
    img = (img - img.min()) / (img.max() - img.min())
    return img.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(tag, name):
    """-> (features (B, H, W, C) T, centres (S, 2), step, (min_size, max_size)) of a fixture case (B = 1) or a seeded one (B = 3:
    three images, the colour term of the same order as the spatial one); never modified"""
    from xai_engine.slic import grid_centroids, size_bounds
    T = DTYPES[name]
    if tag in TAGS:
        g = golden()
        return g[f"{tag}_{name}_features"][None], g[f"{tag}_centroids"], float(g[f"{tag}_step"]), tuple(int(v) for v in g[f"{tag}_sizes"])
    H, W, n = SEEDED[tag]
    rng = np.random.RandomState(H * W + n)
    feat = np.stack([smoothed(rng.randint(1 << 20), H, W, 2) for _ in range(3)]).astype(T) * T(3.0)
    centres, step = grid_centroids(H, W, n)
    return feat, centres, step, size_bounds(H, W, len(centres))


@functools.lru_cache(maxsize=None)
def _want(tag, name):
    """the restatement, image by image -> per iteration the labels (10, B, H, W) and centres (10, B, S, 2 + C), then the status (B,),
    components, final labels and label counts; computed once, never modified"""
    feat, centres, step, (mn, mx) = _case(tag, name)
    labs, cens, stats, comps, finals, counts = [], [], [], [], [], []
    for b in range(feat.shape[0]):
        c = R.initial(centres, feat.shape[3], feat.dtype)
        lab_b, cen_b, st = [], [], 0
        for _ in range(10):
            lab, s1 = R.assign(feat[b], c, step)
            c, s2 = R.update(feat[b], lab, c)
            st |= s1 | s2
            lab_b.append(lab)
            cen_b.append(c)
        comp, s3, _ = R.components(lab, mn, mx)
        final, count = R.number(comp, 0)
        labs.append(lab_b); cens.append(cen_b); stats.append(st | s3); comps.append(comp); finals.append(final); counts.append(count)
    return (np.stack(labs, 1), np.stack(cens, 1), np.array(stats, np.int32), np.stack(comps), np.stack(finals), np.array(counts, np.int32))


CASES = [(t, n) for t in TAGS + list(SEEDED) for n in DTYPES]


@pytest.mark.parametrize("tag,name", CASES)
def test_k65_and_k66_equal_the_restatement_after_every_iteration(K, S, tag, name):
    feat, centres, step, _ = _case(tag, name)
    labs, cens, *_ = _want(tag, name)
    for B in sorted({1, feat.shape[0]}):
        f = _dev(feat[:B])
        c = S.initial_centres(centres, B, feat.shape[3], f.dtype, DEV)
        status = K.slic_clear(torch.empty(B, dtype=torch.int32, device=DEV))
        for it in range(10):
            lab, _ = K.slic_assign(f, c, int(step), status=status)
            assert np.array_equal(lab.cpu().numpy(), labs[it, :B]), (B, it)
            K.slic_update(f, lab, c, int(step), status=status)
            assert c.cpu().numpy().tobytes() == np.ascontiguousarray(cens[it, :B]).tobytes(), (B, it)
        assert (status.cpu().numpy() & 3 == _want(tag, name)[2][:B] & 3).all()


@pytest.mark.parametrize("tag,name", CASES)
def test_k67_and_k68_equal_the_restatement(K, tag, name):
    feat, _, _, (mn, mx) = _case(tag, name)
    labs, _, stats, comps, finals, counts = _want(tag, name)
    for B in sorted({1, feat.shape[0]}):
        raw = _dev(labs[-1][:B])
        status = K.slic_clear(torch.empty(B, dtype=torch.int32, device=DEV))
        comp = K.slic_components(raw, mn, mx, status)
        assert np.array_equal(comp.cpu().numpy(), comps[:B]), B
        assert np.array_equal(status.cpu().numpy(), stats[:B] & R.IRREGULAR), B
        out, n = K.slic_number(comp, 0)
        assert np.array_equal(out.cpu().numpy(), finals[:B]) and np.array_equal(n.cpu().numpy(), counts[:B]), B
        out1, n1 = K.slic_number(comp, 1)
        assert np.array_equal(out1.cpu().numpy(), finals[:B] + 1) and np.array_equal(n1.cpu().numpy(), counts[:B]), B


@pytest.mark.parametrize("tag,name", CASES)
def test_slic_batch_equals_the_restatement_and_skimage_where_the_case_is_regular(S, tag, name):
    feat, centres, step, _ = _case(tag, name)
    labs, cens, stats, _, finals, counts = _want(tag, name)
    for B in sorted({1, feat.shape[0]}):
        labels, n, status, final_centres = S.slic_batch(_dev(feat[:B]), centres, step)
        assert labels.dtype == n.dtype == status.dtype == torch.int32 and labels.is_cuda and final_centres.is_cuda
        assert np.array_equal(labels.cpu().numpy(), finals[:B]) and np.array_equal(n.cpu().numpy(), counts[:B]), B
        assert np.array_equal(status.cpu().numpy(), stats[:B]), B
        assert final_centres.cpu().numpy().tobytes() == np.ascontiguousarray(cens[-1][:B]).tobytes(), B
        raw, n_raw, st_raw, _ = S.slic_batch(_dev(feat[:B]), centres, step, enforce_connectivity=False)
        assert np.array_equal(raw.cpu().numpy(), labs[-1][:B]) and (n_raw.cpu().numpy() == len(centres)).all(), B
        assert np.array_equal(st_raw.cpu().numpy(), stats[:B] & 3), B
        raw1, _, _, _ = S.slic_batch(_dev(feat[:B]), centres, step, enforce_connectivity=False, start_label=1)
        assert raw1.dtype == torch.int32 and np.array_equal(raw1.cpu().numpy(), labs[-1][:B] + 1), B     # skimage's raw labels start there too
    if tag in TAGS:
        g = golden()
        assert np.array_equal(raw[0].cpu().numpy(), g[f"{tag}_{name}_raw"])                      # skimage's own run
        assert final_centres[0].cpu().numpy().tobytes() == g[f"{tag}_{name}_centres"].tobytes()
        assert bool(g[f"{tag}_{name}_regular"]) == (int(status[0]) == 0)
        if int(status[0]) == 0:
            assert np.array_equal(labels[0].cpu().numpy(), g[f"{tag}_{name}_labels"])


@pytest.mark.parametrize("name", DTYPES)
def test_a_tie_goes_to_the_lower_k(K, name):
    T = DTYPES[name]
    feat = np.zeros((1, 4, 9, 1), T)
    cen = np.array([[[1, 2, 0], [1, 6, 0]]], T)                               # column 4 is exactly between the two centres
    lab, status = K.slic_assign(_dev(feat), _dev(cen), 4)
    want, _ = R.assign(feat[0], cen[0], 4)
    got = lab[0].cpu().numpy()
    assert np.array_equal(got, want) and got[:, 4].tolist() == [0] * 4 and got[:, 5].tolist() == [1] * 4 and int(status[0]) == 0
    lab, _ = K.slic_assign(_dev(feat), _dev(np.ascontiguousarray(cen[:, ::-1])), 4)               # the same centres in the other order
    assert lab[0].cpu().numpy()[:, 4].tolist() == [0] * 4 and lab[0].cpu().numpy()[:, 3].tolist() == [1] * 4


@pytest.mark.parametrize("name", DTYPES)
def test_a_tie_between_waves_and_between_listing_passes_goes_to_the_lower_k(K, name):
    """300 clusters: K65 tests them 256 at a time, a wave of 64 lanes each.  Two of them sit at (1, 2) and (1, 6), exactly equidistant
    from column 4; the other 298 share one far centre whose window ends before column 4.  Wherever the two sit -- in two waves of a
    pass, at the last slot of one pass and the first of the next, in either order -- column 4 takes the lower k."""
    T = DTYPES[name]
    feat = np.zeros((1, 4, 40, 1), T)
    for ka, kb in ((10, 70), (70, 10), (10, 290), (290, 70), (255, 256), (256, 255), (63, 64)):
        cen = np.tile(np.array([1, 30, 0], T), (1, 300, 1))                   # window columns [22, 39)
        cen[0, ka], cen[0, kb] = (1, 2, 0), (1, 6, 0)
        lab, status = K.slic_assign(_dev(feat), _dev(cen), 4)
        want, st = R.assign(feat[0], cen[0], 4)
        got = lab[0].cpu().numpy()
        assert np.array_equal(got, want) and int(status[0]) == st == R.UNCOVERED, (ka, kb)        # columns 15 - 21 and 39 are in no window
        assert got[:, 4].tolist() == [min(ka, kb)] * 4 and got[:, 3].tolist() == [ka] * 4 and got[:, 5].tolist() == [kb] * 4, (ka, kb)
        assert (got[:, 22:39] == min(set(range(300)) - {ka, kb})).all(), (ka, kb)


def test_the_sweep_cap_that_runs_out_is_reported_and_an_unsettled_pixel_is_never_followed(K):
    """A path of label 0 down column 0, across the bottom, up column 2 and along row 0: the least index reaches the top of column 2
    one pixel per sweep, so the height decides whether XAI_SLIC_MAX_SWEEPS = 64 sweeps are enough.  57 rows settle in the 64th sweep;
    58 rows are settled but the sweep that would prove it is the 65th; at 59 rows the cap falls while the pixels of row 0 still
    point to a pixel that is no first pixel any more, and K68 numbers those -1; at 66 rows column 2 is cut in two.  The size bounds
    admit everything, so the IRREGULAR bit is the cap's alone.  The counts say how each case was chosen (from the restatement)."""
    seen = {}
    for H in (57, 58, 59, 66):
        lab = np.ones((2, H, 12), np.int32)
        lab[0, :, 0] = lab[0, -1, 1] = lab[0, :, 2] = lab[0, 0, 2:] = 0       # image 1 is one component: it settles at once
        want, st, sweeps = R.components(lab[0], 0, 1 << 30)
        flat = want.ravel()
        loose = flat[flat] != flat
        seen[H] = (st, sweeps, int(loose.sum()))
        status = K.slic_clear(torch.empty(2, dtype=torch.int32, device=DEV))
        comp = K.slic_components(_dev(lab), 0, 1 << 30, status)
        assert status.tolist() == [st, 0], H
        assert np.array_equal(comp[0].cpu().numpy(), want) and (comp[1].cpu().numpy() == 0).all(), H
        out, n = K.slic_number(comp, 1)
        first = flat == np.arange(flat.size)
        numbered = np.where(loose, -1, 1 + (np.cumsum(first) - 1)[flat]).reshape(H, 12)
        assert np.array_equal(out[0].cpu().numpy(), numbered) and n.tolist() == [int(first.sum()), 1] and (out[1].cpu().numpy() == 1).all(), H
    assert seen == {57: (0, 64, 0), 58: (R.IRREGULAR, 64, 0), 59: (R.IRREGULAR, 64, 9), 66: (R.IRREGULAR, 64, 0)}


def test_k67_and_k68_refuse_an_output_that_overlaps_their_input(K):
    lab = torch.zeros((2, 5, 7), dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="comp must not overlap labels"):
        K.slic_components(lab, 0, 100, comp=lab)
    comp = K.slic_components(lab, 0, 100)
    with pytest.raises(ValueError, match="out must not overlap comp"):
        K.slic_number(comp, 0, out=comp)
    both = torch.zeros((3, 5, 7), dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="out must not overlap comp"):        # a view that shares one image
        K.slic_number(both[:2], 0, out=both[1:])
    out, n = K.slic_number(both[:1], 0, out=both[1:2])                       # neighbours in one allocation share no byte
    assert n.tolist() == [1] and (out.cpu().numpy() == 0).all()


@pytest.mark.parametrize("name", DTYPES)
def test_an_uncovered_pixel_and_an_empty_cluster_are_reported(K, S, name, monkeypatch):
    T = DTYPES[name]
    feat = np.zeros((2, 4, 30, 1), T)
    cen = np.array([[1, 2]])                                                  # window columns [0, 7): 23 columns in no window
    lab, status = K.slic_assign(_dev(feat), S.initial_centres(cen, 2, 1, _dev(feat).dtype, DEV), 2)
    want, st = R.assign(feat[0], R.initial(cen, 1, T), 2)
    assert st == R.UNCOVERED and status.tolist() == [R.UNCOVERED] * 2
    assert np.array_equal(lab[0].cpu().numpy(), want) and np.array_equal(lab[1].cpu().numpy(), want) and (want[:, 7:] == -1).all()
    labels, n, status, _ = S.slic_batch(_dev(feat), cen, 2, max_iter=3)
    assert (status.cpu().numpy() & R.UNCOVERED).all()
    feat = np.zeros((1, 6, 6, 1), T)
    twins = np.array([[2, 2], [2, 2]])                                        # the twin loses every tie: no pixel
    labels, n, status, centres = S.slic_batch(_dev(feat), twins, 3, max_iter=3)
    raw, trace, st = R.kmeans(feat[0], R.initial(twins, 1, T), 3, 3)
    assert st == R.EMPTY and int(status[0]) & R.EMPTY and not int(status[0]) & R.UNCOVERED
    got = centres[0].cpu().numpy()
    assert np.isnan(got[1]).all() and got[0].tobytes() == trace[-1][0].tobytes()
    # slic() raises what slic_batch reports; its own grid never produces either state, so the crafted centres are planted
    monkeypatch.setattr(S, "grid_centroids", lambda H, W, n: (twins, 3.0))
    with pytest.raises(S.XaiHipError, match="no pixel"):
        S.slic(np.zeros((6, 6), T), n_segments=2, max_iter=3, device=DEV)
    monkeypatch.setattr(S, "grid_centroids", lambda H, W, n: (cen, 2.0))
    with pytest.raises(S.XaiHipError, match="no cluster's window"):
        S.slic(np.zeros((4, 30), T), n_segments=1, max_iter=3, device=DEV)


def test_an_irregular_case_is_finished_on_the_host_and_equals_skimage(S):
    """The fixture's features go in as the image with convert2lab off and compactness 1, so `image * (1 / 1)` is the features bit for
    bit: `colour` and `wide` are irregular, the device reports it, and the host pass from the raw labels gives skimage's labels."""
    g = golden()
    for tag, n in (("colour", 12), ("wide", 20)):
        for name in DTYPES:
            feat = g[f"{tag}_{name}_features"]
            _, _, status, _ = S.slic_batch(_dev(feat[None]), g[f"{tag}_centroids"], float(g[f"{tag}_step"]))
            assert int(status[0]) == S.IRREGULAR
            got = S.slic(feat, n_segments=n, compactness=1.0, convert2lab=False, start_label=0, device=DEV)
            assert got.dtype == np.int64 and np.array_equal(got, g[f"{tag}_{name}_labels"])
    raw = g["conn1_raw"].astype(np.int64)                                     # and the restated pass where skimage is absent
    mn, mx = (int(v) for v in g["conn1_sizes"])
    assert np.array_equal(S._finish_on_host(raw, mn, mx, 0), g["conn1_labels"])


def test_slic_with_skimages_signature_equals_skimage_at_224_from_the_engines_own_lab(S):
    """224 x 224, 196 segments, compactness 10000, float32: MDA's call.  The features come from the engine's own rgb2lab, which may
    differ from skimage's in the last bits (tests/test_cpu_slic.py bounds it).  That cannot move a label here: a Lab difference is at
    most 255 / 10000 per channel, so the colour term is at most 3 * 0.0255^2 = 0.002 and changes between neighbouring pixels by far
    less, while the spatial term of two clusters competing for a pixel differs by at least 1 / step^2 = 0.0039 per pixel of distance
    unless the pixel is equidistant; a last-bit change of the features moves the colour term by about 1e-10, below half an ulp
    (3e-8) of a spatial term of the order of 1."""
    g = golden()
    img = smoothed(int(g["big_seed"]), 224, 224, 2)
    got = S.slic(img, n_segments=196, compactness=10000, start_label=0, device=DEV)
    assert got.dtype == np.int64 and got.shape == (224, 224) and np.array_equal(got, g["big_labels"])
    assert np.array_equal(S.slic(img, n_segments=196, compactness=10000, device=DEV), got)        # start_label None is 0, as in 0.18.3


def test_two_calls_give_the_same_bytes_and_a_captured_graph_replays_the_eager_launches(S):
    feat, centres, step, _ = _case("s37", "f32")
    f = _dev(feat).clone()
    init = S.initial_centres(centres, 3, 3, f.dtype, DEV)

    def run():
        c = init.clone()
        labels, n, status, _ = S.slic_batch(f, c, step)
        return labels, n, status, c
    first = [t.cpu().numpy().tobytes() for t in run()]
    assert first == [t.cpu().numpy().tobytes() for t in run()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = run()
    other = _dev(_case("s37", "f32")[0][[2, 0, 1]])
    for src, want in ((_dev(feat), first), (other, None), (_dev(feat), first)):
        f.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.cpu().numpy().tobytes() for t in out]
        assert got == (want or [t.cpu().numpy().tobytes() for t in run()])


def _vit_case():
    from helpers import vit_mini_from
    from xai_engine import kernels as K
    from xai_engine.blur import blur_until_unconfident
    from xai_engine.vit_attr import Baselines
    v, g = load_golden("vit_mini.npz"), golden()
    model = vit_mini_from(v, DEV)
    x = torch.from_numpy(v["x"])
    t = torch.tensor(int(v["target"]))
    trans = torch.from_numpy(smoothed(int(g["small_seed"]), 32, 32, 1).transpose(2, 0, 1).copy())[None]
    blur, _, _, _ = blur_until_unconfident(model, x, t, DEV)
    bi, _ = Baselines(model).bidirectional(x.to(DEV), t, device=torch.device(DEV))
    bi = K.resize_bilinear(bi.detach().float().contiguous(), 32, 32)[0].cpu().numpy()[:, :, None] * np.ones((32, 32, 3))
    return model, x, t, trans, blur, bi, torch.from_numpy(g["small_labels"].astype(np.int64))


def test_mda_with_the_device_segmenter_gives_the_maps_of_skimages_segments():
    from xai_engine.mda import MDA, slic_segments
    model, x, t, trans, blur, bi, seg = _vit_case()
    got_seg = slic_segments(trans, 16, "device", DEV)
    assert got_seg.dtype == torch.int64 and torch.equal(got_seg, seg)
    got = MDA(trans, x, bi, 16, blur, model, DEV, 32, max_batch_size=5, segments="device")
    want = MDA(None, x, bi, 16, blur, model, DEV, 32, max_batch_size=5, segments=seg)
    assert len(got) == len(want) == 3 and all(np.array_equal(a, b) for a, b in zip(got, want))


def test_harness_row_with_the_device_key_needs_no_skimage_and_no_segments(monkeypatch):
    import sys
    from xai_engine.mda import MDA
    from xai_engine.sweep import get_VIT_attr
    model, x, t, trans, blur, bi, seg = _vit_case()
    for mod in [m for m in sys.modules if m == "skimage" or m.startswith("skimage.")]:
        monkeypatch.delitem(sys.modules, mod)
    monkeypatch.setitem(sys.modules, "skimage", None)                        # `import skimage` raises ImportError from here on
    td = {"models": [model, model], "img_hw": 32, "batch_size": 25, "device": DEV, "num_patches": 4, "attr_func": "MDA", "mda_slic": "device"}
    got = get_VIT_attr(x.clone(), trans, t, td)
    mda, _, _ = MDA(None, x, bi, 16, blur, model, DEV, 32, max_batch_size=5, segments=seg)
    assert got.shape == (32, 32) and np.array_equal(got, np.abs(np.sum(mda, axis=2)).astype(np.float32))
    with pytest.raises(ValueError, match="mda_slic"):
        get_VIT_attr(x.clone(), trans, t, dict(td, mda_slic="cuda"))
    with pytest.raises(ImportError, match="scikit-image"):                    # the default still asks for skimage, and says so
        get_VIT_attr(x.clone(), trans, t, dict(td, mda_slic="skimage"))
