"""The argument checks of xai_engine/kernels.py as the callers see them, wrapper by wrapper: a caller's buffer of the right size
gives what the allocating call gives (torch.equal), one of the wrong element count is a ValueError with the wrapper's own text,
one of the wrong dtype a TypeError, a strided one a ValueError; the BatchNorm wrappers refuse a mis-shaped identity / gy2 / code
and a gate mask one byte short.  Every refusal is raised before anything is launched; the shapes are the smallest that reach
each path."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64, I32, U8 = torch.float32, torch.float64, torch.int32, torch.uint8


@pytest.fixture(scope="module")
def K():
    from xai_engine import kernels
    from xai_engine import load_library
    load_library()
    return kernels


def rand(*shape, seed=0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def strided(shape, dtype):
    """A tensor of `shape` (so of the right element count) that is not contiguous: every second element of a twice as wide one."""
    return torch.zeros(tuple(shape[:-1]) + (2 * shape[-1],), dtype=dtype, device=DEV)[..., ::2]


def buffer_cases(call, name, shape, wrong_size, dtype=F32, other=F64, fill=torch.empty):
    """call(buf) runs the wrapper with `buf` as its buffer `name` and returns the tensor that buffer holds afterwards (call(None):
    the one the wrapper allocated)."""
    want = call(None)
    assert want.dtype == dtype and tuple(want.shape) == tuple(shape)
    buf = fill(shape, dtype=dtype, device=DEV)
    got = call(buf)
    assert got.data_ptr() == buf.data_ptr() and torch.equal(got, want)
    n = want.numel()
    for bad in (n - 1, n + 1):
        with pytest.raises(ValueError, match=wrong_size):
            call(torch.zeros(bad, dtype=dtype, device=DEV))
    with pytest.raises(TypeError, match=name):
        call(torch.zeros(shape, dtype=other, device=DEV))
    with pytest.raises(ValueError, match=f"{name} must be contiguous"):
        call(strided(shape, dtype))


def test_ig_interp_out(K):
    x, alphas = rand(2, 3, 4, 4), torch.tensor([0.0, 0.5, 1.0], device=DEV)
    buffer_cases(lambda out: K.ig_interp(x, 0.25, alphas, out=out), "out", (2, 3, 3, 4, 4), "^out has the wrong size$")


def test_perturb_batch_out(K):
    start, finish = rand(3, 4, 4), rand(3, 4, 4, seed=1)
    flip = (torch.arange(16, dtype=I32, device=DEV) % 3).contiguous()
    buffer_cases(lambda out: K.perturb_batch(start, finish, flip, 1, 2, out=out), "out", (2, 3, 4, 4), "^out has the wrong size$")


def test_guided_map_attr_and_map(K):
    grad, cam = rand(2, 3, 4, 4), rand(2, 2, 2, seed=1)
    both = lambda **kw: K.guided_map(grad, cam, want_attr=True, want_map=True, **kw)
    buffer_cases(lambda attr: both(attr=attr)[0], "attr", (2, 3, 4, 4), "^attr has the wrong size$")
    buffer_cases(lambda map: both(map=map)[1], "map", (2, 4, 4), "^map has the wrong size$")
    a, m = both()
    assert torch.equal(K.guided_map(grad, cam, attr=torch.empty_like(grad)), a)
    assert torch.equal(K.guided_map(grad, cam, want_attr=False, want_map=True, map=torch.empty_like(m)), m)


def test_ablate_features_out(K):
    x = rand(2, 3, 4, 4)
    ids = (torch.arange(16, dtype=I32, device=DEV) % 4).view(4, 4).contiguous()
    buffer_cases(lambda out: K.ablate_features(x, ids, 0, 4, 0.5, 3, 3, out=out), "out", (3, 3, 4, 4), "^out has the wrong size$")


def test_agi_heatmap_three_buffers(K):
    cd = rand(2, 3, 4, 4)
    buffer_cases(lambda out: K.agi_heatmap(cd, 2, out=out), "out", (2, 4, 4), "^agi_heatmap: out must hold 32 elements$")

    def with_step_grad(sg):
        sg = torch.empty((2, 3, 4, 4), device=DEV) if sg is None else sg
        K.agi_heatmap(cd, 2, step_grad=sg)
        return sg

    def with_qu(qu):
        qu = torch.empty((2, 2), device=DEV) if qu is None else qu
        K.agi_heatmap(cd, 2, qu=qu)
        return qu
    buffer_cases(with_step_grad, "step_grad", (2, 3, 4, 4), "^agi_heatmap: step_grad must hold 96 elements$")
    buffer_cases(with_qu, "qu", (2, 2), "^agi_heatmap: qu must hold 4 elements$")
    assert torch.equal(with_step_grad(None), cd)                     # one class per image: the sum of its pairs is the pair


def test_rownorm_out_keeps_its_shape_rule(K):
    x = rand(3, 10)
    want = K.rownorm(x)
    buf = torch.empty_like(x)
    assert K.rownorm(x, out=buf) is buf and torch.equal(buf, want)
    for bad in (torch.empty(10, 3, device=DEV), torch.empty(30, device=DEV), torch.empty(3, 9, device=DEV)):
        with pytest.raises(ValueError, match="^out must have the shape of x$"):        # the same element count is not enough
            K.rownorm(x, out=bad)
    with pytest.raises(TypeError, match="out"):
        K.rownorm(x, out=torch.empty(3, 10, dtype=F64, device=DEV))
    with pytest.raises(ValueError, match="out must be contiguous"):
        K.rownorm(x, out=strided((3, 10), F32))
    alias = x.clone()
    assert torch.equal(K.rownorm(alias, out=alias), want)


# ------------------------------------------------------------------------------ the BatchNorm wrappers
def bn_params(seed):
    w, b, mean = rand(3, seed=seed), rand(3, seed=seed + 1), rand(3, seed=seed + 2)
    return w, b, mean, rand(3, seed=seed + 3).abs() + 0.5


def test_bn_wrappers_refuse_mis_shaped_operands_and_a_short_mask(K):
    from xai_engine.prepare import BN_VARIANT as V
    x, gy = rand(2, 3, 2, 2), rand(2, 3, 2, 2, seed=9)
    w, b, mean, var = bn_params(20)
    need = K.bn_gate_mask_bytes(x.numel())
    assert need == 32
    y, mask = K.bn_relu_fwd_mask(x, None, w, b, mean, var, 1e-5, V)
    assert mask.dtype == U8 and mask.numel() == need
    given = torch.zeros(need, dtype=U8, device=DEV)
    y2, m2 = K.bn_relu_fwd_mask(x, None, w, b, mean, var, 1e-5, V, mask=given)
    assert m2 is given and torch.equal(m2, mask) and torch.equal(y2, y)
    short = torch.zeros(need - 1, dtype=U8, device=DEV)
    text = f"^mask has {need - 1} bytes, needs {need}$"
    with pytest.raises(ValueError, match=text):
        K.bn_relu_fwd_mask(x, None, w, b, mean, var, 1e-5, V, mask=short)
    with pytest.raises(ValueError, match=text):
        K.bn_relu_bwd_mask(gy, short, w, var, 1e-5, V)
    for bad in (rand(2, 3, 2, 1), rand(2, 3, 4), rand(3, 2, 2, 2)):                    # the last two have the element count of x
        with pytest.raises(ValueError, match="^identity must have the shape of x$"):
            K.bn_act_fwd(x, bad, w, b, mean, var, 1e-5, V)
        with pytest.raises(ValueError, match="^identity must have the shape of x$"):
            K.bn_relu_fwd_mask(x, bad, w, b, mean, var, 1e-5, V)
        with pytest.raises(ValueError, match="^gy2 must have the shape of gy$"):
            K.bn_relu_bwd(gy, y, w, var, 1e-5, V, gy2=bad)
        with pytest.raises(ValueError, match="^gy2 must have the shape of gy$"):
            K.bn_relu_bwd_mask(gy, mask, w, var, 1e-5, V, gy2=bad)
        with pytest.raises(ValueError, match="^gy2 must have the shape of gy$"):
            K.bn_relu_maxpool_bwd(gy, torch.zeros(2, 3, 2, 2, dtype=U8, device=DEV), w, var, 1e-5, V, 4, 4, 2, 2, 0, gy2=bad)
        with pytest.raises(ValueError, match="^code must have the shape of gy$"):
            K.bn_relu_maxpool_bwd(gy, torch.zeros(bad.shape, dtype=U8, device=DEV), w, var, 1e-5, V, 4, 4, 2, 2, 0)
    for i, name in enumerate(("weight", "bias", "mean", "var")):
        p = [w, b, mean, var]
        p[i] = p[i].double()
        for fn in (lambda: K.bn_act_fwd(x, None, *p, 1e-5, V), lambda: K.bn_relu_fwd_mask(x, None, *p, 1e-5, V),
                   lambda: K.bn_relu_maxpool_fwd(x, *p, 1e-5, V, 2, 2, 0), lambda: K.bn_relu_maxpool_fwd_code(x, *p, 1e-5, V, 2, 2, 0)):
            with pytest.raises(TypeError, match=f"^{name}: expected torch.float32"):
                fn()


def test_bn2_reaches_both_kernels_of_each_direction_alike(K):
    from xai_engine.prepare import BN_VARIANT as V
    x, idt, gy = rand(2, 3, 2, 2), rand(2, 3, 2, 2, seed=1), rand(2, 3, 2, 2, seed=2)
    w, b, mean, var = bn_params(30)
    w2, b2, m2, v2 = bn_params(40)
    y = K.bn_act_fwd(x, idt, w, b, mean, var, 1e-5, V, bn2=(w2, b2, m2, v2, 1e-3))
    ym, mask = K.bn_relu_fwd_mask(x, idt, w, b, mean, var, 1e-5, V, bn2=(w2, b2, m2, v2, 1e-3))
    assert torch.equal(y, ym) and not torch.equal(y, K.bn_act_fwd(x, idt, w, b, mean, var, 1e-5, V))
    gx, gid = K.bn_relu_bwd(gy, y, w, var, 1e-5, V, bn2=(w2, v2, 1e-3))                # bn2 alone asks for g_identity
    gxm, gidm = K.bn_relu_bwd_mask(gy, mask, w, var, 1e-5, V, bn2=(w2, v2, 1e-3))
    assert gid is not None and torch.equal(gx, gxm) and torch.equal(gid, gidm)
    plain = K.bn_relu_bwd(gy, y, w, var, 1e-5, V, want_identity=True)
    assert torch.equal(plain[0], gx) and not torch.equal(plain[1], gid)
    assert K.bn_relu_bwd(gy, y, w, var, 1e-5, V)[1] is None and K.bn_relu_bwd_mask(gy, mask, w, var, 1e-5, V)[1] is None
    for i, name in enumerate(("weight2", "bias2", "mean2", "var2")):
        p = [w2, b2, m2, v2]
        p[i] = p[i].double()
        with pytest.raises(TypeError, match=f"^{name}: "):
            K.bn_act_fwd(x, idt, w, b, mean, var, 1e-5, V, bn2=(*p, 1e-3))
        with pytest.raises(TypeError, match=f"^{name}: "):
            K.bn_relu_fwd_mask(x, idt, w, b, mean, var, 1e-5, V, bn2=(*p, 1e-3))
    for i, name in enumerate(("weight2", "var2")):
        p = [w2, v2]
        p[i] = p[i].double()
        with pytest.raises(TypeError, match=f"^{name}: "):
            K.bn_relu_bwd(gy, y, w, var, 1e-5, V, bn2=(*p, 1e-3))
        with pytest.raises(TypeError, match=f"^{name}: "):
            K.bn_relu_bwd_mask(gy, mask, w, var, 1e-5, V, bn2=(*p, 1e-3))


def test_pooled_extents_of_both_stem_forwards(K):
    from xai_engine.prepare import BN_VARIANT as V
    x = rand(1, 2, 5, 5)
    w, b, mean, var = (t[:2].contiguous() for t in bn_params(50))
    y = K.bn_relu_maxpool_fwd(x, w, b, mean, var, 1e-5, V, 3, 2, 1)
    assert tuple(y.shape) == (1, 2, 3, 3) and y.dtype == F32
    yc, code = K.bn_relu_maxpool_fwd_code(x, w, b, mean, var, 1e-5, V, 3, 2, 1)
    assert tuple(yc.shape) == tuple(code.shape) == (1, 2, 3, 3) and code.dtype == U8 and torch.equal(yc, y)


# ------------------------------------------------------------------------------ RISE: the two buffers that had no size check
def rise_inputs():
    grid = torch.tensor([[[1, 0], [0, 1]], [[1, 1], [0, 0]], [[0, 1], [1, 1]]], dtype=U8, device=DEV)
    shift = torch.tensor([[0, 1], [1, 0], [1, 1]], dtype=I32, device=DEV)
    return grid, shift, rand(3, 4, 4), (2, 2)


def test_rise_apply_out(K):
    grid, shift, image, cell = rise_inputs()
    buffer_cases(lambda out: K.rise_apply(grid, shift, cell, image, out=out), "out", (3, 3, 4, 4), "^out has the wrong size$")
    masked, masks = K.rise_apply(grid, shift, cell, image, want_masks=True, out=torch.empty(3, 3, 4, 4, device=DEV))
    assert torch.equal(masked, K.rise_apply(grid, shift, cell, image)) and tuple(masks.shape) == (3, 4, 4)
    only = K.rise_apply(grid, shift, cell, image, want_masked=False, want_masks=True)
    assert torch.equal(only, masks)


def test_rise_accum_acc(K):
    grid, shift, _, cell = rise_inputs()
    scores = torch.tensor([0.5, -1.0, 2.0], device=DEV)
    buffer_cases(lambda acc: K.rise_accum(grid, shift, scores, cell, 4, 4, 0.25, acc=acc), "acc", (4, 4), "^acc has the wrong size$",
                 dtype=F64, other=F32, fill=torch.zeros)
    carried = torch.ones((4, 4), dtype=F64, device=DEV)
    once = K.rise_accum(grid, shift, scores, cell, 4, 4, 0.25)
    assert torch.equal(K.rise_accum(grid, shift, scores, cell, 4, 4, 0.25, acc=carried), once + 1.0)


# ------------------------------------------------------------------------------ the checks the segmenters and clusterers share
def slic_operands():
    return torch.zeros(2, 4, 4, 3, device=DEV), torch.zeros(2, 2, 5, device=DEV), torch.zeros(2, 4, 4, dtype=I32, device=DEV)


def felz_operands():
    E = 4 * 3 + 3 * 4 + 2 * 3 * 3                              # the edges of a 4 x 4 image
    return (torch.zeros(2, E, dtype=torch.int64, device=DEV), torch.arange(E, dtype=I32, device=DEV).repeat(2, 1).contiguous(),
            torch.ones(1, dtype=F64, device=DEV))


def kmeans_operands():
    return (torch.zeros(8, 4, device=DEV), torch.zeros(2, 4, device=DEV), torch.zeros(8, dtype=I32, device=DEV),
            torch.zeros(2, dtype=I32, device=DEV), torch.zeros(6, dtype=I32, device=DEV))


def test_int_refuses_a_bool_in_three_families(K):
    f, cen, _ = slic_operands()
    with pytest.raises(TypeError, match="^step: expected an int, got bool$"):
        K.slic_assign(f, cen, True)
    keys, index, scales = felz_operands()
    with pytest.raises(TypeError, match="^min_size: expected an int, got bool$"):
        K.felz_merge(keys, index, scales, 4, 4, True)
    x, C, assign, counts, state = kmeans_operands()
    with pytest.raises(TypeError, match="^max_iter: expected an int, got bool$"):
        K.kmeans_update(x, C, assign, counts, K.kmeans_workspace(x, 2), state, True, 1e-4)
    with pytest.raises(TypeError, match="^n_clusters: expected an int, got bool$"):
        K.kmeans_workspace(x, True)
    with pytest.raises(ValueError, match="^step must be >= 1, got 0$"):
        K.slic_assign(f, cen, 0)
    with pytest.raises(ValueError, match="^max_iter must be >= 1, got 0$"):
        K.kmeans_update(x, C, assign, counts, K.kmeans_workspace(x, 2), state, 0, 1e-4)


def test_image_check_refuses_float16_and_a_missing_axis_in_three_families(K):
    f, cen, _ = slic_operands()
    with pytest.raises(TypeError, match="^features: expected torch.float32 or torch.float64, got torch.float16$"):
        K.slic_assign(f.half(), cen, 2)
    with pytest.raises(TypeError, match="^image: expected torch.float64, got torch.float16$"):
        K.felz_costs(f.half())
    with pytest.raises(TypeError, match="^features: expected torch.float64, got torch.float16$"):
        K.quickshift_density(f.half(), torch.zeros(2, 4, 4, dtype=F64, device=DEV), 1.0)
    with pytest.raises(ValueError, match=r"^features must be \(B, H, W, C\) with at least one element, got \(4, 4, 3\)$"):
        K.slic_assign(f[0], cen, 2)
    with pytest.raises(ValueError, match=r"^image must be \(B, H, W, C\) with at least one element, got \(4, 4, 3\)$"):
        K.felz_costs(f[0].double())
    with pytest.raises(ValueError, match=r"^features must be \(B, H, W, C\) with at least one element, got \(4, 4, 3\)$"):
        K.quickshift_density(f[0].double(), torch.zeros(2, 4, 4, dtype=F64, device=DEV), 1.0)
    with pytest.raises(TypeError, match="^points: expected torch.float32, got torch.float16$"):
        K.kmeans_workspace(torch.zeros(8, 4, dtype=torch.float16, device=DEV), 2)
    with pytest.raises(TypeError, match="^distance: expected torch.float32, got torch.float16$"):
        K.linkage_workspace(torch.zeros(4, 4, dtype=torch.float16, device=DEV))


def test_workspace_refuses_a_short_one_in_three_families(K):
    _, _, labels = slic_operands()
    need = K.slic_workspace(labels).numel()
    for call in (lambda ws: K.slic_components(labels, 1, 17, ws=ws), lambda ws: K.slic_number(labels, 0, ws=ws)):
        with pytest.raises(ValueError, match=r"^ws must be slic_workspace\(labels\) on the device of labels$"):
            call(torch.zeros(need - 1, dtype=U8, device=DEV))
        with pytest.raises(TypeError, match="^ws: expected torch.uint8"):
            call(torch.zeros(need, dtype=I32, device=DEV))
    keys, index, scales = felz_operands()
    need = K.felz_workspace(DEV, 2, 4, 4, 1).numel()
    for call in (lambda ws: K.felz_sort(keys, index, 4, 4, ws=ws), lambda ws: K.felz_merge(keys, index, scales, 4, 4, 1, ws=ws)):
        with pytest.raises(ValueError, match=r"^ws must be felz_workspace\(device, B, H, W, S\) on the device of the keys$"):
            call(torch.zeros(need - 1, dtype=U8, device=DEV))
    assert K.felz_sort(keys, index, 4, 4, ws=torch.zeros(need, dtype=U8, device=DEV))[0] is keys
    x, C, _, _, state = kmeans_operands()
    need = K.kmeans_workspace(x, 2).numel()
    first = torch.tensor([0, 1], device=DEV)
    with pytest.raises(ValueError, match=r"^ws must be kmeans_workspace\(points, k\) on the device of points$"):
        K.kmeans_init(x, first, C, torch.zeros(need - 1, dtype=U8, device=DEV), state)
    with pytest.raises(TypeError, match="^ws: expected a torch.Tensor, got NoneType$"):
        K.kmeans_init(x, first, C, None, state)


def test_status_refuses_a_wrong_length_in_two_families_and_is_cleared_when_new(K):
    f, cen, labels = slic_operands()
    for bad in (1, 3):
        with pytest.raises(ValueError, match="^status must hold 2 int32 on the device of its images$"):
            K.slic_assign(f, cen, 2, status=torch.zeros(bad, dtype=I32, device=DEV))
        with pytest.raises(ValueError, match="^status must hold 2 int32 on the device of its images$"):
            K.slic_components(labels, 1, 17, status=torch.zeros(bad, dtype=I32, device=DEV))
    keys, index, scales = felz_operands()
    for call in (lambda st: K.felz_costs(f.double(), status=st), lambda st: K.felz_merge(keys, index, scales, 4, 4, 1, status=st),
                 lambda st: K.felz_labels(labels, status=st)):
        with pytest.raises(ValueError, match="^status must hold one int32 on the device of its images$"):
            call(torch.zeros(2, dtype=I32, device=DEV))
        with pytest.raises(TypeError, match="^status: expected torch.int32"):
            call(torch.zeros(1, dtype=torch.int64, device=DEV))
    assert K.felz_costs(f.double())[2].tolist() == [0]                 # a new word is cleared by the library's own entry
    for clear in (K.slic_clear, K.felz_clear):
        given = torch.full((3,), 7, dtype=I32, device=DEV)
        assert clear(given) is given and given.tolist() == [0, 0, 0]
        with pytest.raises(ValueError, match="^status must hold at least one int32$"):
            clear(torch.zeros(0, dtype=I32, device=DEV))
        with pytest.raises(TypeError, match="^status: expected a torch.Tensor, got NoneType$"):
            clear(None)


def test_a_cpu_tensor_is_refused_alike_in_every_family(K):
    from xai_engine import XaiHipError
    f, cen, labels = slic_operands()
    keys, index, scales = felz_operands()
    x = kmeans_operands()[0]
    for call in (lambda: K.slic_assign(f.cpu(), cen, 2), lambda: K.slic_number(labels.cpu()), lambda: K.felz_costs(f.double().cpu()),
                 lambda: K.felz_labels(labels.cpu()), lambda: K.quickshift_density(f.double().cpu(), torch.zeros(2, 4, 4, dtype=F64), 1.0),
                 lambda: K.quickshift_labels(labels.cpu()), lambda: K.kmeans_workspace(x.cpu(), 2),
                 lambda: K.linkage_workspace(torch.zeros(4, 4)), lambda: K.slic_clear(torch.zeros(2, dtype=I32)),
                 lambda: K.slic_number(labels, 0, ws=torch.zeros(4096, dtype=U8)),
                 lambda: K.felz_sort(keys, index, 4, 4, ws=torch.zeros(4096, dtype=U8))):
        with pytest.raises(XaiHipError, match="lives on 'cpu'.*no CPU fallback"):
            call()
