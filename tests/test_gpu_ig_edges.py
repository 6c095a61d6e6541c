"""The IG family of csrc/ig_kernels.hip (the two stream mappings of K2 and ig_accum_kernel<4 | 1>, ig_accum_add / ig_finish,
store_grads, the Left-IG cutoff, sumsq and idgi_accum) on the MI355X against tests/ig_restated.py at their edges.

Every float result is held bit for bit to the fp32 restatement -- s ascending per (pixel, channel), a true division, the
butterflies of sumsq -- then inside the derived bound around the fp64 definition (the fraction goes to the ledger at 1.0) and
inside the project's 1e-5; integer data comes back element for element as int64; copies and cutoffs are compared as int32.
Calls go through K._call with raw pointers, so that any one operand can sit one word past a 16-byte boundary; every output
lives between guard words that must come back untouched and every input is read back after the call.  Which instantiation ran
is read from a profiler trace and compared with the host's choice restated in ig_restated.accum_kernel_for on the device's own
CU count.  K1 (ig_interp_kernel) keeps its bit-exact tests in tests/test_gpu_kernels.py; here it gets the HBM-sized plan with an odd
step count and its operands misaligned in turn."""
import numpy as np
import pytest
import torch

import ig_restated as R
from conftest import BAR, check
from test_cpu_ig import cell_case, held_to_fp64, inside
from test_gpu_blur_edges import kernels_of
from test_gpu_masker_edges import POISON, In, Out, same_bits

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
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def call(K, name, *args):
    """-> the names of the kernels the entry launched"""
    return kernels_of(lambda: K._call(name, torch.device(DEV), *args))[1]


def one_of(names, kernel, args):
    """exactly one instantiation of `kernel` ran, and it is <args>"""
    mine = [n for n in names if kernel + "<" in n or kernel + "I" in n]
    return len(mine) == 1 and any(s in mine[0] for s in R.spellings(kernel, args))


def floats(out, shape):
    return out.get().view(F32).reshape(shape).copy()


# ---- K1: an odd step count on the HBM-sized plan, and misaligned operands --------------------------------------------------------------

def interp_on_device(x, b, al):
    """base + alpha * (x - base) with torch's two roundings, as test_ig_interp_full_size_hbm_branch_bit_exact states it"""
    base = b if isinstance(b, torch.Tensor) else torch.full_like(x, b)
    return base[None] + al.view(-1, 1, 1, 1) * (x - base)[None]


def test_interp_hbm_plan_with_an_odd_step_count(K):
    """24 images x 19 alphas x 3x224x224 is 262 MiB written: past the 256 MiB threshold, two step rows per lane, so the last of
    the ten chunks holds one row.  Bit for bit on the device, shared and per-image alphas; then the same output one word past a
    16-byte boundary, which is the scalar non-temporal form, between guard words."""
    n_img, n_alpha, shape = 24, 19, (3, 224, 224)
    assert n_img * n_alpha * 3 * 224 * 224 * 4 >= 256 << 20 and n_alpha % 2 == 1
    gen = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn((n_img,) + shape, device=DEV, generator=gen)
    b = torch.randn((n_img,) + shape, device=DEV, generator=gen) * 0.3
    al = torch.rand((n_img, n_alpha), device=DEV, generator=gen)
    got, names = kernels_of(lambda: K.ig_interp(x, b, al[3]))
    assert one_of(names, "ig_interp_kernel", (4, True)), names
    for i in (0, 11, 23):
        assert torch.equal(got[i], interp_on_device(x[i], b[i], al[3]))
    got = K.ig_interp(x, 0.25, al)
    for i in (0, 7, 23):
        assert torch.equal(got[i], interp_on_device(x[i], 0.25, al[i]))
    del got
    n = n_img * n_alpha * x[0].numel()
    buf = torch.full((4 + 1 + n + 4,), POISON, dtype=torch.int32, device=DEV)
    out = buf[5:5 + n].view(torch.float32).view((n_img, n_alpha) + shape)
    assert out.data_ptr() % 16 == 4
    _, names = kernels_of(lambda: K.ig_interp(x, b, al, out=out))
    assert one_of(names, "ig_interp_kernel", (1, True)), names
    for i in (0, 12, 23):
        assert torch.equal(out[i], interp_on_device(x[i], b[i], al[i]))
    assert (buf[:5] == POISON).all() and (buf[5 + n:] == POISON).all()


@pytest.mark.parametrize("n_elem", [1024, 4 * 257, 1023])
def test_interp_with_each_operand_misaligned_in_turn(K, n_elem):
    """a cache-sized call through raw pointers: x, the baseline and the output in turn one word past a 16-byte boundary take the
    scalar form (as an odd row length does) and return the bits of the aligned call, which are oracle.ig.interpolate's"""
    from oracle import ig as oig
    n_img, n_alpha = 2, 5
    rng = np.random.default_rng([42, n_elem])
    x, b = rng.standard_normal((n_img, n_elem), dtype=F32), rng.standard_normal((n_img, n_elem), dtype=F32)
    al = rng.random((n_img, n_alpha), dtype=F32)
    want = np.stack([oig.interpolate(x[i].reshape(1, 1, -1), b[i].reshape(1, 1, -1), al[i]) for i in range(n_img)])
    for off in (None, "x", "base", "out"):
        xi, bi, ai, out = In(x, int(off == "x")), In(b, int(off == "base")), In(al), Out(n_img * n_alpha * n_elem, int(off == "out"))
        names = call(K, "xai_ig_interp_f32", xi.ptr, bi.ptr, 0.0, ai.ptr, n_alpha, n_img, n_alpha, n_elem, out.ptr)
        assert one_of(names, "ig_interp_kernel", (4 if off is None and n_elem % 4 == 0 else 1, False)), (off, names)
        same_bits(out.get(), want, (n_elem, off))
        xi.unchanged(), bi.unchanged(), ai.unchanged()


# ---- accumulate --------------------------------------------------------------------------------------------------------------------

def run_accum(K, grads, n_use, x, base, w1=None, w2=None, off=None):
    """xai_ig_accum_f32 with out_abs -> (out (n_img, C, hw), abs (n_img, hw)), kernel names.  n_use: an int32 array (on the device),
    an int or None (host); `off` names the operand that sits one word past a 16-byte boundary."""
    n_img, n_steps, C, hw = grads.shape
    o = lambda op: int(off == op)
    g, xi = In(grads, o("grads")), In(x, o("x"))
    b = None if np.isscalar(base) else In(base, o("base"))
    nu = In(np.asarray(n_use, np.int32)) if isinstance(n_use, np.ndarray) else None
    n_host = n_steps if n_use is None or nu is not None else int(n_use)
    wa, wb = (None if w is None else In(w) for w in (w1, w2))
    out, out_abs = Out(n_img * C * hw, o("out")), Out(n_img * hw, o("out_abs"))
    ptr = lambda t: None if t is None else t.ptr
    names = call(K, "xai_ig_accum_f32", g.ptr, n_img, n_steps, ptr(nu), n_host, ptr(wa), ptr(wb), xi.ptr, ptr(b),
                 0.0 if b is not None else float(base), C, hw, out.ptr, out_abs.ptr)
    got = floats(out, (n_img, C, hw)), floats(out_abs, (n_img, hw))
    for t in (g, xi, b, nu, wa, wb):
        if t is not None:
            t.unchanged()
    return got, names


def held_to_the_restatement(name, got, case):
    """bits of accum_fp32; inside accum_bound around accum64 (the fractions go to the ledger at 1.0); the project's norm at 1e-5"""
    want = R.accum_fp32(**case)
    same_bits(got[0], want[0], (name, "out"))
    same_bits(got[1], want[1], (name, "abs"))
    r_out, r_abs, o64, a64 = held_to_fp64(got, case)
    print(f"{name}: out {r_out:.4f}, abs {r_abs:.4f} of the derived bound")
    for part, ratio, mine, want64 in (("out", r_out, got[0], o64), ("abs", r_abs, got[1], a64)):
        check(f"{name}/{part}/bound", ratio, 0, 1.0, against=AGAINST, absolute=True)
        check(f"{name}/{part}", mine, want64, BAR, against=AGAINST)


@pytest.mark.parametrize("cell", R.accum_cells(), ids=R.accum_name)
def test_accumulate_cell_has_the_bits_of_the_restatement(K, cus, cell):
    case = cell_case(cell, cus)
    launch = R.cell_launch(cell, cus)
    got, names = run_accum(K, off=cell.off, **case)
    assert R.ran(names, launch), (names, launch)
    held_to_the_restatement(f"ig_edges/accum/{cell.name}", got, case)


def test_either_side_of_the_threshold_gives_the_same_bits(K, cus):
    """n_img = cus * 8 + 1 at hw = 512 runs the big mapping, the first cus * 8 - 1 of the same images the small one: the images
    both hold come back with the same bits."""
    cells = {c.name: c for c in R.accum_cells()}
    over, under = cells["big_C3_over"], cells["big_C3_under"]
    case = cell_case(over, cus)
    n = R.n_img_of(under, cus)
    fewer = {k: (v[:n] if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    big, names = run_accum(K, **case)
    assert R.ran(names, R.cell_launch(over, cus)) and R.cell_launch(over, cus).args[:3] == (256, 4, 1), names
    small, names = run_accum(K, **fewer)
    assert R.ran(names, R.cell_launch(under, cus)) and R.cell_launch(under, cus).args[:3] == (64, 1, 5), names
    same_bits(small[0], big[0][:n], "out")
    same_bits(small[1], big[1][:n], "abs")


@pytest.mark.parametrize("name", R.PER_KERNEL)
def test_n_use_outside_its_range_is_clamped(K, cus, name):
    """n_use_dev of 0, -3 and n_steps + 5 is n_use of 1, 1 and n_steps"""
    cell = next(c for c in R.accum_cells() if c.name == name)
    case = cell_case(cell, cus)
    n_img = case["grads"].shape[0]
    wild = np.asarray([(0, -3, cell.n_steps + 5)[i % 3] for i in range(n_img)], np.int32)
    tame = np.asarray([(1, 1, cell.n_steps)[i % 3] for i in range(n_img)], np.int32)
    got, names = run_accum(K, **dict(case, n_use=wild))
    assert R.ran(names, R.cell_launch(cell, cus)), names
    want, _ = run_accum(K, **dict(case, n_use=tame))
    restated = R.accum_fp32(**dict(case, n_use=tame))
    for i in (0, 1):
        same_bits(got[i], want[i], (name, i))
        same_bits(got[i], restated[i], (name, i, "restated"))


@pytest.mark.parametrize("name", R.PER_KERNEL)
def test_integer_data_comes_back_exactly(K, cus, name):
    """... and a step row read past n_use, which holds 2^20 + 1, would show at every pixel"""
    cell = next(c for c in R.accum_cells() if c.name == name)
    n_img = R.n_img_of(cell, cus)
    n_use = R.cell_n_use(cell, n_img)
    grads, x, base, out, out_abs = R.exact_accum_case(n_img, cell.n_steps, cell.C, cell.hw, n_use)
    got, names = run_accum(K, grads, n_use, x, base)
    assert R.ran(names, R.cell_launch(cell, cus)), names
    assert (got[0] == np.rint(got[0])).all(), "integer data came back with a fraction"
    np.testing.assert_array_equal(got[0].astype(np.int64), out)
    np.testing.assert_array_equal(got[1].astype(np.int64), out_abs)


# ---- accum_add / finish ------------------------------------------------------------------------------------------------------------

def run_add(K, grads, acc, goff=0, aoff=0):
    """xai_ig_accum_add_f32 in place on a pre-filled acc between guard words -> acc, kernel names"""
    n_batch, n = grads.shape
    g, a = In(grads, goff), Out(n, aoff, fill=acc)
    names = call(K, "xai_ig_accum_add_f32", g.ptr, n_batch, a.ptr, n)
    got = floats(a, (n,))
    g.unchanged()
    return got, names


def run_finish(K, acc, n_steps, x, base, want_abs=True, off=None):
    n_img, C, hw = acc.shape
    o = lambda op: int(off == op)
    a, xi = In(acc, o("acc")), In(x, o("x"))
    b = None if np.isscalar(base) else In(base, o("base"))
    out, out_abs = Out(n_img * C * hw, o("out")), Out(n_img * hw, o("out_abs"))
    names = call(K, "xai_ig_finish_f32", a.ptr, n_img, n_steps, xi.ptr, None if b is None else b.ptr, 0.0 if b is not None else float(base),
                 C, hw, out.ptr, out_abs.ptr if want_abs else None)
    got = floats(out, (n_img, C, hw)), (floats(out_abs, (n_img, hw)) if want_abs else None)
    assert want_abs or out_abs.untouched()
    for t in (a, xi, b):
        if t is not None:
            t.unchanged()
    return got, names


@pytest.mark.parametrize("cell", R.ADD_CELLS, ids=R.add_name)
def test_accum_add_cell_has_the_bits_of_the_restatement(K, cell):
    n_batch, n, goff, aoff = cell
    rng = np.random.default_rng([41, n_batch, n, goff, aoff])
    grads, acc = rng.standard_normal((n_batch, n), dtype=F32), rng.standard_normal(n, dtype=F32)
    got, names = run_add(K, grads, acc, goff, aoff)
    assert one_of(names, "ig_accum_add_kernel", (4 if n % 4 == 0 and not goff and not aoff else 1,)), names
    same_bits(got, R.accum_add_fp32(grads, acc), cell)
    ints = rng.integers(-8, 9, (n_batch, n))
    got, _ = run_add(K, ints.astype(F32), np.full(n, 3, F32), goff, aoff)
    np.testing.assert_array_equal(got.astype(np.int64), 3 + ints.sum(axis=0))


@pytest.mark.parametrize("cell", R.FINISH_CELLS, ids=R.finish_name)
def test_finish_cell_has_the_bits_of_the_restatement(K, cell):
    """with and without out_abs, a scalar and a tensor baseline, and each operand in turn one word off (the scalar form)"""
    n_img, C, hw = cell
    d = R.normal_accum_case(n_img, 9, C, hw, seed=1)
    acc = d["grads"][:, 0]
    for base in (d["base"], R.SCALAR_BASE):
        want = R.finish_fp32(acc, 9, d["x"], base)
        for want_abs in (True, False):
            got, names = run_finish(K, acc, 9, d["x"], base, want_abs)
            assert one_of(names, "ig_finish_kernel", (4 if hw % 4 == 0 else 1,)), names
            same_bits(got[0], want[0], (cell, want_abs))
            if want_abs:
                same_bits(got[1], want[1], (cell, "abs"))
    if hw % 4 == 0:
        want = R.finish_fp32(acc, 9, d["x"], d["base"])
        for off in ("acc", "x", "base", "out", "out_abs"):
            got, names = run_finish(K, acc, 9, d["x"], d["base"], True, off)
            assert one_of(names, "ig_finish_kernel", (1,)), (off, names)
            same_bits(got[0], want[0], (cell, off))
            same_bits(got[1], want[1], (cell, off, "abs"))


@pytest.mark.parametrize("cell", R.CHAINED_CELLS, ids=R.chained_name)
def test_finish_of_accum_add_has_the_bits_of_the_accumulate_kernels(K, cell):
    """the streaming form, batches of step gradients added into a zeroed accumulator and finished, against accum_fp32 on the
    same data and against xai_ig_accum_f32 itself"""
    n_img, C, hw, batches = cell
    n_steps = sum(batches)
    d = R.normal_accum_case(n_img, n_steps, C, hw, seed=2)
    acc = np.zeros(n_img * C * hw, F32)
    s = 0
    for nb in batches:
        rows = np.ascontiguousarray(d["grads"][:, s:s + nb].transpose(1, 0, 2, 3)).reshape(nb, -1)      # [step][image]
        acc, _ = run_add(K, rows, acc)
        s += nb
    got, _ = run_finish(K, acc.reshape(n_img, C, hw), n_steps, d["x"], d["base"])
    case = {"grads": d["grads"], "n_use": None, "x": d["x"], "base": d["base"]}
    held_to_the_restatement(f"ig_edges/stream/{R.chained_name(cell)}", got, case)
    whole, _ = run_accum(K, **case)
    same_bits(got[0], whole[0], (cell, "K2"))
    same_bits(got[1], whole[1], (cell, "K2 abs"))


# ---- store_grads -------------------------------------------------------------------------------------------------------------------

def test_store_grads_returns_the_bits(K, cus):
    """random words with NaN payloads, -0.0 and subnormals; both forms, and the second trip of each one's grid-stride loop"""
    for n, soff, doff in R.store_cells(cus):
        words = R.store_payload(n)
        src, dst = In(words, soff), Out(n, doff)
        names = call(K, "xai_ig_store_grads_f32", src.ptr, dst.ptr, n)
        mine = [k for k in names if "store_stream" in k]
        assert len(mine) == 1 and R.store_kernel_for(n, not soff, not doff) in mine[0], (n, soff, doff, names)
        np.testing.assert_array_equal(dst.get(), words, err_msg=str((n, soff, doff)))
        src.unchanged()


# ---- cutoff ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("alpha", R.CUTOFF_ALPHAS + (R.NO_HIT_ALPHA,))
def test_cutoff_is_the_reference_on_every_planted_row(K, alpha):
    """one launch per n_steps over all planted rows; the int32 results are R.cutoff's -- a NaN anywhere gives 1, as torch.max makes
    it in the reference -- and the rows behind the launch's last image stay untouched"""
    for n in R.CUTOFF_STEPS:
        labels, rows = R.cutoff_rows(n, alpha)
        lg, out = In(rows), Out(len(rows) + 3)
        K._call("xai_ig_cutoff_f32", torch.device(DEV), lg.ptr, len(rows), n, float(alpha), out.ptr)
        got = out.get()
        want = [R.cutoff(row, alpha) for row in rows]
        assert got[:len(rows)].tolist() == want, [(n, k, g, w) for k, g, w in zip(labels, got.tolist(), want) if g != w]
        assert (got[len(rows):] == POISON).all()
        lg.unchanged()


# ---- sumsq -------------------------------------------------------------------------------------------------------------------------

def run_sumsq(K, rows, off=0):
    r, out = In(rows, off), Out(rows.shape[0])
    K._call("xai_sumsq_f32", torch.device(DEV), r.ptr, rows.shape[0], rows.shape[1], out.ptr)
    got = floats(out, (rows.shape[0],))
    r.unchanged()
    return got


@pytest.mark.parametrize("cell", R.SUMSQ_CELLS, ids=R.sumsq_name)
def test_sumsq_cell_has_the_bits_of_the_restatement(K, cell):
    n_rows, n, off = cell
    name = f"ig_edges/sumsq/{R.sumsq_name(cell)}"
    rows = R.sumsq_case(cell)
    got = run_sumsq(K, rows, off)
    same_bits(got, R.sumsq_fp32(rows, aligned=not off), name)
    ratio = inside(got, R.sumsq64(rows), R.sumsq_bound(rows, aligned=not off))
    print(f"{name}: {ratio:.4f} of the derived bound")
    check(name + "/bound", ratio, 0, 1.0, against=AGAINST, absolute=True)
    check(name, got, R.sumsq64(rows), BAR, against=AGAINST)
    if off:                                                  # the scalar form: other bits than the same rows on a boundary
        assert (got.view(np.int32) != run_sumsq(K, rows, 0).view(np.int32)).any()
    ints = R.sumsq_case(cell, integer=True)
    np.testing.assert_array_equal(run_sumsq(K, ints, off).astype(np.int64), (ints.astype(np.int64) ** 2).sum(axis=1))


# ---- IDGI --------------------------------------------------------------------------------------------------------------------------

def run_idgi(K, g, lg, sq, off=0):
    gi, li, si, out = In(g), In(lg), In(sq), Out(g.shape[1], off)
    names = call(K, "xai_idgi_accum_f32", gi.ptr, g.shape[0], li.ptr, si.ptr, g.shape[1], out.ptr)
    assert one_of(names, "idgi_accum_kernel", (4 if g.shape[1] % 4 == 0 and not off else 1,)), names
    got = floats(out, (g.shape[1],))
    gi.unchanged(), li.unchanged(), si.unchanged()
    return got


def idgi_held(name, got, g, lg, sq):
    same_bits(got, R.idgi_fp32(g, lg, sq), name)
    want = R.idgi64(g, lg, sq)[0]
    ratio = inside(got, want, R.idgi_bound(g, lg, sq))
    print(f"{name}: {ratio:.4f} of the derived bound")
    check(name + "/bound", ratio, 0, 1.0, against=AGAINST, absolute=True)
    check(name, got, want, BAR, against=AGAINST)


@pytest.mark.parametrize("cell", R.IDGI_CELLS, ids=R.idgi_name)
def test_idgi_cell_has_the_bits_of_the_restatement(K, cell):
    """sumsq comes from the restatement, so that the two kernels are held separately"""
    g, lg = R.idgi_case(cell)
    sq = R.sumsq_fp32(g)
    idgi_held(f"ig_edges/idgi/{R.idgi_name(cell)}", run_idgi(K, g, lg, sq, cell[2]), g, lg, sq)


def test_idgi_with_a_zero_gradient_step_is_nan_where_the_reference_is(K):
    g, lg = R.idgi_case(R.IDGI_ZERO_STEP, zero_step=2)
    sq = R.sumsq_fp32(g)
    got = run_idgi(K, g, lg, sq)
    same_bits(got, R.idgi_fp32(g, lg, sq), "zero step")
    assert np.isnan(got).all()
    same_bits(run_sumsq(K, g), sq, "sumsq with a zero row")


def test_sumsq_feeds_idgi(K):
    g, lg = R.idgi_case(R.IDGI_CHAINED)
    gd = torch.from_numpy(g).to(DEV)
    sq = K.sumsq(gd)
    got = K.idgi_accum(gd, torch.from_numpy(lg).to(DEV), sq).cpu().numpy()
    same_bits(sq.cpu().numpy(), R.sumsq_fp32(g), "sumsq")
    idgi_held("ig_edges/idgi_chained/" + R.idgi_name(R.IDGI_CHAINED), got, g, lg, R.sumsq_fp32(g))
