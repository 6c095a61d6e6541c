"""The NumPy restatement of K75-K77 (tests/clip_restated.py: k75, k76, k77) against the expressions it restates, without a device.

The device tests compare the kernels with the restatement alone, so a misreading shared by both would pass.  Here the restatement is
held to the reference's expressions, written below with plain torch operations as xai_engine/eclip.py words them (attention_layer,
_ksim, grad_eclip behind its autograd step, mask_clip, the .sum(0) over the texts) and evaluated in fp64 on the same operand values,
at the shapes of tests/test_gpu_clip_edges.py with L * D <= 2^18 and at the value cases that make NORMALIZE clamp or divide by zero.

NaN positions: those of the same expressions evaluated in the operand dtype T on the CPU.

Finite values: a first-order forward-error bound, computed in fp64 from the operands by carrying (value, error bound) pairs through the
expressions (class `Q`), the way tests/helpers.py computes its excused footprint.  u_T = 2^-24 (float) or 2^-11 (half), eta_T half
the least subnormal spacing of T (2^-150, 2^-25), u = 2^-24 for the fp32 operations that are not rounded to T.
  a rounding to T:           dx + u_T |x| + eta_T
  a product, a quotient:     |a| db + |b| da;   da / |m| + |a| dm / m^2
  a rounded sum of n terms with r element-wise roundings per term (SUM, DOT, SUMSQ: a lane's chain of ceil(n / 64) additions, six
    butterfly steps, the roundings of the terms; in half the fp32 additions are charged at u_T, which also pays the sum's own rT):
                             sum_i dt_i + (ceil(n / 64) + 6 + r) u_T sum_i |t_i| + (r n + 1) eta_T
  a norm:                    rT(sqrt(s)): ds / (2 sqrt(s)), then a rounding;  the clamp max(n, 1e-12) is 1-Lipschitz (in half the
                             clamp is rT(1e-12) = 0, a norm is 0 or above 2^-25, and 0 / 0 is a NaN, compared by position)
  min and max:               1-Lipschitz in the largest error of the cosines, so w_i = (c_i - lo) / (hi - lo) carries the cosines' error
                             through 1 / (hi - lo)
  relu:                      1-Lipschitz;  the sum over T texts: T roundings, T u_T sum_t |m_t|
  K75 behind the scores:     the fp64 softmax is fed the restated (rounded) scores s, whose own error is bounded as a DOT above and
    is not the softmax's to answer for.  z = s - max is rounded in fp32 (|z| u absolute, so |z| u relative in exp z), exp is within
    one ulp (2u relative, 2^-149 absolute below 2^-126): de = (|z| + 2) u e + 2^-149;  BLOCKSUM: sum de + n u sum e, n = ceil(L / 1024) + 22;
    p = rT(e / sum): a quotient, u, a rounding;  att_out_d = rT(sum_j p_j v_jd), L fp32 additions: sum dp |v| + L u sum |p v|, a rounding.
The whole is multiplied by 2 for the second-order terms.  The same torch expressions evaluated in T must stay inside the bound at every
case too, so that a correct implementation with another summation order passes; both ratios go to profiles/r22_clip_edges.json."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import clip_restated as R
from conftest import ROOT

f64 = np.float64
U = 2.0 ** -24
DTYPES = (np.float32, np.float16)
SHAPES = [s for s in R.EDGE_SHAPES if s[0] * s[1] <= 1 << 18]
CASES = [(s, dt) for s in SHAPES for dt in DTYPES]
IDS = ["x".join(map(str, s)) + "-" + np.dtype(dt).name for s, dt in CASES]
PAIRS = [(True, True), (True, False), (False, True), (False, False)]
_LEDGER = []


@pytest.fixture(scope="module", autouse=True)
def _write_the_ledger():
    yield
    if _LEDGER:
        R.merge_ledger(os.path.join(ROOT, "profiles", "r22_clip_edges.json"), _LEDGER)


# ------------------------------------------------------------------------------------------------ the reference's expressions
def attention_layer(q, k, v, num_heads=1):
    L, N, D = q.shape
    hd = D // num_heads
    q, k, v = (t.contiguous().view(-1, N * num_heads, hd).transpose(0, 1) for t in (q * float(hd) ** -0.5, k, v))
    scores = torch.bmm(q, k.transpose(1, 2))
    w = F.softmax(scores, dim=-1)
    out = torch.bmm(w, v).transpose(0, 1).contiguous().view(L, N, D)
    return out, w.view(N, num_heads, L, -1).sum(dim=1) / num_heads, scores


def softmax_row(scores, v):
    """attention_layer from its softmax on, for given scores (N, 1, L) and v (L, N, D) -> (attn (N, L), att_out (N, D))"""
    w = F.softmax(scores, dim=-1)
    return w[:, 0], torch.bmm(w, v.transpose(0, 1))[:, 0]


def _ksim(first, k_out):
    return (F.normalize(first, dim=-1) * F.normalize(k_out[1:, 0, :], dim=-1)).sum(-1)


def grad_eclip(grad, q_out, k_out, v, withksim=True, withgrad=True):
    """grad_eclip behind its autograd step: `grad` is grad[:1, 0, :] of that step"""
    rows = v[1:, 0, :]
    if withgrad:
        rows = grad * rows
    if withksim:
        cos = _ksim(q_out[:1, 0, :], k_out)
        cos = (cos - cos.min()) / (cos.max() - cos.min())
        rows = rows * cos[:, None]
    return F.relu_(rows.sum(-1))


def mask_clip(txt_feats, v_final, k_out):
    cosine_v = (F.normalize(v_final, dim=-1) @ txt_feats)[0].transpose(1, 0)
    return cosine_v * _ksim(k_out[:1, 0, :], k_out)[None, :]


def tensors(h, dtype):
    return {n: torch.from_numpy(a).to(dtype) for n, a in h.items()}


def ref_k76(h, dtype, withksim, withgrad):
    """the stacked .sum(0) over the texts of grad_eclip, image by image -> (B, L - 1)"""
    t = tensors(h, dtype)
    B, T = t["grad"].shape[:2]
    return torch.stack([torch.stack([grad_eclip(t["grad"][b, x][None], t["q_out0"][None, b:b + 1], t["k_out"][:, b:b + 1], t["v"][:, b:b + 1],
                                                withksim, withgrad) for x in range(T)]).sum(0) for b in range(B)]).double().numpy()


def ref_k77(h, dtype):
    t = tensors(h, dtype)
    B = t["txt"].shape[0]
    return torch.stack([mask_clip(t["txt"][b].T, t["v_final"][b:b + 1], t["k_out"][:, b:b + 1]).sum(0) for b in range(B)]).double().numpy()


# ------------------------------------------------------------------------------------------------ the bound
class Q:
    """a quantity: its exact value x (fp64) and a first-order bound dx on the error of its rounded counterpart"""
    def __init__(self, x, dx=0.0):
        self.x = np.asarray(x, dtype=f64)
        self.dx = np.broadcast_to(np.asarray(dx, dtype=f64), self.x.shape)


class Rules:
    def __init__(self, dt):
        self.u, self.eta = (2.0 ** -11, 2.0 ** -25) if dt == np.float16 else (2.0 ** -24, 2.0 ** -150)

    def rnd(self, q):
        return Q(q.x, q.dx + self.u * np.abs(q.x) + self.eta)

    @staticmethod
    def mul(a, b):
        return Q(a.x * b.x, np.abs(a.x) * b.dx + np.abs(b.x) * a.dx)

    @staticmethod
    def div(a, m):
        with np.errstate(all="ignore"):
            return Q(a.x / m.x, a.dx / np.abs(m.x) + np.abs(a.x) * m.dx / m.x ** 2)

    def rsum(self, t, r):
        n = t.x.shape[-1]
        return Q(t.x.sum(-1), t.dx.sum(-1) + (-(-n // 64) + 6 + r) * self.u * np.abs(t.x).sum(-1) + (r * n + 1) * self.eta)

    def normalize(self, a):
        """NORMALIZE of exact rows a (..., n)"""
        a = Q(a)
        s = self.rsum(Q(a.x * a.x), 0)
        root = np.sqrt(s.x)
        norm = self.rnd(Q(root, s.dx / (2 * np.maximum(root, 2.0 ** -160))))
        m = Q(np.maximum(norm.x, 1e-12), np.maximum(norm.dx, self.u * 1e-12))
        return self.rnd(self.div(a, Q(m.x[..., None], m.dx[..., None])))

    def cosines(self, first, rows):
        """SUM(rT(first' * rows')) of exact first (B, D) and rows (L - 1, B, D) -> Q (B, L - 1)"""
        f, k = self.normalize(first), self.normalize(rows)
        c = self.rsum(self.mul(Q(f.x[None], f.dx[None]), k), 1)
        return Q(c.x.T, c.dx.T)

    def minmax(self, c):
        lo = Q(c.x.min(1, keepdims=True), c.dx.max(1, keepdims=True))
        hi = Q(c.x.max(1, keepdims=True), c.dx.max(1, keepdims=True))
        num, den = self.rnd(Q(c.x - lo.x, c.dx + lo.dx)), self.rnd(Q(hi.x - lo.x, hi.dx + lo.dx))
        return self.rnd(self.div(num, den))

    def over_texts(self, m):
        """rT(sum_t m_t) of m (T, ...): T roundings"""
        return Q(m.x.sum(0), m.dx.sum(0) + m.x.shape[0] * self.u * np.abs(m.x).sum(0) + self.eta)


def bound_k76(h, dt, withksim, withgrad):
    r = Rules(dt)
    g, v = h["grad"].astype(f64), np.transpose(h["v"][1:], (1, 0, 2)).astype(f64)             # (B, T, D), (B, L - 1, D)
    w = r.minmax(r.cosines(h["q_out0"].astype(f64), h["k_out"][1:].astype(f64))) if withksim else None
    per_text = []
    for t in range(g.shape[1]):
        terms = Q(g[:, t, None, :] * v if withgrad else v)
        if withksim:
            terms = r.mul(terms, Q(w.x[..., None], w.dx[..., None]))
        m = r.rsum(terms, int(withgrad) + int(withksim))
        per_text.append((np.maximum(m.x, 0), m.dx))
    out = r.over_texts(Q(np.stack([x for x, _ in per_text]), np.stack([dx for _, dx in per_text])))
    return out.x, 2 * out.dx


def bound_k77(h, dt):
    r = Rules(dt)
    c = r.cosines(h["k_out"][0].astype(f64), h["k_out"][1:].astype(f64))                      # (B, L - 1)
    f = r.normalize(h["v_final"].astype(f64))                                                 # (B, L - 1, E)
    txt = h["txt"].astype(f64)
    prods = [r.rnd(r.mul(r.rsum(r.mul(f, Q(txt[:, t, None, :])), 0), c)) for t in range(txt.shape[1])]
    out = r.over_texts(Q(np.stack([p.x for p in prods]), np.stack([p.dx for p in prods])))
    return out.x, 2 * out.dx


def bound_k75_scores(h, dt):
    r = Rules(dt)
    D = h["q0"].shape[1]
    qs = h["q0"].astype(f64) * float(D) ** -0.5
    qs = r.rnd(Q(qs, U * np.abs(qs)))                                                        # the scaling is rounded to float first
    s = r.rsum(r.mul(Q(qs.x[None], qs.dx[None]), Q(h["k"].astype(f64))), 0)                  # (L, B)
    return s.x.T, 2 * s.dx.T


def bound_k75_softmax(s, v, dt):
    """s (B, L): the restated scores;  v (L, B, D) -> (p, 2 dp, o, 2 do)"""
    r = Rules(dt)
    L = s.shape[1]
    z = s.astype(f64) - s.astype(f64).max(1, keepdims=True)
    e = Q(np.exp(z), (np.abs(z) + 2) * U * np.exp(z) + 2.0 ** -149)
    n = -(-L // 1024) + 22
    total = Q(e.x.sum(1, keepdims=True), e.dx.sum(1, keepdims=True) + n * U * e.x.sum(1, keepdims=True))
    p = r.div(e, total)
    p = r.rnd(Q(p.x, p.dx + U * np.abs(p.x)))
    absv = np.abs(v.astype(f64))
    o = np.einsum("bj,jbd->bd", p.x, v.astype(f64))
    do = np.einsum("bj,jbd->bd", p.dx, absv) + L * U * np.einsum("bj,jbd->bd", np.abs(p.x), absv)
    o = r.rnd(Q(o, do))
    return p.x, 2 * p.dx, o.x, 2 * o.dx


# ------------------------------------------------------------------------------------------------ the comparison
def hold(name, dt, restated, in_t, exact, bound):
    """NaN positions of the restatement are those of the expressions in T; its finite values and those of the expressions in T are
    within `bound` of the fp64 values `exact`"""
    restated, in_t = np.asarray(restated, f64), np.asarray(in_t, f64)
    assert restated.shape == in_t.shape == exact.shape == bound.shape, name
    assert np.array_equal(np.isnan(restated), np.isnan(in_t)), name
    ok = ~np.isnan(restated)
    assert not np.isnan(exact[ok]).any() and not np.isnan(bound[ok]).any() and (bound[ok] >= 0).all(), name
    for who, got in (("restated", restated), ("torch-in-T", in_t)):
        err = np.abs(got - exact)[ok]
        with np.errstate(all="ignore"):
            ratio = float(np.where(err == 0, 0.0, err / bound[ok]).max()) if ok.any() else 0.0
        _LEDGER.append({"name": f"cpu/{who}/{name}/{np.dtype(dt).name}", "measured": ratio, "bound": 1.0})
        assert ratio <= 1.0, (name, who, ratio)
    return ok


def tdt(dt):
    return torch.float16 if dt == np.float16 else torch.float32


def hold_k75(name, h, dt):
    _qs, s, p, o = R.k75(h["q0"], h["k"], h["v"], dt)
    t64, tT = tensors(h, torch.float64), tensors(h, tdt(dt))
    exact_s, ds = bound_k75_scores(h, dt)
    s_T = attention_layer(tT["q0"][None], tT["k"], tT["v"])[2][:, 0]
    s64 = attention_layer(t64["q0"][None], t64["k"], t64["v"])[2][:, 0].numpy()
    assert np.allclose(exact_s, s64, rtol=1e-9, atol=1e-300), name                          # the bound's own values are the expressions'
    hold(f"k75/scores/{name}", dt, s, s_T.double().numpy(), s64, ds)
    exact_p, dp, exact_o, do = bound_k75_softmax(s, h["v"], dt)
    p64, o64 = softmax_row(torch.from_numpy(s).double()[:, None], t64["v"])
    assert np.allclose(exact_p, p64.numpy(), rtol=1e-12, atol=0) and np.allclose(exact_o, o64.numpy(), rtol=1e-9, atol=1e-300)
    p_T, o_T = softmax_row(torch.from_numpy(s).to(tdt(dt))[:, None], tT["v"])
    hold(f"k75/attn/{name}", dt, p, p_T.double().numpy(), p64.numpy(), dp)
    hold(f"k75/att_out/{name}", dt, o, o_T.double().numpy(), o64.numpy(), do)


def hold_k76(name, h, dt, pairs=PAIRS):
    oks = {}
    for withksim, withgrad in pairs:
        got, _ = R.k76(h["q_out0"], h["k_out"], h["v"], h["grad"], h["grad"].shape[1], withksim, withgrad, dt)
        exact, bound = bound_k76(h, dt, withksim, withgrad)
        ref = ref_k76(h, torch.float64, withksim, withgrad)
        both = ~np.isnan(ref) & ~np.isnan(exact)
        assert np.allclose(exact[both], ref[both], rtol=1e-9, atol=1e-300), name           # the bound's own values are the expressions'
        oks[withksim, withgrad] = hold(f"k76/{name}/ksim{int(withksim)}grad{int(withgrad)}", dt, got, ref_k76(h, tdt(dt), withksim, withgrad),
                                       ref, bound)
    return oks


def hold_k77(name, h, dt):
    exact, bound = bound_k77(h, dt)
    ref = ref_k77(h, torch.float64)
    assert np.allclose(exact, ref, rtol=1e-9, atol=1e-300), name
    return hold(f"k77/{name}", dt, R.k77(h["v_final"], h["txt"], h["k_out"], dt), ref_k77(h, tdt(dt)), ref, bound)


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("shape,dt", CASES, ids=IDS)
def test_k75_restated_is_attention_layers_class_row(shape, dt):
    L, D, B = shape
    hold_k75("x".join(map(str, shape)), R.edge_operands(L, D, B, dt, names=("q0", "k", "v")), dt)


@pytest.mark.parametrize("shape,dt", CASES, ids=IDS)
def test_k76_restated_is_grad_eclip_summed_over_the_texts(shape, dt):
    """L = 2: one patch, 0 / 0 in the restatement and in torch alike whenever withksim is set"""
    L, D, B = shape
    oks = hold_k76("x".join(map(str, shape)), R.edge_operands(L, D, B, dt, names=("q_out0", "k_out", "v", "grad")), dt)
    for (withksim, _), ok in oks.items():
        assert ok.all() != (L == 2 and withksim) and ok.any() != (L == 2 and withksim)


@pytest.mark.parametrize("shape,dt", CASES, ids=IDS)
def test_k77_restated_is_mask_clip_summed_over_the_texts(shape, dt):
    L, D, B = shape
    assert hold_k77("x".join(map(str, shape)), R.edge_operands(L, D, B, dt, names=("k_out", "v_final", "txt")), dt).all()


@pytest.mark.parametrize("dt", DTYPES, ids=("float32", "float16"))
def test_restated_where_normalize_clamps_or_divides_by_zero(dt):
    """(6, 70, 4), the operands of the device test of the same name: a zero patch row of k_out (image 1), a zero q_out0 and a zero
    class row k_out[0] (image 2), patch rows and embedding rows of tiny norm (image 3), a zero row of v_final (image 0)"""
    half = dt == np.float16
    h = R.edge_operands(6, 70, 4, dt)
    h["k_out"][2, 1] = 0
    h["q_out0"][2] = 0
    h["k_out"][0, 2] = 0
    h["k_out"][1:, 3] = R.tiny_rows(h["k_out"][1:, 3], dt)
    h["v_final"][3] = R.tiny_rows(h["v_final"][3], dt)
    h["v_final"][0, 3] = 0
    oks = hold_k76("clamp", h, dt)
    for pair in PAIRS:
        nan = ~oks[pair]
        if pair[0]:
            assert not nan[0].any() and nan[1].all() == half and nan[1].any() == half and nan[2].all() and not nan[3].any()
        else:
            assert not nan.any()
    nan = ~hold_k77("clamp", h, dt)
    assert np.array_equal(nan[0], (np.arange(5) == 3) & half) and np.array_equal(nan[1], (np.arange(5) == 1) & half)
    assert nan[2].all() == half and nan[2].any() == half and not nan[3].any()


def test_k75_restated_with_exp_results_down_to_the_subnormal_range_and_zero():
    """fp32, (70, 8, 1), scores 0, -2, ..., -138: the operands of the device test of the same name"""
    h = R.edge_operands(70, 8, 1, np.float32, names=("q0", "k", "v"))
    h["q0"][:] = np.sqrt(np.float32(8))
    h["k"][:] = 0
    h["k"][:, 0, 0] = -2 * np.arange(70, dtype=np.float32)
    hold_k75("exp-range", h, np.float32)
    p = R.k75(h["q0"], h["k"], h["v"], np.float32)[2][0]
    assert ((p > 0) & (p < 2.0 ** -126)).sum() >= 6 and (p == 0).sum() >= 15
