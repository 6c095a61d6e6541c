#!/usr/bin/env python3
"""One SHA-256 per output of every xai_engine.kernels entry outside the classifier fusion (bn_*, maxpool_*, guided_map), on
small seeded inputs: run it on two builds of libxai_hip.so (and libxai_ext.so) and compare the lists line by line.
    python profiles/experiments/exp_same_bytes.py [--lib other/libxai_hip.so] [--ext-lib other/libxai_ext.so] > hashes.txt
A tolerance would let a changed summation order through; equal bytes do not.  The inputs take both flavours of every entry
(element counts that are and are not multiples of 4, views offset by one float) and give the shared reductions, the radix
select and the argmax their edge cases: more elements than lanes and fewer, ties, +-0, +-inf, NaN first and last, rows of -inf.
Shapes stay at or under 2 images of 32 x 32; the whole run takes seconds."""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "image-classification-xai_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from xai_engine import _lib  # noqa: E402
from xai_engine import kernels as K  # noqa: E402
from xai_engine.rise import draw_masks  # noqa: E402

DEV = "cuda:0"
INF, NAN = float("inf"), float("nan")
SHAPES = ((3, 8, 8), (3, 7, 9), (3, 32, 32), (3, 31, 27))       # 192, 189, 3072 and 2511 floats
GEN = torch.Generator().manual_seed(20)


def emit(name, *outs):
    torch.cuda.synchronize()
    for i, t in enumerate(outs):
        if t is None:
            continue
        a = np.ascontiguousarray(t.detach().cpu().numpy())
        print(f"{name}[{i}] {a.dtype}{list(a.shape)} {hashlib.sha256(a.tobytes()).hexdigest()}")


def randn(*shape):
    return torch.randn(*shape, generator=GEN)


def dev(t, shift=False):
    """The tensor on the device; shift: as a contiguous view that starts one float (4 bytes) into its buffer"""
    t = t.to(DEV).contiguous()
    if not shift:
        return t
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    return v


def variants():
    for shape in SHAPES:
        yield "x".join(map(str, shape)), shape, False
    yield "x".join(map(str, SHAPES[0])) + "+4B", SHAPES[0], True


def spiced(*shape):
    """Normal values with ties, +-0 and +-inf among them"""
    t = randn(*shape)
    f = t.view(-1)
    n = f.numel()
    f[1::7] = f[0]
    f[2::11] = 0.0
    f[3::13] = -0.0
    f[n // 2] = INF
    f[n // 3] = -INF
    return t


def edge_logits(k):
    """Rows: random, NaN first, NaN last, ties at the maximum, all -inf, +0 and -0 tied"""
    z = randn(6, k)
    z[1, 0] = NAN
    z[2, k - 1] = NAN
    z[3, :] = z[3, :].round()
    z[3, k // 2:] = z[3].max()
    z[4, :] = -INF
    z[5, :] = -1.0
    z[5, k // 2] = -0.0
    z[5, k - 1] = 0.0
    return z


def ig_entries():
    for tag, shape, sh in variants():
        x, b = dev(randn(2, *shape), sh), dev(randn(2, *shape), sh)
        al = dev(torch.linspace(0, 1, 5))
        emit(f"ig_interp {tag}", K.ig_interp(x, b, al), K.ig_interp(x, 0.25, dev(torch.rand(2, 5, generator=GEN))))
        g = dev(randn(2, 11, *shape), sh)
        w1, w2 = dev(randn(2, 11)), dev(randn(2, 11))
        n_use = dev(torch.tensor([3, 11], dtype=torch.int32))
        emit(f"ig_accum {tag}", *K.ig_accum(g, x, b, want_abs=True), K.ig_accum(g, x, 0.5, n_use=n_use), K.ig_accum(g, x, b, n_use=7),
             *K.ig_accum(g, x, b, w1=w1, w2=w2, want_abs=True), K.ig_accum(g, x, b, w1=w1))
        g1 = dev(randn(2, 11, 1, shape[1], shape[2]), sh)
        emit(f"ig_accum C=1 {tag}", *K.ig_accum(g1, x[:, :1].contiguous(), 0.0, n_use=n_use, want_abs=True))
        emit(f"store_grads {tag}", K.store_grads(g, dev(torch.zeros(g.shape), sh)))
        emit(f"ig_accum_add {tag}", K.ig_accum_add(g[0], dev(randn(*shape), sh)))
        emit(f"ig_finish {tag}", *K.ig_finish(g[:, 0].contiguous(), 11, x, b, want_abs=True), K.ig_finish(g[:, 1].contiguous(), 11, x, 0.5))
        sq = K.sumsq(g[0])
        emit(f"sumsq {tag}", sq, K.sumsq(dev(spiced(4, *shape), sh)))
        emit(f"idgi_accum {tag}", K.idgi_accum(g[0], dev(randn(11)), sq))
    for n in (1, 10, 65, 1000):
        lg = edge_logits(n)
        lg[0] = lg[0].abs() + 0.1
        emit(f"ig_cutoff n={n}", K.ig_cutoff(dev(lg), 0.9), K.ig_cutoff(dev(lg), 1.0), K.ig_cutoff(dev(-lg.abs()), 0.5))


def cam_rise_blur_entries():
    for B, C, h, w in ((2, 5, 7, 7), (1, 64, 4, 6)):
        act, grad = dev(randn(B, C, h, w)), dev(randn(B, C, h, w))
        cam = K.gradcam(act, grad)
        emit(f"gradcam {B}x{C}x{h}x{w}", cam, K.gradcam(act, grad, relu=False), K.bilinear_up(cam, 32, 32), K.bilinear_up(cam, 27, 31, scale=0.5, take_abs=True))
    for (H, W), s in (((32, 32), 8), ((27, 31), 8), ((32, 32), 4), ((31, 27), 7)):
        grid, shifts, cell = draw_masks((H, W), 6, s, 0.5, rng=np.random.RandomState(3))
        g8, shf = dev(torch.from_numpy(grid)), dev(torch.from_numpy(shifts))
        for sh in (False, True):
            image = dev(randn(3, H, W), sh)
            emit(f"rise_apply {H}x{W} s={s} shift={sh}", *K.rise_apply(g8, shf, cell, image, want_masked=True, want_masks=True))
        emit(f"rise_apply C=2 {H}x{W} s={s}", K.rise_apply(g8, shf, cell, dev(randn(2, H, W))))
        emit(f"rise_accum {H}x{W} s={s}", K.rise_accum(g8, shf, dev(torch.rand(6, generator=GEN)), cell, H, W, 1.0 / 3.0))
    for shape in ((2, 3, 32, 32), (1, 3, 27, 31)):
        x = dev(randn(*shape))
        for klen in (1, 11, 31, 67):
            k = torch.rand(klen, generator=GEN)
            emit(f"blur_sep {list(shape)} klen={klen}", K.blur_sep(x, dev(k / k.sum())))


def insdel_entries():
    for n_seg, hw in ((2, 1024), (2, 189), (1, 64), (3, 2511)):
        for name, sal in (("spiced", spiced(n_seg, hw)), ("non-negative", randn(n_seg, hw).abs()), ("constant", torch.full((n_seg, hw), 2.0))):
            if name == "spiced":
                sal[0, hw // 5] = NAN
            order, rk = K.rank(dev(sal))
            emit(f"rank {n_seg}x{hw} {name}", order, rk)
    for shape in SHAPES:
        C, H, W = shape
        hw = H * W
        sal = randn(hw).abs()
        order, rk = K.rank(dev(sal[None]))
        for desc in (False, True):
            step = max(1, hw // 9)
            n_steps = -(-hw // step)
            flip = K.flip_steps(rk[0].contiguous(), desc, step)
            emit(f"flip_steps {hw} desc={desc}", flip)
            emit(f"segment_sums {hw} desc={desc}", *K.segment_sums(dev(sal), order[0].contiguous(), desc, step, n_steps))
            for sh in (False, True):
                emit(f"perturb_batch {C}x{H}x{W} desc={desc} shift={sh}",
                     K.perturb_batch(dev(randn(*shape), sh), dev(randn(*shape), sh), flip, 2, 5, out=dev(torch.zeros(5, *shape), sh)))
    for k in (1, 10, 65, 1000):
        z = dev(edge_logits(k))
        emit(f"softmax_stats K={k}", *K.softmax_stats(z), *K.softmax_stats(z, target=k - 1),
             *K.softmax_stats(z, target=dev(torch.tensor([k // 2], dtype=torch.int32)), want_entropy=False))


def masker_entries():
    for (h, w), (H, W) in (((7, 7), (32, 32)), ((5, 6), (27, 31)), ((14, 14), (28, 32))):
        src = dev(randn(5, h, w))
        emit(f"up_rownorm {h}x{w}->{H}x{W}", K.up_rownorm(src, H, W))
    for R, P in ((5, 1024), (3, 189), (9, 2511), (2, 3072)):
        for sh in (False, True):
            rows = dev(randn(R, P), sh)
            emit(f"rownorm {R}x{P} shift={sh}", K.rownorm(rows))
            inplace = dev(randn(R, P), sh)
            emit(f"rownorm in place {R}x{P} shift={sh}", K.rownorm(inplace, out=inplace))
            members = dev(torch.randperm(R, generator=GEN).to(torch.int32))
            offs = dev(torch.tensor([0, R // 2, R], dtype=torch.int32))
            emit(f"cluster_sum {R}x{P} shift={sh}", K.cluster_sum(rows, members, offs))
            emit(f"masked_sums {R}x{P} shift={sh}", *K.masked_sums(rows, dev(randn(R))))
    for tag, shape, sh in variants():
        C, H, W = shape
        emit(f"causal_apply {tag}", K.causal_apply(dev(randn(*shape), sh), dev(torch.rand(4, H * W, generator=GEN), sh), dev(randn(4, *shape), sh)))


def vit_entries():
    for L, H, S, D in ((2, 3, 17, 24), (3, 2, 65, 40)):
        attns = [dev(torch.softmax(randn(H, S, S), -1)) for _ in range(L)]
        grads = [dev(randn(H, S, S)) for _ in range(L)]
        Ih = K.attn_head_importance(attns, grads)
        acts = [[dev(randn(S, D)) for _ in range(L)] for _ in range(4)]
        b1, b2 = K.residual_shares(*acts)
        aug = K.rave_matrices(attns, Ih, b1, b2)
        aug_g = K.rave_matrices(attns, Ih, b1, b2, bgrads=grads, ablate=1)
        emit(f"vit L={L} H={H} S={S}", Ih, b1, b2, aug, aug_g, K.rollout_row(aug, 0), K.rollout_row(torch.stack([aug, aug_g]), S - 1))
    for B, H, S in ((2, 3, 17), (1, 4, 197), (2, 2, 1025), (1, 1, 2050)):
        attn = dev(torch.rand(B, H, S, S, generator=GEN))
        emit(f"attn_cam {B}x{H}x{S}", K.attn_cam(attn, dev(randn(B, H, S, S))), K.attn_cam(attn, dev(torch.ones(B, H, S, S))))


def gig_entries():
    for tag, shape, sh in variants():
        for grads in ("normal", "spiced"):
            xi, xb = dev(torch.rand(2, *shape, generator=GEN), sh), dev(torch.rand(2, *shape, generator=GEN) * 0.1, sh)
            xb[1, 0, 0, :3] = xi[1, 0, 0, :3]                                   # features that never move
            for fraction in (0.0, 0.25, 1.0):
                x, attr = dev(torch.zeros(2, *shape), sh), dev(torch.zeros(2, *shape), sh)
                l1, state = dev(torch.zeros(2)), dev(torch.zeros(8, dtype=torch.int32))
                K.gig_init(xi, xb, x, attr, l1, state)
                emit(f"gig_init {tag} {grads} f={fraction}", x, attr, l1, state)
                g_gen = torch.Generator().manual_seed(7)
                for step in range(4):
                    g = torch.randn(2, *shape, generator=g_gen)
                    if grads == "spiced":
                        f = g.view(2, -1)
                        f[:, 1::5] = f[:, :1]
                        f[:, 2::9] = 0.0
                        f[:, 3::9] = -0.0
                        f[0, 5], f[0, 6], f[1, 7] = INF, -INF, -INF
                    K.gig_step(xi, xb, dev(g, sh), 4, fraction, 0.02, x, attr, l1, state)
                    emit(f"gig_step {step} {tag} {grads} f={fraction}", x, attr, state)


def agi_entries():
    for n_out in (1, 10, 65, 1000):
        for tag, shape, sh in variants():
            if n_out != 10 and shape != SHAPES[0]:
                continue
            lg = edge_logits(n_out)
            B = lg.shape[0]
            classes = dev(torch.tensor(sorted({0, n_out // 2, n_out - 1}), dtype=torch.int32))
            Kc = classes.numel()
            n = int(np.prod(shape))
            data = dev(torch.rand(B, *shape, generator=GEN), sh)
            x_cur, c_delta = dev(torch.zeros(B * Kc, n), sh), dev(torch.zeros(B * Kc, n), sh)
            state, pred = dev(torch.zeros(4 * B * Kc, dtype=torch.int32)), dev(torch.zeros(B, dtype=torch.int64))
            K.agi_init(dev(lg), data, classes, pred, x_cur, c_delta, state)
            emit(f"agi_init n_out={n_out} {tag}", pred, x_cur, c_delta, state)
            for it in range(3):
                lgs = torch.cat([edge_logits(n_out) for _ in range(Kc)])[: B * Kc]
                g_adv = spiced(B * Kc, n)
                g_adv[0, 0] = NAN
                K.agi_step(dev(lgs), dev(g_adv, sh), dev(randn(B * Kc, n), sh), data, classes, 0.05, 2, x_cur, c_delta, state)
                emit(f"agi_step {it} n_out={n_out} {tag}", x_cur, c_delta, state)
    for n_img, Kc, C, H, W in ((2, 3, 3, 32, 32), (2, 2, 3, 7, 9), (1, 1, 1, 8, 8), (2, 2, 3, 31, 27), (1, 2, 2, 1, 1)):
        for nan in (False, True):
            cd = spiced(n_img * Kc, C, H, W)
            if nan:
                cd[0, 0, H // 2, W // 2] = NAN                                          # image 0 only
            for q_lo, q_hi in ((80, 99), (0, 100), (50, 50.5)):
                sg, qu = dev(torch.zeros(n_img, C, H, W)), dev(torch.zeros(n_img, 2))
                emit(f"agi_heatmap {n_img}x{Kc}x{C}x{H}x{W} nan={nan} q=({q_lo},{q_hi})", K.agi_heatmap(dev(cd), n_img, q_lo, q_hi, step_grad=sg, qu=qu), sg, qu)
            emit(f"agi_heatmap {n_img}x{Kc}x{C}x{H}x{W} nan={nan} map only", K.agi_heatmap(dev(cd), n_img))


def ablation_entries():
    for tag, shape, sh in variants():
        C, H, W = shape
        x = dev(randn(2, *shape), sh)
        base = dev(randn(*shape), sh)
        ids = torch.randint(2, 9, (H, W), generator=GEN, dtype=torch.int32)
        ids_c = torch.randint(2, 9, shape, generator=GEN, dtype=torch.int32)
        for nm, idt in (("hw", ids), ("chw", ids_c)):
            idd = dev(idt, sh)
            emit(f"ablate_features {nm} {tag}", K.ablate_features(x, idd, 2, 7, base, 3, 9), K.ablate_features(x, idd, 2, 7, 0.5, 0, 14))
            s0, scores = dev(randn(2)), dev(randn(2, 7))
            emit(f"ablation_finish_features {nm} {tag}", *K.ablation_finish_features(s0, scores, idd, 2, (2, C, H, W), g=3))
        window, strides = (min(4, H), min(3, W)), (2, 2)
        ch, cw = K.window_counts(H, W, window, strides)
        emit(f"ablate_windows {tag}", K.ablate_windows(x, window, strides, base, 1, 2 * ch * cw - 1), K.ablate_windows(x, window, strides, 0.0, 0, 3))
        emit(f"ablation_finish_windows {tag}", *K.ablation_finish_windows(dev(randn(2)), dev(randn(2, ch * cw)), window, strides, (2, C, H, W), g=2))


def xrai_entries():
    for H, W in ((32, 32), (7, 9), (31, 27)):
        labels = torch.randint(1, 6, (2, H, W), generator=GEN, dtype=torch.int32)
        lo, hi = dev(torch.tensor([1, 1], dtype=torch.int32)), dev(torch.tensor([5, 5], dtype=torch.int32))
        masks = (torch.rand(4, H, W, generator=GEN) < 0.2).to(torch.uint8)
        masks[3] = 0
        attr = randn(2, H, W)
        for radius in (0, 2):
            bits_l, span_l = K.xrai_pack(H, W, radius, 10, labels=dev(labels), label_min=lo, label_max=hi)
            bits_m, span_m = K.xrai_pack(H, W, radius, 4, masks=dev(masks))
            emit(f"xrai_pack {H}x{W} r={radius}", bits_l, span_l, bits_m, span_m)
            first = dev(torch.tensor([0, 5, 10], dtype=torch.int32))
            for fast in (False, True):
                emit(f"xrai_rank labels {H}x{W} r={radius} fast={fast}", *K.xrai_rank(dev(attr), bits_l, span_l, first, 3, 0.9, fast=fast))
            emit(f"xrai_rank masks {H}x{W} r={radius}", *K.xrai_rank(dev(attr[:1]), bits_m, span_m, dev(torch.tensor([0, 4], dtype=torch.int32)), 1, 1.0))


def lime_gshap_entries():
    for tag, shape, sh in variants():
        C, H, W = shape
        x = dev(randn(2, *shape), sh)
        seg = dev(torch.randint(-1, 70, (2, H, W), generator=GEN, dtype=torch.int32))       # -1 and 66 .. 69 are no row's to switch off
        bits = torch.randint(0, 2, (10, 66), generator=GEN)
        bits[0], bits[1] = 1, 0
        rows = torch.zeros(10, 2, dtype=torch.int64)
        for z in range(66):
            rows[:, z // 64] |= bits[:, z] << (z % 64)
        rows, D = dev(rows), dev(torch.tensor([66, 40], dtype=torch.int32))
        emit(f"lime_compose {tag}", K.lime_compose(x, seg, rows, D, dev(randn(C)), 3, 6),
             K.lime_compose(x, seg, rows, D, None, 0, 10, fudged=dev(randn(2, *shape), sh)))
        x_rows, base = dev(randn(8, *shape), sh), dev(randn(3, *shape), sh)
        alpha, idx = dev(torch.rand(8, generator=GEN)), dev(torch.randint(0, 3, (8,), generator=GEN))
        emit(f"gshap_scale {tag}", K.gshap_scale(x, base, alpha, idx, 4, out=dev(torch.zeros(8, *shape), sh)),
             K.gshap_scale(x_rows, base, alpha, idx, 4, out=dev(torch.zeros(8, *shape), sh)))
        g = dev(spiced(8, *shape), sh)
        emit(f"gshap_finish {tag}", *K.gshap_finish(g, x, base, idx, 4, want_map=True, attr=dev(torch.zeros(2, *shape), sh)),
             K.gshap_finish(g, x_rows, base, idx, 4, want_attr=False, want_map=True))


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--lib", help="another build of libxai_hip.so to load instead of the package's")
    ap.add_argument("--ext-lib", help="another build of libxai_ext.so to load instead of the package's")
    args = ap.parse_args()
    if args.lib:
        _lib.LIBRARIES["hip"].path = os.path.abspath(args.lib)
    if args.ext_lib:
        _lib.LIBRARIES["ext"].path = os.path.abspath(args.ext_lib)
    _lib.load()
    for part in (ig_entries, cam_rise_blur_entries, insdel_entries, masker_entries, vit_entries, gig_entries, agi_entries, ablation_entries,
                 xrai_entries, lime_gshap_entries):
        part()


if __name__ == "__main__":
    main()
