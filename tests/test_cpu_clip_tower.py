"""xai_engine/clip_tower.py without a GPU: the one layout check under every row's name, the one native-resolution check, the
written-out attention block against the block's own forward, and the order in which sweep.get_CLIP_attr looks at its option keys."""
import os

import numpy as np
import pytest
import torch

import m2ib_restated as M
from conftest import GOLDEN

ROWS = ("eclip", "clip_attn", "surgery", "m2ib", "game")                      # the four modules' names, and any other string


def zoo_model(fp16=False):
    """the twelve-block mini CLIP of the M2IB fixtures with its stored weights: every row's model"""
    from xai_engine import zoo
    res, patch, width, n, heads, embed, _ = M.MODELS["seventeen"]
    m = zoo.clip_vit(0, **dict(embed_dim=embed, image_resolution=res, vision_layers=n, vision_width=width, vision_patch_size=patch,
                               vision_heads=heads, **M.TEXT))
    z = np.load(os.path.join(GOLDEN, "m2ib_w_seventeen.npz"), allow_pickle=False)
    m.load_state_dict({k: torch.from_numpy(z[k]).float() for k in z.files}, strict=True)
    return zoo.convert_weights_fp16(m) if fp16 else m


@pytest.mark.parametrize("row", ROWS)
def test_check_layout_names_the_missing_attribute_and_the_row(row):
    from xai_engine import clip_tower
    visual, blocks, H = clip_tower.check_layout(zoo_model(), row, every_block=True, heads=True)
    assert len(blocks) == 12 and H == 2 and clip_tower.check_layout(zoo_model(), row)[2] is None
    with pytest.raises(TypeError, match=rf"^{row} needs a CLIP of OpenAI's layout: Linear has no `visual`$"):
        clip_tower.check_layout(torch.nn.Linear(2, 2), row)
    m = zoo_model()
    del m.visual.ln_post
    with pytest.raises(TypeError, match=rf"^{row} needs .*: CLIP has no `visual\.ln_post`$"):
        clip_tower.check_layout(m, row)
    m = zoo_model()
    del m.visual.transformer.resblocks[-1].attn.in_proj_bias
    with pytest.raises(TypeError, match=rf"^{row} needs .* has no `visual\.transformer\.resblocks\[-1\]\.attn\.in_proj_bias`$"):
        clip_tower.check_layout(m, row)
    m = zoo_model()
    del m.visual.transformer.resblocks[0].attn.num_heads
    with pytest.raises(TypeError, match=rf"^{row} needs .* has no `visual\.transformer\.resblocks\[0\]\.attn\.num_heads`$"):
        clip_tower.check_layout(m, row, every_block=True, heads=True)
    assert clip_tower.check_layout(m, row, heads=True)[2] == 2                  # the last block only: block 0 is not read
    assert clip_tower.check_layout(m, row, every_block=True)[2] is None         # no heads: num_heads is not read
    m.visual.transformer.resblocks[-1].attn.num_heads = 3
    with pytest.raises(TypeError, match=rf"^{row}: attn.num_heads = 3 does not divide the width 64$"):
        clip_tower.check_layout(m, row, heads=True)
    m.visual.transformer.resblocks = torch.nn.Sequential()
    with pytest.raises(TypeError, match=rf"^{row} needs .* has no `visual\.transformer\.resblocks\[-1\]`$"):
        clip_tower.check_layout(m, row)


def test_the_four_modules_checks_are_check_layout_under_their_names_and_only_two_refuse_a_resnet_by_name():
    from xai_engine import clip_attn, clip_tower, eclip, m2ib, surgery

    class ResNetTower(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.attnpool = torch.nn.Identity()
    resnet = torch.nn.Module()
    resnet.visual = ResNetTower()
    for row, check in (("surgery", surgery.check_model), ("m2ib", m2ib.check_model)):
        for call in (check, lambda model: clip_tower.check_layout(model, row)):
            with pytest.raises(NotImplementedError, match=rf"^{row}: a ResNet visual tower \(AttentionPool2d\) is not served; the reference's"):
                call(resnet)
    for row, check in (("eclip", eclip.check_layout), ("clip_attn", clip_attn.check_layout)):
        for call in (check, lambda model: clip_tower.check_layout(model, row)):
            with pytest.raises(TypeError, match=rf"^{row} needs .*: Module has no `visual\.conv1`$"):
                call(resnet)
    m = zoo_model()
    visual, last = eclip.check_layout(m)
    assert visual is m.visual and last is m.visual.transformer.resblocks[-1]
    for check in (clip_attn.check_layout, surgery.check_model, m2ib.check_model):
        v, blocks, H = check(m)
        assert v is m.visual and blocks == list(m.visual.transformer.resblocks) and H == 2


@pytest.mark.parametrize("row", ["clip_attn", "surgery", "m2ib"])
def test_native_input_refuses_what_is_not_the_models_own_square(row):
    from xai_engine import clip_tower
    visual = zoo_model().visual
    assert clip_tower.native_input(visual, torch.zeros(2, 3, 32, 32), row) == (32, (4, 4))
    for hw in ((32, 48), (64, 64), (16, 16)):
        with pytest.raises(NotImplementedError, match=rf"^{row}: x is {hw[0]} x {hw[1]}, the model's input_resolution is 32") as e:
            clip_tower.native_input(visual, torch.zeros(1, 3, *hw), row)
        assert "preprocess" in str(e.value)
    for bad in (torch.zeros(3, 32, 32), torch.zeros(1, 1, 32, 32), torch.zeros(1, 4, 32, 32), torch.zeros(1, 3, 32, 32, 1)):
        with pytest.raises(ValueError, match=r"^x must be \(B, 3, H, W\), got"):
            clip_tower.native_input(visual, bad, row)
    for bad in (None, np.zeros((1, 3, 32, 32), np.float32), [[0.0]]):
        with pytest.raises(TypeError, match=r"^x: expected a torch.Tensor, got"):
            clip_tower.native_input(visual, bad, row)


def test_written_out_block_is_the_blocks_own_forward_and_the_text_block_of_m2ib_is_its_output():
    """Bound: 1e-5 of the largest output, what tests/test_cpu_m2ib.py allows in fp32 between the written-out attention and
    nn.MultiheadAttention through a whole text tower and two projections (sums of at most 64 products ordered differently); one
    block makes fewer such sums."""
    from xai_engine import clip_tower, m2ib
    m = zoo_model()
    g = torch.Generator().manual_seed(3)
    visual_blk, text_blk = m.visual.transformer.resblocks[5], m.transformer.resblocks[0]
    text_mask, text_blk.attn_mask = text_blk.attn_mask, None                   # the written-out block takes no mask
    for blk, x, H in ((visual_blk, torch.randn(17, 2, 64, generator=g), 2), (text_blk, torch.randn(4, 3, 16, generator=g), 1)):
        with torch.no_grad():
            out, probs = clip_tower.written_out_block(blk, x, H)
            want = blk(x)
        L, N, _ = x.shape
        assert out.shape == want.shape and tuple(probs.shape) == (N * H, L, L)
        assert (probs.sum(-1) - 1).abs().max() <= 1e-6 and (probs >= 0).all()
        err = (out - want).abs().max().item()
        print(f"H = {H}: measured {err:.3e}, bound {1e-5 * want.abs().max().item():.3e}")
        assert err <= 1e-5 * want.abs().max().item()
    text_blk.attn_mask = text_mask
    with torch.no_grad():
        x = torch.randn(4, 3, 16, generator=g)
        assert torch.equal(m2ib._text_block(text_blk, x), clip_tower.written_out_block(text_blk, x, 1)[0])
        half = zoo_model(fp16=True).transformer.resblocks[0]
        assert torch.equal(m2ib._text_block(half, x.half()), clip_tower.written_out_block(half, x.half(), 1)[0])
    assert text_blk.attn_mask is not None                                      # the model's own block keeps its mask


def test_get_clip_attr_serves_a_row_before_it_looks_at_the_later_keys_and_checks_the_first_key_for_every_row():
    from xai_engine import _lib, sweep
    img = torch.zeros(3, 32, 32)
    td = {"models": [zoo_model(fp16=True)], "img_hw": 32, "embeddings": torch.zeros(2, 16), "device": "cpu"}
    assert [key for key, _, _ in sweep.CLIP_PLAIN_ROWS] == ["clip_attention_rows", "clip_surgery", "clip_m2ib"]
    with pytest.raises(_lib.XaiHipError, match="not a HIP GPU"):               # served (the model is on the CPU) before clip_surgery is read
        sweep.get_CLIP_attr(img, 0, dict(td, attr_func="game", clip_attention_rows="plain", clip_surgery="bogus"))
    with pytest.raises(ValueError, match="clip_attention_rows must be 'plain' or 'modified'"):
        sweep.get_CLIP_attr(img, 0, dict(td, attr_func="surgery", clip_attention_rows="bogus"))
    with pytest.raises(ValueError, match="clip_surgery must be 'plain' or 'modified'"):      # not served: every later key is read
        sweep.get_CLIP_attr(img, 0, dict(td, attr_func="game", clip_surgery="bogus"))
    with pytest.raises(ValueError, match="clip_m2ib must be 'plain' or 'modified'"):
        sweep.get_CLIP_attr(img, 0, dict(td, attr_func="eclip", clip_m2ib="bogus"))
