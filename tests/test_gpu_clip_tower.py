"""The ten CLIP rows through sweep.get_CLIP_attr against image 0 of their row module's batch function, on the device: one dispatch,
one tower layer, the same bytes."""
import os

import numpy as np
import pytest
import torch

import m2ib_restated as M
import clip_restated as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = ("eclip", "eclip_wo", "eclip_nograd", "maskclip", "selfattn", "game", "rollout", "lrp", "surgery", "m2ib")
SEED = 11
_MODEL = []


def dev_model():
    """the twelve-block mini CLIP of the M2IB fixtures in mixed fp16, frozen: the one stored model that every row takes (surgery
    needs six blocks, m2ib's layer 9 eleven)"""
    if not _MODEL:
        from xai_engine import zoo
        res, patch, width, n, heads, embed, _ = M.MODELS["seventeen"]
        m = zoo.clip_vit(0, embed_dim=embed, image_resolution=res, vision_layers=n, vision_width=width, vision_patch_size=patch,
                         vision_heads=heads, **M.TEXT)
        z = np.load(os.path.join(GOLDEN, "m2ib_w_seventeen.npz"), allow_pickle=False)
        m.load_state_dict({k: torch.from_numpy(z[k]).float() for k in z.files}, strict=True)
        _MODEL.append(zoo.convert_weights_fp16(m).to(DEV).eval())
    return _MODEL[0]


@pytest.mark.parametrize("row", ROWS)
def test_get_clip_attr_is_image_0_of_the_rows_batch_function_bit_for_bit(row):
    from xai_engine import clip_attn, eclip, m2ib, surgery, sweep
    m = dev_model()
    imgs = [R.fixture_image(seed, 32, 32) for seed in (3, 4)]
    emb = 3.0 * R.fixture_texts(5, 3, 16).to(DEV)                              # the target class is row 1; the rows are not normalised
    context = 0.5 * R.fixture_texts(6, 4, 16)
    table = m2ib.wrapper_text_features(m, torch.cat([M.fixture_ids(s) for s in (7, 8, 9)]).to(DEV))
    td = {"attr_func": row, "models": [m], "img_hw": 48, "embeddings": emb, "device": DEV, "device_maps": True,
          "clip_attention_rows": "plain", "clip_surgery": "plain", "surgery_text_features": context,
          "clip_m2ib": "plain", "m2ib_text_features": table, "m2ib_noise": "host", "m2ib_seed": SEED}
    got = sweep.get_CLIP_attr(imgs[0], 1, td)
    txt = torch.nn.functional.normalize(emb[1][None], dim=-1)
    x = torch.cat([sweep.clip_keepsize_input(i, (1, 1) if row not in eclip.METHODS else (16, 16)) for i in imgs])
    if row in eclip.METHODS:
        want = eclip.eclip_batch(m, x, txt, row, img_hw=48)
    elif row in clip_attn.METHODS:
        want = clip_attn.attention_rows_batch(m, x, txt, row, img_hw=48)
    elif row == "surgery":
        want = surgery.surgery_batch(m, x, torch.nn.functional.normalize(torch.cat([emb[1][None].float(), context.to(DEV)]), dim=-1), img_hw=48)
    else:
        want = m2ib.m2ib_batch(m, x, table[1], img_hw=48, noise="host", seed=SEED)
    assert got.is_cuda and tuple(got.shape) == (48, 48) and tuple(want.shape) == (2, 48, 48)
    assert got.cpu().numpy().tobytes() == want[0].cpu().numpy().tobytes()
    assert not np.isnan(want.cpu().numpy()).any() and (want[0] != want[1]).any()
