"""Reference module path `util.attribution_methods.VIT_LRP.ViT_explanation_generator`
(imported at evaluatePerturbation.py:45): `Baselines` (:135-520 of the reference file -- attention-space
IG, rollouts, transition attention maps, bidirectional attribution, generate_cam_attn, generate_RAVE) and `LRP` (:107-133 --
Transformer Attribution, `generate_LRP`, on the engine's hooked ViT: xai_engine/lrp.py) on the HIP engine.

`LRP` is the engine's unless a reference tree follows on sys.path: that tree's own `LRP` runs on its timm-derived relprop twin of the
model (`models[1]` of its harness), which the engine's does not take, so there the name keeps resolving to the reference's, as it
always has.  The harness rows of this build (`--attr_func t_attr`) call xai_engine.lrp directly.  The helpers of the reference file
are out of scope and are taken, on first use, from the same-named file of the next `util` on sys.path (xai_engine/_shim.py)."""
from xai_engine._shim import fall_through as _fall_through
from xai_engine._shim import next_file as _next_file
from xai_engine.vit_attr import Baselines  # noqa: F401

_next = _fall_through(__name__, __file__)


def __getattr__(attr):
    if attr == "LRP" and _next_file(__name__, __file__) is None:
        from xai_engine.lrp import LRP
        return LRP
    return _next(attr)
