"""Reference module path `util.attribution_methods.lime.limeAttr` (imported at evaluatePerturbation.py:40): get_lime_attr,
batch_predict and make_tensor (limeAttr.py:8-36) on the HIP engine (xai_engine/lime.py: K31 builds the perturbed images, K32 fits,
K33 paints).  Any other name is taken from the same-named file of the next `util` on sys.path on first use
(xai_engine/_shim.py)."""
from xai_engine._shim import fall_through as _fall_through
from xai_engine.lime import batch_predict, get_lime_attr, make_tensor  # noqa: F401

__getattr__ = _fall_through(__name__, __file__)
