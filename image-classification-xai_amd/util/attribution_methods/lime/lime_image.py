"""Reference module path `util.attribution_methods.lime.lime_image`: LimeImageExplainer and ImageExplanation (lime_image.py:19-220)
on the HIP engine (xai_engine/lime.py).  Any other name is taken from the same-named file of the next `util` on sys.path on
first use (xai_engine/_shim.py)."""
from xai_engine._shim import fall_through as _fall_through
from xai_engine.lime import ImageExplanation, LimeImageExplainer  # noqa: F401

__getattr__ = _fall_through(__name__, __file__)
