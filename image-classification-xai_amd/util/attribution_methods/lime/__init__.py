"""Reference package path `util.attribution_methods.lime` (evaluatePerturbation.py:40): limeAttr and lime_image are served by the
HIP engine (xai_engine/lime.py); lime_base, wrappers and utils resolve from the same-named directory of the next `util` on
sys.path (xai_engine/_shim.py)."""
from xai_engine._shim import extend as _extend

__path__ = _extend(__path__, __name__)
