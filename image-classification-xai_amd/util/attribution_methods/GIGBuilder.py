"""Reference module path `util.attribution_methods.GIGBuilder`, Guided IG part only (GuidedIG.GetMask :312-372 and
call_model_function :296-310 of the reference file, imported at evaluatePerturbation.py:41) on the HIP engine
(xai_engine/guided_ig.py: every step's inner loop runs in the K22 kernel).  The rest of that file (CoreSaliency,
IntegratedGradients, the visualisation helpers, the key constants, ...) is not served: asking this module for one of those
names loads the same-named file of the next `util` on sys.path on first use (xai_engine/_shim.py) and hands its attribute
over.  CoreSaliency.GetSmoothedMask stays the reference's own."""
from xai_engine._shim import fall_through as _fall_through
from xai_engine.guided_ig import GuidedIG, call_model_function  # noqa: F401

__getattr__ = _fall_through(__name__, __file__)
