"""Reference module path `util.attribution_methods.XRAIBuilder` (imported at evaluatePerturbation.py:44): XRAI, XRAIParameters,
XRAIOutput (:295-616 of the reference file) and call_model_function (:376-390) on the HIP engine (xai_engine/xrai.py: the
segments are packed by K29, the greedy loop of XRAI._xrai / _xrai_fast, :619-789, runs in K30).  The rest of that file
(CoreSaliency, the Felzenszwalb helpers, the key constants, ...) is not served: asking this module for one of those names loads
the same-named file of the next `util` on sys.path on first use (xai_engine/_shim.py) and hands its attribute over."""
from xai_engine._shim import fall_through as _fall_through
from xai_engine.xrai import XRAI, XRAIOutput, XRAIParameters, call_model_function  # noqa: F401

__getattr__ = _fall_through(__name__, __file__)
