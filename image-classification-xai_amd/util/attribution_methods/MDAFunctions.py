"""Reference module path `util.attribution_methods.MDAFunctions` (imported at evaluatePerturbation.py:48): MDA,
find_insertion_patches, find_deletion_patches and normalize_curve (:12-626 of the reference file) on the HIP engine
(xai_engine/mda.py: the candidate images of a search step are composed by K36, the step's decision is K37, the winner is
committed by K38, one hipGraph replay per step).  Every other name is not served: asking this module for it loads the
same-named file of the next `util` on sys.path on first use (xai_engine/_shim.py) and hands its attribute over."""
from xai_engine._shim import fall_through as _fall_through
from xai_engine.mda import MDA, find_deletion_patches, find_insertion_patches, normalize_curve  # noqa: F401

__getattr__ = _fall_through(__name__, __file__)
