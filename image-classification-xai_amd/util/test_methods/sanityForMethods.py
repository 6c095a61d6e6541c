"""Reference module path `util.test_methods.sanityForMethods`: normalize_image and evaluate (:60-92 of the reference file) on the
HIP engine (xai_engine/sanity.py: K39 without the constant-map guard, K40 SSIM, K8 + K41 + K42 Spearman, K43 HOG), and the layer
randomisation helpers get_layers, independent_layer_rand and cascading_layer_rand (:10-58) restated on the host, where they
always ran.  Every other name is not served: asking this module for it loads the same-named file of the next `util` on sys.path
on first use (xai_engine/_shim.py) and hands its attribute over."""
import numpy as np
import torch

from xai_engine import kernels as _K
from xai_engine import sanity as _sanity
from xai_engine._shim import fall_through as _fall_through

__getattr__ = _fall_through(__name__, __file__)


def get_layers(model):
    """The distinct first components of the parameter names, in order of first appearance (:10-18)."""
    return list(dict.fromkeys(name.split(".")[0] for name, _ in model.named_parameters()))


def _randomize(model, empty_model, prefixes):
    """Every parameter whose name starts with one of `prefixes` (visited prefix by prefix) takes empty_model's value, or
    torch.rand of its shape where empty_model's is all zero; then the state is loaded back (:22-38, :42-58)."""
    params, fresh = model.state_dict(), empty_model.state_dict()
    for prefix in prefixes:
        for name, _ in model.named_parameters():
            if name.startswith(prefix):
                all_zero = torch.nonzero(fresh[name]).numel() == 0
                params[name] = torch.rand(params[name].shape) if all_zero else fresh[name]
    model.load_state_dict(params)
    return model


def independent_layer_rand(model, empty_model, layer):
    """Layer `layer` alone is re-initialised from empty_model (:22-38)."""
    return _randomize(model, empty_model, [layer])


def cascading_layer_rand(model, empty_model, layers, index):
    """Layers layers[0 .. index] are re-initialised from empty_model (:42-58)."""
    return _randomize(model, empty_model, layers[:index + 1])


def normalize_image(x):
    """(:60-72) +-Inf -> 0, then (x - min) / (max - min) in float32, by K39 with guard = 0; a host array comes back as one."""
    if isinstance(x, torch.Tensor) and x.is_cuda:
        t = x.detach().to(torch.float32).contiguous()
        return _K.sanity_normalize(t.reshape(1, -1), guard=False).view(t.shape)
    arr = np.array(x).astype(np.float32)
    if arr.size == 0:
        raise ValueError("normalize_image: an empty map has no minimum")
    dev = _sanity.hip_device("cuda")
    out = _K.sanity_normalize(torch.from_numpy(np.ascontiguousarray(arr)).to(dev).reshape(1, -1), guard=False)
    return out.cpu().numpy().reshape(arr.shape)


def evaluate(normal_attr, random_layer_attr, abs=False):
    """(:75-92) -> (ssim_val, spr_val, hog_val) of one pair of maps, (H, W, 1) with abs=False or (H, W) with abs=True."""
    c = _sanity.get_sanity(normal_attr, random_layer_attr, abs=abs, guard=False)
    return c["SSIM"], c["SPR"], c["HOG"]
