"""The streamed workgroup prefix sum (block_scan_excl, csrc/xai_common.h) through its four 1024-lane users, K68 slic_number, K74
felz_labels, K55 quickshift_labels and the counter scan of felz_sort, at the sizes where a pass of 1024 lanes and a wave of 64 begin
and end: n = H * W of 1, 63, 64, 65 (one wave and its neighbours), 1023, 1024, 1025 (one pass and its neighbours), 2049 and 3 * 1024
(a third pass of one element, and three full ones), as one row and once as 25 x 41.  Every call has three images, so that the
carry of one image must not reach the next: a seeded map, every pixel its own root, one root at pixel 0.

All maps and all expected arrays are made on the host (tests/slic_restated.py, felzenszwalb_restated.py, quickshift_restated.py,
np.argsort); everything is an integer and compared exactly.  The select kernel of MDA, the fifth user, is held by
tests/test_gpu_mda.py."""
import functools

import numpy as np
import pytest
import torch

import felzenszwalb_restated as FR
import quickshift_restated as QR
import slic_restated as SR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 1), (1, 63), (1, 64), (1, 65), (1, 1023), (1, 1024), (1, 1025), (25, 41), (1, 2049), (1, 3 * 1024)]
# felz_sort scans 256 * ceil(E / 1024) counters an image, E = W - 1 edges in a row of W pixels.  (1, 4097): E = 4096, four chunks, 1024
# counters, exactly one pass.  (1, 4098): E = 4097 crosses a multiple of 1024, a fifth chunk of one edge, 1280 counters: a second pass.
SORT_SHAPES = SHAPES + [(1, 4097), (1, 4098)]


def _ids(shapes):
    return [f"{h}x{w}" for h, w in shapes]


@pytest.fixture(scope="module")
def K():
    from xai_engine import kernels
    return kernels


def _dev(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _rng(kind, n):
    return np.random.RandomState(1000 * kind + n % 1000 + n // 1000)


@functools.lru_cache(maxsize=None)
def first_pixel_maps(n):
    """(3, n): comp[p] = the first pixel of p's component, so comp[p] <= p and comp[comp[p]] = comp[p]"""
    rng = _rng(1, n)
    first = rng.rand(n) < 0.3
    first[0] = True
    seeded = np.zeros(n, np.int64)
    for p in range(n):
        seeded[p] = p if first[p] else rng.choice(np.flatnonzero(first[:p]))
    return np.stack([seeded, np.arange(n), np.zeros(n, np.int64)])


@functools.lru_cache(maxsize=None)
def root_maps(n):
    """(3, n): roots[p] = the root of p's tree, anywhere in the image, roots[roots[p]] = roots[p]"""
    rng = _rng(2, n)
    is_root = rng.rand(n) < 0.4
    is_root[rng.randint(n)] = True
    where = np.flatnonzero(is_root)
    seeded = np.where(is_root, np.arange(n), where[rng.randint(len(where), size=n)])
    return np.stack([seeded, np.arange(n), np.zeros(n, np.int64)])


@functools.lru_cache(maxsize=None)
def parent_forests(n):
    """(3, n): a seeded forest (a pixel's parent comes earlier in a random order, or is the pixel itself), every pixel a root, and
    the chain n - 1 -> n - 2 -> ... -> 0 of n - 1 links"""
    rng = _rng(3, n)
    order = rng.permutation(n)
    seeded = np.arange(n)
    for j in range(1, n):
        if rng.rand() >= 0.1:
            seeded[order[j]] = order[rng.randint(j)]
    return np.stack([seeded, np.arange(n), np.maximum(np.arange(n) - 1, 0)])


@pytest.mark.parametrize("start_label", [0, 1])
@pytest.mark.parametrize("H,W", SHAPES, ids=_ids(SHAPES))
def test_slic_number_ranks_the_first_pixels_in_pixel_order(K, H, W, start_label):
    comp = first_pixel_maps(H * W).reshape(3, H, W)
    out, counts = K.slic_number(_dev(comp), start_label)
    want = [SR.number(c, start_label) for c in comp]
    assert np.array_equal(out.cpu().numpy(), np.stack([w[0] for w in want]))
    assert counts.tolist() == [w[1] for w in want]


@pytest.mark.parametrize("H,W", SHAPES, ids=_ids(SHAPES))
def test_felz_labels_ranks_the_roots_in_pixel_order(K, H, W):
    roots = root_maps(H * W)
    labels, counts, status = K.felz_labels(_dev(roots.reshape(3, H, W)))
    want = [FR.labels_of(r) for r in roots]
    assert np.array_equal(labels.cpu().numpy().reshape(3, -1), np.stack([w[0] for w in want]))
    assert counts.tolist() == [w[1] for w in want] and status.tolist() == [0]


@pytest.mark.parametrize("H,W", SHAPES, ids=_ids(SHAPES))
def test_quickshift_labels_numbers_the_roots_of_a_forest_and_of_a_chain(K, H, W):
    parent = parent_forests(H * W).reshape(3, H, W)
    labels, D = K.quickshift_labels(_dev(parent))
    want = [QR.labels_of(p) for p in parent]
    assert np.array_equal(labels.cpu().numpy(), np.stack([w[0] for w in want]))
    assert D.tolist() == [w[1] for w in want]


@pytest.mark.parametrize("H,W", SORT_SHAPES, ids=_ids(SORT_SHAPES))
def test_felz_sort_is_stable_where_ties_dominate(K, H, W):
    E = K.felz_edges(H, W)
    values = np.array([1e-300, 0.1, 0.3]).view(np.int64)          # the bits of three costs; all eight digits of the key differ
    keys = values[_rng(4, H * W).randint(3, size=(3, max(E, 1)))]
    index = np.tile(np.arange(max(E, 1)), (3, 1))
    got_keys, got_index = K.felz_sort(_dev(keys, np.int64), _dev(index), H, W)
    order = np.argsort(keys, axis=1, kind="stable")
    assert np.array_equal(got_index.cpu().numpy(), order)
    assert np.array_equal(got_keys.cpu().numpy(), np.take_along_axis(keys, order, axis=1))

