"""The connectivity pass of scikit-image 0.18.3's SLIC restated on the host, in Python and NumPy alone (no torch, so that the
interpreter that regenerates tests/golden/slic.npz can hold it to skimage's binary).  xai_engine/slic.py uses it for an irregular case
on a machine without scikit-image."""
import numpy as np


def enforce_connectivity_host(labels, min_size, max_size, start_label=0):
    """_enforce_label_connectivity_cython of _slic.pyx (0.18.3) restated for one (H, W) image: the raster scan with a breadth-first
    fill per unlabelled pixel (neighbours in the order x + 1, x - 1, y + 1, y - 1), cut at max_size, a component below min_size
    handed to the last labelled neighbour seen (0 if none).  The output starts as start_label - 1 everywhere, and that value means
    "unlabelled": with start_label = 1 a small component without a labelled neighbour goes back to 0, so a later fill of its raw
    label takes it in again (read off the binary, which the restatement equals for both start labels).  Sequential, pure Python:
    exact for any input and slow (about a second at 224 x 224); it only runs for an irregular case on a machine without
    scikit-image.  labels: the raw labels, from start_label up.  -> (H, W) int64."""
    seg = np.asarray(labels)
    if seg.ndim != 2:
        raise ValueError(f"enforce_connectivity_host: labels must be (H, W), got {seg.shape}")
    H, W = seg.shape
    seg = seg.astype(np.int64).tolist()
    unlabelled = int(start_label) - 1                  # what skimage fills its output with; `adjacent` starts at 0 whatever it is
    out = [[unlabelled] * W for _ in range(H)]
    current = int(start_label)
    max_size, min_size = int(max_size), int(min_size)
    for y in range(H):
        for x in range(W):
            if out[y][x] > unlabelled:
                continue
            adjacent = 0
            label = seg[y][x]
            out[y][x] = current
            coords = [(y, x)]
            visited = 0
            while visited < len(coords) < max_size:
                cy, cx = coords[visited]
                for yy, xx in ((cy, cx + 1), (cy, cx - 1), (cy + 1, cx), (cy - 1, cx)):
                    if 0 <= xx < W and 0 <= yy < H:
                        o = out[yy][xx]
                        if seg[yy][xx] == label and o == unlabelled:
                            out[yy][xx] = current
                            coords.append((yy, xx))
                            if len(coords) >= max_size:
                                break
                        elif o > unlabelled and o != current:
                            adjacent = o
                visited += 1
            if len(coords) < min_size:
                for cy, cx in coords:
                    out[cy][cx] = adjacent
            else:
                current += 1
    return np.asarray(out, dtype=np.int64)
