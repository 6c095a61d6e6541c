"""csrc/xai_launch_plan.h on the CPU: the row-chunk plan that K6 (xai_perturb_batch_f32), K26 (xai_ablate_*_f32), K31
(xai_lime_compose_f32) and K1 (xai_ig_interp_f32) share must give each of them the grid it computed for itself before the plan
was shared.  The header is built alone by the host compiler (tests/launch_plan_main.cpp: it needs nothing of HIP) and asked for
the plan of every case below.  The expected values never come from the header: K6's are insdel_restated.perturb_plan's, the
others are restated here from the text of the four entries as they stood before the plan was shared."""
import os
import subprocess

import pytest

import insdel_restated as R
from conftest import PKG, ROOT

BLOCK = 256
MIB = 1 << 20


def _ceil(a, b):
    return -(-a // b)


def _tiles(length, vec):
    return _ceil(length, BLOCK * (4 if vec else 1))


def _finish(tiles, n, per, zdim, hbm):
    chunks = _ceil(n, per)
    return tiles, chunks, zdim, per, int(chunks <= 65535), int(hbm)


def plan_k26(C, hw, n, vec):
    """launch_ablate: K6's plan over the rows of a pass"""
    tiles, zdim = _tiles(hw, vec), 1
    hbm = n * C * hw * 4 >= 64 * MIB and C <= 64
    if hbm:
        per, zdim = (2 if n >= 2 else 1), C
    else:
        c0 = min(n, max(1, _ceil(2048, tiles)))
        per = _ceil(n, c0)
    return _finish(tiles, n, per, zdim, hbm)


def plan_k31(chw, n, vec):
    """xai_lime_compose_f32 in front of its LDS clamp: the row spans the channels, which are never split"""
    tiles = _tiles(chw, vec)
    hbm = n * chw * 4 >= 64 * MIB
    if hbm:
        per = 2 if n >= 2 else 1
    else:
        c0 = min(n, max(1, _ceil(2048, tiles)))
        per = _ceil(n, c0)
    return _finish(tiles, n, per, 1, hbm)


def plan_k1(n_elem, n_alpha, n_img, vec):
    """xai_ig_interp_f32: 256 MiB over all images, which also multiply the workgroups of a chunk"""
    tiles = _tiles(n_elem, vec)
    hbm = n_img * n_alpha * n_elem * 4 >= 256 * MIB
    if hbm:
        per = 2 if n_alpha >= 2 else 1
    else:
        c0 = min(n_alpha, max(1, _ceil(2048, tiles * n_img)))
        per = _ceil(n_alpha, c0)
    return _finish(tiles, n_alpha, per, 1, hbm)


def _k6_cases():
    """(header arguments, expected line) of every case insdel_restated lists for perturb_plan and tests/test_cpu_insdel.py adds"""
    listed = [c[:3] + (True,) for c in R.K6_SMALL + R.K6_HBM + (R.K6_REFUSED,)]
    listed += [(1, 524032, 3, False), (4, 4096, 1024, False), (3, 4099, 1364, True), (1, 132, 131070, True), (1, 4, 1 << 20, True), (1, 1, 1, True)]
    for C, hw, n, aligned in listed:
        vec, per, chunks, zdim = R.perturb_plan(C, hw, n, aligned=aligned)
        hbm = n * C * hw * 4 >= R.HBM_BYTES and C <= 64
        yield (hw, BLOCK, int(vec), n, C, 1, R.HBM_BYTES, 1), (_tiles(hw, vec), chunks, zdim, per, int(chunks <= 65535), int(hbm))


# (C, row length, rows): at 64 MiB and one row below it, C = 64 against 65 at HBM size, one row at HBM size, 2048 tiles and more,
# one tile, 65 536 chunks against 65 535, lengths that are no multiple of 4
ROWS_64MIB = ((4, 4096, 1024), (4, 4096, 1023), (64, 1024, 256), (65, 1024, 256), (64, 1024, 255), (1, 1 << 24, 1), (1, (1 << 24) - 1, 1),
              (3, 4096, 1366), (3, 4096, 1365), (1, 2048 * 1024, 3), (1, 2048 * 1024 + 1, 7), (1, 2047 * 1024, 3), (3, 4, 1), (3, 4, 2049), (3, 5, 2049),
              (1, 132, 131072), (1, 132, 131071), (1, 132, 131070), (3, 4099, 1365), (3, 4099, 1364), (2, 1021, 13), (3, 3001, 1009))
# (n_elem, n_alpha, n_img): 256 MiB with 2 images and one row below it, one image, tiles * n_img at and over 2048, one tile
ROWS_K1 = ((65536, 512, 2), (65536, 511, 2), (65536, 1024, 1), (65536, 1023, 1), (1 << 26, 1, 1), (3000, 1000, 2), (3001, 1000, 3), (150528, 50, 16), (150528, 5, 16),
           (150528, 50, 1), (1024, 5, 2), (7, 1, 1), (131, 131072, 4), (131, 131070, 4), (1024 * 1024, 9, 2), (1024 * 1024 + 3, 9, 2))


def _cases():
    out = [("K6",) + c for c in _k6_cases()]
    for vec in (0, 1):
        for C, hw, n in ROWS_64MIB:
            out.append(("K26", (hw, BLOCK, vec, n, C, 1, 64 * MIB, 1), plan_k26(C, hw, n, vec)))
            out.append(("K31", (C * hw, BLOCK, vec, n, 1, 1, 64 * MIB, 0), plan_k31(C * hw, n, vec)))
        for n_elem, n_alpha, n_img in ROWS_K1:
            out.append(("K1", (n_elem, BLOCK, vec, n_alpha, 1, n_img, 256 * MIB, 0), plan_k1(n_elem, n_alpha, n_img, vec)))
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("launch_plan") / "launch_plan"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(PKG, "csrc"),
           os.path.join(ROOT, "tests", "launch_plan_main.cpp"), "-o", str(path)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(path)


def test_the_shared_plan_is_each_entrys_own(exe):
    cases = _cases()
    args = [str(v) for _, a, _ in cases for v in a]
    lines = subprocess.run([exe] + args, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == len(cases)
    for (who, a, want), line in zip(cases, lines):
        assert tuple(int(v) for v in line.split()) == tuple(want), (who, a, line, want)


def test_the_cases_reach_every_edge():
    """what the list above claims, from the restatements alone"""
    assert plan_k26(4, 4096, 1024, 1)[2:4] == (4, 2) and plan_k26(4, 4096, 1023, 1)[2] == 1               # at 64 MiB and one row below
    assert plan_k26(64, 1024, 256, 1)[2] == 64 and plan_k26(65, 1024, 256, 1)[2:] == (1, 1, 1, 0)         # C = 65 is never split
    assert plan_k31(65 * 1024, 256, 1)[2:] == (1, 2, 1, 1)                                                 # K31 has no such bound
    assert plan_k26(1, 1 << 24, 1, 1)[1:] == (1, 1, 1, 1, 1)                                               # one row at HBM size
    assert plan_k26(1, 2048 * 1024, 3, 1)[:4] == (2048, 1, 1, 3) and plan_k26(3, 4, 2049, 1)[:4] == (1, 1025, 1, 2)
    assert plan_k31(132, 131072, 0)[1:] == (65536, 1, 2, 0, 1) and plan_k31(132, 131070, 0)[1:] == (65535, 1, 2, 1, 1)
    assert plan_k26(3, 4096, 1366, 1)[5] == 1 and plan_k26(3, 4096, 1365, 1)[5] == 0                       # the GPU tests' pair of passes
    assert plan_k1(65536, 512, 2, 1)[3:] == (2, 1, 1) and plan_k1(65536, 511, 2, 1)[5] == 0               # 256 MiB over 2 images
    assert plan_k1(65536, 1023, 1, 1)[5] == 0 and plan_k26(1, 65536, 1023, 1)[5] == 1                      # K1's threshold is its own
    assert plan_k1(3000, 1000, 2, 1)[:4] == (3, 334, 1, 3) and plan_k1(3000, 1000, 1, 1)[:4] == (3, 500, 1, 2)        # images multiply the tiles
    assert plan_k1(150528, 5, 16, 1) == (147, 1, 1, 5, 1, 0) and plan_k1(150528, 50, 16, 1)[3:] == (2, 1, 1)        # 2352 workgroups a chunk
    assert plan_k26(3, 4099, 1365, 0)[0] == 17 and plan_k26(3, 4099, 1365, 1)[0] == 5                      # both flavours of an odd length
