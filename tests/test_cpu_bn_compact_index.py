"""The index helpers csrc/xai_bn_index.h holds for bnrelu_compact_kernels.hip, on the CPU: the image of a flat element (first of a
lane and by stepping), its place in the channel-major twin, and what a strided window reads.  Built alone by the host compiler
(tests/bn_compact_index_main.cpp), once plainly and once with -fsanitize=address,undefined -- that stand-alone program is the
sanitizer run of this arithmetic -- and both are asked the same cases.  The expected values are Python integers."""
import os
import subprocess

import pytest

from conftest import PKG, ROOT

# (N, C, HW): lanes that straddle channels and images (HW = 49, 9), four (image, channel) pairs in one lane (HW = 1, C = 1 and 2),
# a vector-path shape, C = 1 (every plane is a new image)
SMALL = ((4, 3, 49), (4, 2, 9), (4, 2, 1), (8, 1, 1), (3, 5, 196), (4, 1, 3), (50, 16, 49))
# n just below 2^31 (32-bit arithmetic) and just above (64-bit); first and last 512 lanes only
BELOW, ABOVE = (4, 10956549, 49), (8, 5478275, 49)
EDGE = 512
STRIDED = ((2, 3, 5, 5, 2), (1, 2, 6, 8, 2), (3, 1, 7, 4, 3), (2, 2, 1, 1, 2), (1, 1, 14, 14, 1), (2, 3, 4, 9, 4))


def _n(case):
    return case[0] * case[1] * case[2]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    path = tmp_path_factory.mktemp("bn_compact_index_" + request.param) / "bn_compact_index"
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + extra + ["-I" + os.path.join(PKG, "csrc"),
                                                                                os.path.join(ROOT, "tests", "bn_compact_index_main.cpp"), "-o", str(path)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(path)


def _run(exe, mode, args):
    r = subprocess.run([exe, mode] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr              # a sanitizer report ends the program with a non-zero status
    return r.stdout.splitlines()


def test_the_cases_are_what_they_claim():
    assert all(_n(c) % 4 == 0 for c in SMALL + (BELOW, ABOVE)) and _n(BELOW) < 2 ** 31 < _n(ABOVE)
    images = lambda case, t: [(4 * t + k) // (case[1] * case[2]) for k in range(4)]                     # noqa: E731
    assert any(len(set(images((4, 2, 9), t))) == 2 for t in range(18)) and images((8, 1, 1), 1) == [4, 5, 6, 7]
    assert images((4, 2, 1), 0) == [0, 0, 1, 1] and all(len(set(images((3, 5, 196), t))) == 1 for t in range(735))


def test_image_and_channel_major_index_of_every_lanes_elements(exe):
    ranges = [(case, 0, _n(case) // 4) for case in SMALL]
    for case in (BELOW, ABOVE):
        ranges += [(case, 0, EDGE), (case, _n(case) // 4 - EDGE, EDGE)]
    lines = _run(exe, "images", [v for (N, C, HW), first, count in ranges for v in (N, C, HW, first, count)])
    assert len(lines) == sum(count for _, _, count in ranges)
    it = iter(lines)
    for (N, C, HW), first, count in ranges:
        for t in range(first, first + count):
            got = [int(v) for v in next(it).split()]
            flat = [4 * t + k for k in range(4)]
            image = [e // (C * HW) for e in flat]
            twin = [(((e // HW) % C) * N + e // (C * HW)) * HW + e % HW for e in flat]
            assert got[0] == t and got[1:5] == image and got[5:9] == twin, ((N, C, HW), t, got, image, twin)


def test_the_channel_major_index_is_a_permutation(exe):
    N, C, HW = SMALL[1]
    lines = _run(exe, "images", [N, C, HW, 0, _n(SMALL[1]) // 4])
    seen = sorted(int(v) for line in lines for v in line.split()[5:9])
    assert seen == list(range(N * C * HW))


def test_a_strided_window_reads_the_positions_of_a_strided_slice(exe):
    lines = iter(_run(exe, "strided", [v for case in STRIDED for v in case]))
    for N, C, H, W, s in STRIDED:
        Ho, Wo = len(range(0, H, s)), len(range(0, W, s))
        assert [int(v) for v in next(lines).split()] == [Ho, Wo]
        want = [((n * C + c) * H + h) * W + w for c in range(C) for n in range(N) for h in range(0, H, s) for w in range(0, W, s)]
        got = [int(next(lines)) for _ in want]
        assert got == want and max(got) < N * C * H * W
    assert next(lines, None) is None
