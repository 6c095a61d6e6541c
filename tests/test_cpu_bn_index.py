"""csrc/xai_bn_index.h on the CPU: the lane-to-channel arithmetic of the flat 16-byte path of the fused BN/ReLU kernels and the
wrappers' three-way path choice.  The header is built alone by the host compiler (tests/bn_index_main.cpp: it needs nothing of
HIP), once plainly and once with -fsanitize=address,undefined -- that stand-alone program is the sanitizer run of this
arithmetic -- and both are asked the same cases.  The expected values are Python integers: the channel of flat element e is
(e // HW) % C."""
import os
import subprocess

import pytest

from conftest import PKG, ROOT

SCALAR, VEC4, FLAT4 = 0, 1, 2

# (N, C, HW): lanes that straddle channels (HW = 49), an image boundary (c wraps to 0), four channels in one lane (HW = 1),
# three (HW = 3), a vector-path shape, many groups
SMALL = ((4, 3, 49), (4, 2, 9), (2, 4, 1), (1, 8, 3), (3, 5, 196), (50, 16, 49))
# n = 2 147 483 604 (just below 2^31: 32-bit arithmetic) and 2 147 483 800 (just above: 64-bit); first and last 1024 lanes only
BELOW, ABOVE = (4, 10956549, 49), (8, 5478275, 49)
EDGE = 1024


def _n(case):
    return case[0] * case[1] * case[2]


def _ranges():
    out = [(case, 0, _n(case) // 4) for case in SMALL]
    for case in (BELOW, ABOVE):
        out += [(case, 0, EDGE), (case, _n(case) // 4 - EDGE, EDGE)]
    return out


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    path = tmp_path_factory.mktemp("bn_index_" + request.param) / "bn_index"
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + extra + ["-I" + os.path.join(PKG, "csrc"),
                                                                                os.path.join(ROOT, "tests", "bn_index_main.cpp"), "-o", str(path)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(path)


def _run(exe, mode, args):
    r = subprocess.run([exe, mode] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr              # a sanitizer report ends the program with a non-zero status
    return r.stdout.splitlines()


def test_the_cases_are_what_they_claim():
    assert all(_n(c) % 4 == 0 for c in SMALL + (BELOW, ABOVE))
    assert _n(BELOW) < 2 ** 31 < _n(ABOVE) and 2 ** 31 - _n(BELOW) < 64 and _n(ABOVE) - 2 ** 31 < 256
    assert 4 * (_n(ABOVE) // 4 - 1) > 2 ** 31                                     # the last lanes of ABOVE start past 2^31


def test_every_lanes_channels_are_those_of_its_flat_elements(exe):
    ranges = _ranges()
    lines = _run(exe, "lanes", [v for (N, C, HW), first, count in ranges for v in (N, C, HW, first, count)])
    assert len(lines) == sum(count for _, _, count in ranges)
    it = iter(lines)
    for (N, C, HW), first, count in ranges:
        for t in range(first, first + count):
            got = [int(v) for v in next(it).split()]
            want = [((4 * t + k) // HW) % C for k in range(4)]
            assert got[0] == t and got[1:5] == want, ((N, C, HW), t, got, want)
            assert got[5:9] == (want if HW >= 4 else [-1] * 4), ((N, C, HW), t, got, want)


def test_the_cases_hold_straddling_wrapping_and_four_channel_lanes():
    def channels(case, t):
        return [((4 * t + k) // case[2]) % case[1] for k in range(4)]
    assert any(len(set(channels((4, 3, 49), t))) == 2 for t in range(147))
    assert any(channels((4, 2, 9), t)[0] == 1 and channels((4, 2, 9), t)[3] == 0 for t in range(18))      # into the next image
    assert channels((2, 4, 1), 0) == [0, 1, 2, 3] and len(set(channels((1, 8, 3), 2))) == 2
    assert all(len(set(channels((3, 5, 196), t))) == 1 for t in range(735))


def _want_path(n, HW, low):
    if n % 4 or low % 16:
        return SCALAR
    return VEC4 if HW % 4 == 0 else FLAT4


def test_the_three_way_path_choice(exe):
    # n % 4 in {0, 1, 2, 3}, HW % 4 in {0, 1}, all pointers aligned or one off by 4 bytes (its low bits reach the OR)
    cases = [(n, HW, low) for n in (39200, 39201, 39202, 39203, 2 ** 31 + 4, 2 ** 31 + 5) for HW in (196, 49) for low in (0x7F00, 0x7F04, 0x7F10, 0x7F08)]
    got = [int(v) for v in _run(exe, "path", [v for c in cases for v in c])]
    assert got == [_want_path(*c) for c in cases]
    by_case = dict(zip(cases, got))
    assert by_case[(39200, 196, 0x7F00)] == VEC4 and by_case[(39200, 49, 0x7F00)] == FLAT4 and by_case[(39200, 49, 0x7F10)] == FLAT4
    assert by_case[(39200, 49, 0x7F04)] == SCALAR and by_case[(39200, 196, 0x7F04)] == SCALAR and by_case[(39200, 49, 0x7F08)] == SCALAR
    assert all(by_case[(n, HW, 0x7F00)] == SCALAR for n in (39201, 39202, 39203) for HW in (196, 49))
    assert by_case[(2 ** 31 + 4, 49, 0x7F00)] == FLAT4
