"""MDA without a GPU: the restatement (tests/mda_restated.py) against the reference's own run (tests/golden/mda.npz), the
host step plan against a transcription of the reference's loop bounds, the signatures, the mirrored module, every argument
check, and the second extension library (include/xai_hip_ext2.h bound by the strict header reader, its exports, its version
pair, the kernels' argument checks made before any HIP call)."""
import ctypes as C
import inspect
import json
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

import mda_restated as R
from abi_libs import built, declared, exported, exported_elsewhere
from conftest import BAR, GOLDEN, PKG, ROOT, check, load_golden

EXT2_HEADER = os.path.join(ROOT, "include", "xai_hip_ext2.h")
_p, _i, _l, _f = C.c_void_p, C.c_int, C.c_int64, C.c_float
CASES = sorted(R.CASES)


# ------------------------------------------------------------------------------------------------ the restatement vs the reference
def test_fixture_holds_every_kind_of_case_and_every_case_is_well_conditioned():
    g = load_golden("mda.npz")
    kinds = set()
    for tag in CASES:
        S = len(g[f"{tag}_order_a"])
        L = R.subsearch_len(S)
        wm_ins, wm_del, sm, batch_diff, factor = g[f"{tag}_cond"]
        assert factor == 100 and min(wm_ins, wm_del, sm) >= factor * batch_diff, tag
        stopped, slot = int(g[f"{tag}_stopped"]), int(g[f"{tag}_cutoff_slot"])
        steps = int((g[f"{tag}_order_a"] >= 0).sum())
        kinds.add("never" if not stopped else ("phase1" if steps <= S - L else "phase2"))
        if stopped and steps > S - L:
            assert slot == steps - 1 - (S - L) and slot != steps - 1, tag          # the phase-local slot, not the slot just filled
        kinds.add(("grid", "irregular")[S == 17])
        kinds.add("ordered" if R.CASES[tag][-1] else "unordered")
    assert kinds == {"never", "phase1", "phase2", "grid", "irregular", "ordered", "unordered"}
    assert R.subsearch_len(17) == 8 < 17


@pytest.fixture(scope="module")
def restated():
    """every case once, grouped as the reference groups its passes"""
    out = {}
    for tag in CASES:
        c = R.seeded_case(tag)
        log = {}
        maps = R.MDA(c["trans_img"], c["input_tensor"], c["saliency_map"], c["patch_count"], c["blur"], c["model"], "cpu", c["img_hw"],
                     max_batch_size=5, ordered=c["ordered"], vis=True, segments=c["segments"], log=log)
        out[tag] = (c, maps, log)
    return out


@pytest.mark.parametrize("tag", CASES)
def test_restatement_reproduces_the_references_searches_and_maps(restated, tag):
    g = load_golden("mda.npz")
    c, maps, log = restated[tag]
    S = c["patch_count"]
    # orders, end_index and the slot of every write: equal
    assert np.array_equal(np.asarray(log["order_a"]), g[f"{tag}_order_a"])
    assert log["end_index"] == int(g[f"{tag}_end_index"])
    assert np.array_equal(log["best_segment_list"].numpy(), g[f"{tag}_best"])
    written = np.zeros(len(g[f"{tag}_MR_ins"]), bool)
    if int(g[f"{tag}_stopped"]):
        written[log["insertion"]["slots"]] = True
        written[log["insertion"]["cutoff_slot"]] = True
        assert log["insertion"]["cutoff_slot"] == int(g[f"{tag}_cutoff_slot"])
    else:
        written[:] = True
        assert "cutoff_slot" not in log["insertion"]
    assert np.array_equal(written, g[f"{tag}_MR_written"])
    # responses and maps: the parity contract
    mr = np.where(written, np.asarray(log["MR_ins"], np.float64), 0.0)
    check(f"mda/{tag}/MR_ins", mr, g[f"{tag}_MR_ins"], BAR)
    check(f"mda/{tag}/del_raw", log["deletion"]["raw_deletion"], g[f"{tag}_del_raw"], BAR)
    check(f"mda/{tag}/del_curve", log["deletion"]["final_curve"], g[f"{tag}_del_curve"], BAR, absolute=True)
    flat = c["segments"].flatten().numpy()
    for name, m in (("g0", maps[0]), ("g10", maps[4])):
        vals = np.array([m[:, :, 0].reshape(-1)[flat == s][0] for s in range(S)])
        check(f"mda/{tag}/{name}", vals, g[f"{tag}_{name}"], BAR)
        assert m.shape == (c["img_hw"], c["img_hw"], 3) and m.dtype == np.float32


def test_one_pass_of_L_rows_selects_what_the_references_batches_select(restated):
    tag = "vor17_p2"
    c, _, log5 = restated[tag]
    logL = {}
    R.MDA(c["trans_img"], c["input_tensor"], c["saliency_map"], c["patch_count"], c["blur"], c["model"], "cpu", c["img_hw"],
          max_batch_size=5, vis=True, segments=c["segments"], pass_rows=R.subsearch_len(c["patch_count"]), log=logL)
    assert torch.equal(torch.as_tensor(logL["order_a"]), torch.as_tensor(log5["order_a"]))
    assert torch.equal(logL["best_segment_list"], log5["best_segment_list"]) and logL["end_index"] == log5["end_index"]


# ------------------------------------------------------------------------------------------------ the step plan
@pytest.mark.parametrize("S", [2, 3, 4, 5, 9, 16, 17, 49, 196, 900])
def test_step_plan_is_the_references_loop_bounds(S):
    from xai_engine import mda
    L = R.subsearch_len(S)
    assert mda.subsearch_len(S) == L == min(2 * int(np.sqrt(S)), 28)
    assert mda.step_plan(S, S, 0, True) == R.reference_step_plan(S, S, 0, True)
    plan = mda.step_plan(S, S, 0, True)
    assert len(plan) == S and sorted(p[0] for p in plan) == list(range(S))
    assert [p[2] for p in plan[S - L:]] == list(range(L))                          # the phase-local cutoff slot
    for input_length in sorted({0, 1, L, S - L, S - 1, S}):
        got = mda.step_plan(S, S, input_length, False)
        assert got == R.reference_step_plan(S, S, input_length, False), (S, input_length)
        assert len(got) == S - input_length and all(c == -1 for _, _, c in got)
        assert sorted(p[0] for p in got) == list(range(S - input_length))          # the pre-loaded tail is never a slot
        assert all(1 <= n <= L for _, n, _ in got)
    assert S - 1 > S - L or L == 1                                                  # the cases above include input_length > n_searches - L


def test_one_segment_raises_because_the_sub_search_is_wider_than_the_map():
    from xai_engine import mda
    assert R.subsearch_len(1) == 2
    with pytest.raises(ValueError, match="sub-search width of 2"):
        mda.check_segments(torch.zeros((4, 4), dtype=torch.int64), 1, "MDA")


# ------------------------------------------------------------------------------------------------ signatures and the mirrored module
def test_signatures_are_the_references_plus_segments():
    from xai_engine import mda
    api = json.load(open(os.path.join(GOLDEN, "mda_api.json")))
    for name in ("normalize_curve", "find_insertion_patches", "find_deletion_patches", "MDA"):
        params = list(inspect.signature(getattr(mda, name)).parameters.values())
        got = [{"name": p.name, "has_default": p.default is not inspect.Parameter.empty,
                "default": None if p.default is inspect.Parameter.empty else p.default} for p in params]
        want = api[name] + ([{"name": "segments", "has_default": True, "default": None}] if name == "MDA" else [])
        assert got == want, name
    assert "test_kappa" in inspect.signature(mda.find_deletion_patches).parameters


SHIM = textwrap.dedent("""
    import sys
    sys.path.insert(0, sys.argv[2]); sys.path.insert(0, sys.argv[1])
    from util.attribution_methods import MDAFunctions
    import xai_engine.mda as m
    assert MDAFunctions.MDA is m.MDA and MDAFunctions.find_insertion_patches is m.find_insertion_patches
    assert MDAFunctions.find_deletion_patches is m.find_deletion_patches and MDAFunctions.normalize_curve is m.normalize_curve
    assert MDAFunctions.WHO == "sibling" and MDAFunctions.something_else() == "sibling fn"
    try:
        MDAFunctions.not_there
    except AttributeError as e:
        assert "not_there" in str(e)
    else:
        raise SystemExit("no AttributeError")
    print("shim ok")
""")


def test_mirrored_module_serves_the_four_names_and_falls_through_for_the_rest(tmp_path):
    d = tmp_path / "site" / "util" / "attribution_methods"
    d.mkdir(parents=True)
    (tmp_path / "site" / "util" / "__init__.py").write_text("")
    (d / "__init__.py").write_text("")
    (d / "MDAFunctions.py").write_text("WHO = 'sibling'\ndef something_else(): return 'sibling fn'\ndef MDA(): return 'sibling MDA'\n")
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    r = subprocess.run([sys.executable, "-c", SHIM, PKG, str(tmp_path / "site")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "shim ok" in r.stdout, r.stdout + r.stderr


def test_the_harness_row_and_the_cli_know_mda_and_the_dispatch_tuple_does_not():
    from xai_engine.sweep import VIT_ATTR_FUNCS, VIT_TRANS_ATTR_FUNCS
    from xai_engine.evaluate_perturbation import build_parser
    assert VIT_TRANS_ATTR_FUNCS == ("MDA",) and "MDA" not in VIT_ATTR_FUNCS and len(VIT_ATTR_FUNCS) == 10
    assert "MDA}" in build_parser().format_help().replace("\n", "").replace(" ", "")


# ------------------------------------------------------------------------------------------------ argument checks
class _FakeCuda(torch.Tensor):
    is_cuda = True


def test_every_argument_check_comes_before_any_device_work(capsys):
    from xai_engine import XaiHipError, mda
    net = R.SmallNet(1).eval()
    x, sal = torch.zeros(1, 3, 8, 8), torch.ones(8, 8, 3)
    seg = R.grid_labels(8, 2)
    blur = R.box_blur(3)
    clip = {"prediction_function": None}
    with pytest.raises(NotImplementedError, match="CLIP"):
        mda.MDA(x, x, sal.numpy(), 4, blur, net, "cuda:0", 8, CLIP_test_info=clip, segments=seg)
    with pytest.raises(NotImplementedError, match="CLIP"):
        mda.find_insertion_patches(x, sal, seg, blur, 4, 1, net, "cuda:0", 8, CLIP_test_info=clip)
    with pytest.raises(NotImplementedError, match="CLIP"):
        mda.find_deletion_patches(x, seg, sal, torch.tensor([0]), blur, 4, net, "cuda:0", 8, CLIP_test_info=clip)
    with pytest.raises(XaiHipError, match="not a HIP GPU"):
        mda.find_insertion_patches(x, sal, seg, blur, 4, 1, net, "cpu", 8)
    gaps = seg.clone()
    gaps[gaps == 3] = 5
    for fn in (lambda s, n: mda.find_insertion_patches(x, sal, s, blur, n, 1, net, "cuda:0", 8),
               lambda s, n: mda.find_deletion_patches(x, s, sal, torch.tensor([0]), blur, n, net, "cuda:0", 8)):
        with pytest.raises(ValueError, match="without gaps"):
            fn(gaps, 4)
        with pytest.raises(ValueError, match="without gaps"):
            fn(seg + 1, 4)
        for n in (3, 5):
            with pytest.raises(ValueError, match=rf"n_searches = {n} but the label map has 4 segments"):
                fn(seg, n)
        with pytest.raises(ValueError, match="integer labels"):
            fn(seg.float(), 4)
    with pytest.raises(ValueError, match="type 0"):
        mda.find_insertion_patches(x, sal, seg, blur, 4, 0, net, "cuda:0", 8)
    assert mda.find_insertion_patches(x, sal, seg, blur, 4, 1, net, "cuda:0", 8, cutoff=0)[2].numel() == 0       # :40-41
    # batch_size > n_steps (:47-49, :318-320): the reference's check, message and 0 are kept, and no S >= 1 can reach them --
    # batch_size is min(S, max_batch_size) below 50 segments and min(25, max_batch_size) from there on
    assert all(mda._batch_size_ok(S, m) for S in (1, 2, 4, 16, 49, 50, 196, 900) for m in (1, 5, 25, 1000))
    assert capsys.readouterr().out == ""


def test_without_skimage_and_without_segments_the_error_names_the_argument():
    from xai_engine import mda
    try:
        import skimage  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="segments="):
            mda.MDA(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8), np.ones((8, 8, 3), np.float32), 4, R.box_blur(3), R.SmallNet(1), "cuda:0", 8)
    else:
        assert callable(mda.slic_segments)


def test_end_index_is_the_first_response_at_or_above_090_else_the_length():
    from xai_engine import mda
    for arr, want in (([0.1, 0.9, 0.95], 1), ([0.1, 0.2], 2), ([0.95], 0), ([], 0)):
        assert mda.end_index_of(torch.tensor(arr)) == R.end_index_of(torch.tensor(arr)) == want
    assert mda.end_index_of(np.array([0.0, 0.5, 1.0])) == 2


# ------------------------------------------------------------------------------------------------ the second extension library
def test_ext2_header_parses_with_the_strict_reader_and_the_table_equals_the_parse():
    from xai_engine import _lib
    rec = _lib.LIBRARIES["ext2"]
    assert os.path.samefile(rec.header_path, EXT2_HEADER)
    text = open(EXT2_HEADER).read()
    args, ret, version = _lib.parse_header(text, rec.defines)
    assert args == rec.signatures and sorted(args) == declared(EXT2_HEADER)
    assert version == (rec.version, rec.minor)
    # the pair is read from the header, whatever it has grown to
    assert rec.version == int(re.search(r"^#define XAI_EXT2_VERSION (\d+)$", text, flags=re.M).group(1))
    assert rec.minor == int(re.search(r"^#define XAI_EXT2_MINOR (\d+)$", text, flags=re.M).group(1))
    assert args["xai_ext2_version"] == [] and args["xai_ext2_version_minor"] == [] and args["xai_mda_max_segments"] == []
    assert args["xai_mda_compose_f32"] == [_p, _p, _p, _p, _i, _i, _i, _l, _p, _p]
    assert args["xai_mda_select_f32"] == [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _f, _p, _p, _p, _p, _p, _p]
    assert args["xai_mda_commit_f32"] == [_p, _p, _p, _i, _i, _l, _p, _p]
    assert all(t is _i for t in ret.values())
    # the three headers do not share a name
    assert not set(args) & set(_lib.SIGNATURES) and not set(args) & set(_lib.LIBRARIES["ext"].signatures)
    # every MDA launch entry cites the lines of MDAFunctions.py it replaces (a later feature's entries cite their own source)
    for name in args:
        if name.startswith("xai_mda_") and name.endswith(("_f32", "_f64", "_i32", "_u64")):
            at = text.index(name + "(")
            comment = text[text.rfind("/*", 0, at):at]
            assert re.search(r"replaces\s+MDAFunctions\.py:\d+", comment), name
    with pytest.raises(_lib.XaiHipError, match="XAI_EXT2_MINOR"):
        _lib.parse_header(open(_lib.LIBRARIES["ext"].header_path).read(), rec.defines)


def test_ext2_library_exports_exactly_its_header_and_the_other_two_are_untouched():
    from xai_engine import _lib
    assert exported(built("ext2")) == declared(EXT2_HEADER) == sorted(_lib.LIBRARIES["ext2"].signatures)
    assert not [(o, n) for o, n in exported_elsewhere("ext2") if "mda" in n or "ext2" in n]
    lib = _lib.load("ext2")
    assert lib.xai_mda_max_segments() >= 1024 and lib.xai_mda_max_width() >= 28


def test_the_three_kernels_check_their_arguments_without_a_gpu():
    from xai_engine import _lib
    built("ext2")
    lib = _lib.load("ext2")
    cap = lib.xai_mda_max_segments()
    p = 16                               # a non-NULL pointer that is never dereferenced: validation comes first

    def compose(start=p, finish=p, seg=p, cand=p, out=p, n=1, L=8, Cc=3, HW=49):
        return lib.xai_mda_compose_f32(start, finish, seg, cand, n, L, Cc, HW, out, None)
    assert [compose(**{k: None}) for k in ("start", "finish", "seg", "cand", "out")] == [-1] * 5
    assert compose(n=0) == -2 and compose(L=0) == -2 and compose(Cc=0) == -2 and compose(HW=0) == -2

    def select(resp=p, order=p, plan=p, ref=p, mr=p, chosen=p, taken=p, cand=p, state=p, n=1, S=17, L=8, stride=17, mode=1, stop=1):
        return lib.xai_mda_select_f32(resp, order, plan, ref, n, S, L, stride, mode, stop, 0.9, mr, chosen, taken, cand, state, None)
    assert [select(**{k: None}) for k in ("resp", "order", "plan", "ref", "mr", "chosen", "taken", "cand", "state")] == [-1] * 9
    assert select(n=0) == -2 and select(S=0) == -2 and select(L=0) == -2 and select(stride=0) == -2 and select(mode=2) == -2
    assert select(S=cap + 1) == -3 and select(L=lib.xai_mda_max_width() + 1) == -3          # XAI_E_UNSUPPORTED

    def commit(finish=p, seg=p, state=p, start=p, n=1, Cc=3, HW=49):
        return lib.xai_mda_commit_f32(finish, seg, state, n, Cc, HW, start, None)
    assert [commit(**{k: None}) for k in ("finish", "seg", "state", "start")] == [-1] * 4
    assert commit(n=0) == -2 and commit(Cc=0) == -2 and commit(HW=0) == -2
    assert b"NULL" in _lib.load().xai_strerror(compose(start=None))
