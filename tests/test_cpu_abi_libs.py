"""The C ABI libraries as one table (xai_engine._lib.LIBRARIES): every test here runs for every key of it, the main library
included.  What a library exports against its header and its pinned version pair, what the loaded handle carries, what the loader
and the header reader refuse, and that build() checks them all.  What is particular to one feature's entries (literal argtypes,
the lines a header cites, the argument checks of its kernels) is in that feature's own test file."""
import ctypes as C
import glob
import os
import re
import subprocess

import pytest

from abi_libs import PINNED, built, declared, exported
from conftest import PKG, ROOT
from xai_engine import _lib

KEYS = list(_lib.LIBRARIES)
ELEVEN = ["hip", "ext", "ext2", "ext3", "ext4", "ext5", "ext6", "ext7", "compact", "slic", "felz"]
SIXTEEN = ELEVEN + ["clip", "conv", "convw", "cattn", "csurg"]
# the file name of each header, literally: the eleven by the rule xai_hip[_<key>].h, the five after them by name
HEADERS = dict({key: "xai_hip.h" if key == "hip" else f"xai_hip_{key}.h" for key in ELEVEN},
               clip="xai_clip.h", conv="xai_conv.h", convw="xai_convw.h", cattn="xai_cattn.h", csurg="xai_csurg.h")
_p, _i = C.c_void_p, C.c_int


@pytest.fixture(scope="module")
def L():
    return _lib


def pin(rec):
    """the literal pair of tests/abi_libs.py: a key without one fails, the record under test is never its own pin"""
    return PINNED[rec.key]


def test_the_table_begins_with_the_sixteen_libraries_and_the_old_names_are_aliases_of_the_main_record(L):
    """The table begins with these sixteen keys in this order; keys after them are allowed.  "And no other key" is given up on
    purpose: it made every new library a new table beside this one.  What holds the table to the tree instead is the closure
    test below, which grows with the tree: the headers, the Makefile's LIBS and the kernel files must all say the same keys."""
    import xai_engine
    assert KEYS[:16] == SIXTEEN and set(PINNED) <= set(KEYS)
    for key, rec in L.LIBRARIES.items():
        header = HEADERS.get(key, f"xai_hip_{key}.h")
        stem = "xai" if key == "hip" else f"xai_{key}"
        assert isinstance(rec, L.Library) and rec.key == key and os.path.basename(rec.path) == f"libxai_{key}.so"
        assert os.path.dirname(rec.path) == os.path.join(os.path.dirname(os.path.abspath(L.__file__)), "lib")
        assert os.path.samefile(rec.header_path, os.path.join(ROOT, "include", header))
        assert rec.version_entries == (f"{stem}_version", f"{stem}_version_minor") and set(rec.version_entries) <= set(rec.signatures)
        assert rec.defines == (("XAI_ABI_VERSION", "XAI_ABI_MINOR") if key == "hip" else (f"XAI_{key.upper()}_VERSION", f"XAI_{key.upper()}_MINOR"))
    hip = L.LIBRARIES["hip"]
    assert (L.LIB_PATH, L.HEADER_PATH, L.ABI_VERSION, L.ABI_MINOR, L.ABI_DEFINES) == (hip.path, hip.header_path, hip.version, hip.minor, hip.defines)
    assert L.SIGNATURES is hip.signatures and xai_engine.LIB_PATH == hip.path and xai_engine.load_library is L.load
    with pytest.raises(KeyError):
        L.load("ext8")


def test_the_table_the_headers_the_makefile_and_the_kernel_files_name_the_same_libraries(L):
    """(a) include/*.h is exactly the records' headers, one record each, (b) LIBS as make reads it is the table's keys in order and
    the SRCS_* variables are one per key, (c) every .hip under csrc/ outside csrc/tune/ is in exactly one SRCS_<key> and every file
    a SRCS_<key> names exists, (d) `all` builds exactly the records' library files and `clean` removes $(OUTS)"""
    csrc = os.path.join(PKG, "csrc")
    headers = glob.glob(os.path.join(ROOT, "include", "*.h"))
    assert sorted(map(os.path.realpath, headers)) == sorted(os.path.realpath(rec.header_path) for rec in L.LIBRARIES.values())
    assert len(headers) == len(KEYS)
    db = subprocess.run(["make", "-C", csrc, "-pnq"], capture_output=True, text=True).stdout      # the database, nothing is run
    make = dict(re.findall(r"^(LIBS|SRCS_\w+) :?= (.*)$", db, flags=re.M))
    assert make["LIBS"].split() == KEYS and set(make) == {"LIBS"} | {f"SRCS_{key}" for key in KEYS}
    listed = sorted(f for key in KEYS for f in make[f"SRCS_{key}"].split())
    found = glob.glob(os.path.join(csrc, "**", "*.hip"), recursive=True)
    assert listed == sorted(f for f in (os.path.relpath(f, csrc) for f in found) if not f.startswith("tune" + os.sep))
    assert len(listed) == len(set(listed)) and all(os.path.isfile(os.path.join(csrc, f)) for f in listed)
    goal = re.search(r"^all:(.*)$", db, flags=re.M).group(1).split()
    assert len(goal) == len(KEYS)
    assert sorted(os.path.realpath(os.path.join(csrc, f)) for f in goal) == sorted(os.path.realpath(rec.path) for rec in L.LIBRARIES.values())
    clean = re.search(r"^clean:\n(?:#.*\n)*((?:\t.*\n)+)", db, flags=re.M).group(1)
    assert clean == "\trm -rf build $(OUTS)\n" and re.search(r"^OUTS := (.*)$", db, flags=re.M).group(1).split() == goal


@pytest.mark.parametrize("key", KEYS)
def test_library_exports_exactly_its_header_at_the_pinned_version(L, key):
    rec = L.LIBRARIES[key]
    assert exported(built(key)) == declared(rec.header_path) == sorted(rec.signatures)
    text = open(rec.header_path).read()
    major, minor = (int(re.search(rf"^#define {d} (\d+)$", text, flags=re.M).group(1)) for d in rec.defines)
    assert (rec.version, rec.minor) == pin(rec) == (major, minor)
    assert L.parse_header(text, rec.defines) == (rec.signatures, rec.restypes, pin(rec))      # the table is the parse, nothing else
    assert all(rec.signatures[e] == [] and rec.restypes[e] is _i for e in rec.version_entries)
    if key == "hip":
        assert len(rec.signatures) == 64
    for other in KEYS:                                                                         # no name is declared by two headers
        assert other == key or not set(rec.signatures) & set(L.LIBRARIES[other].signatures), other


@pytest.mark.parametrize("key", KEYS)
def test_loaded_handle_is_cached_reports_the_headers_pair_and_carries_the_headers_types(L, key):
    rec = L.LIBRARIES[key]
    built(key)
    lib = L.load(key)
    assert lib is L.load(key) is rec.load() is rec.handle
    assert tuple(getattr(lib, e)() for e in rec.version_entries) == (rec.version, rec.minor) == pin(rec)
    for name, types in rec.signatures.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == types and fn.restype is rec.restypes[name], name


@pytest.mark.parametrize("key", KEYS)
def test_loader_refuses_an_absent_an_older_and_a_stale_library_and_caches_none_of_them(L, key, monkeypatch, tmp_path):
    rec = L.LIBRARIES[key]
    real = built(key)
    a, b = pin(rec)
    monkeypatch.setattr(rec, "handle", None)
    monkeypatch.setattr(rec, "path", str(tmp_path / f"libxai_{key}.so"))
    with pytest.raises(L.XaiHipError, match="not found") as e:
        L.load(key)
    assert "make -C" in str(e.value) and str(e.value).startswith(rec.path) and rec.handle is None
    monkeypatch.setattr(rec, "path", real)
    monkeypatch.setattr(rec, "minor", b + 1)                              # the package wants a later minor than the library has
    with pytest.raises(L.XaiHipError, match=rf"has ABI {a}\.{b}, this package needs {a}\.{b + 1}") as e:
        L.load(key)
    assert f"(include/{os.path.basename(rec.header_path)})" in str(e.value) and rec.handle is None
    monkeypatch.setattr(rec, "minor", b)
    monkeypatch.setattr(rec, "version", a + 1)                            # or another major
    with pytest.raises(L.XaiHipError, match=rf"has ABI {a}\.{b}, this package needs {a + 1}\.{b}"):
        L.load(key)
    assert rec.handle is None
    monkeypatch.setattr(rec, "version", a)
    monkeypatch.setitem(rec.signatures, "xai_not_in_the_library_f32", [_p])  # a header ahead of the .so: stale
    monkeypatch.setitem(rec.restypes, "xai_not_in_the_library_f32", _i)
    with pytest.raises(AttributeError):
        L.load(key)
    assert rec.handle is None
    monkeypatch.undo()
    assert "xai_not_in_the_library_f32" not in rec.signatures and (rec.path, rec.version, rec.minor) == (real, a, b)
    assert L.load(key) is not None and rec.handle is L.load(key)          # and the real library loads again


@pytest.mark.parametrize("key", KEYS)
def test_an_absent_or_broken_header_is_an_error_that_names_the_path(L, key, monkeypatch, tmp_path):
    rec = L.LIBRARIES[key]
    hdr = open(rec.header_path).read()
    entry = f"int {rec.version_entries[0]}(void);"
    assert hdr.count(entry) == 1
    assert rec.read_header() == (rec.signatures, rec.restypes, (rec.version, rec.minor))       # read once at import, from header_path
    for name, text in ((f"absent_{key}.h", None), (f"broken_{key}.h", hdr.replace(entry, "long" + entry[3:]))):
        path = tmp_path / name
        if text is not None:
            path.write_text(text)
        monkeypatch.setattr(rec, "header_path", str(path))
        with pytest.raises(L.XaiHipError, match=name):
            rec.read_header()


@pytest.mark.parametrize("key", KEYS)
def test_a_header_asked_for_another_librarys_define_pair_is_refused_by_the_name_of_the_define(L, key):
    text = open(L.LIBRARIES[key].header_path).read()
    for other in KEYS:
        if other != key:
            with pytest.raises(L.XaiHipError, match=rf"`#define {L.LIBRARIES[other].defines[1]} <n>`"):      # the pair asked for is the pair required
                L.parse_header(text, L.LIBRARIES[other].defines)


@pytest.mark.parametrize("key", KEYS)
def test_build_version_checks_every_library(L, key, monkeypatch):
    """build() itself (its `make` stubbed: the libraries are built), with one record asking for a later minor than the built
    library has: it must not get past that library"""
    import __graft_entry__ as g
    rec = L.LIBRARIES[key]
    real = built(key)
    a, b = pin(rec)
    made = []
    monkeypatch.setattr(g.subprocess, "run", lambda cmd, **kw: made.append((cmd, kw)))
    monkeypatch.setattr(rec, "handle", None)
    monkeypatch.setattr(rec, "minor", b + 1)
    with pytest.raises(L.XaiHipError, match=rf"{re.escape(real)} has ABI {a}\.{b}, this package needs {a}\.{b + 1}"):
        g.build()
    assert rec.handle is None and [cmd[:2] for cmd, _ in made] == [["make", "-C"]] and made[0][1] == {"check": True}


def test_build_passes_on_the_built_tree_and_imports_the_feature_modules(L, monkeypatch):
    import sys
    import __graft_entry__ as g
    for key in KEYS:
        built(key)
    monkeypatch.setattr(g.subprocess, "run", lambda cmd, **kw: None)
    g.build()
    assert all(rec.handle is not None for rec in L.LIBRARIES.values())
    assert all(f"xai_engine.{m}" in sys.modules for m in ("segeval", "lrp", "quickshift", "linkage", "kmeans", "slic", "felzenszwalb",
                                                            "eclip", "clip_attn", "surgery"))
