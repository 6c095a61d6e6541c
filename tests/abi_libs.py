"""What the tests of the C ABI libraries share: the names a header declares, the names a built library exports, the built
file of a key of xai_engine._lib.LIBRARIES, and the version pairs the headers are frozen or pinned at.

The rule.  A new library is: its header under include/; one record in xai_engine._lib.LIBRARIES; the same key in csrc/Makefile's
LIBS with a SRCS_<key> line, plus a header override if its header is not xai_hip_<key>.h; and its literal pair appended to PINNED
below.  A feature's own test file holds only what is particular to its entries; it never asserts a complete list of keys or the
absence of its key from somewhere.  The completeness checks live in tests/test_cpu_abi_libs.py and read the tree."""
import os
import re
import subprocess

from conftest import PKG

# literal pins, not read from the code under test: a header that moves has to move this line too
PINNED = {"hip": (1, 11), "ext": (1, 0), "ext2": (1, 1), "ext3": (1, 0), "ext4": (1, 0), "ext5": (1, 0), "ext6": (1, 0), "ext7": (1, 0),
          "compact": (1, 0), "slic": (1, 0), "felz": (1, 0), "clip": (1, 0), "conv": (1, 0), "convw": (1, 0), "cattn": (1, 0), "csurg": (1, 0)}


def declared(header):
    """sorted names of the prototypes in the header at path `header`, comments dropped"""
    src = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(xai_[a-z0-9_]+)\s*\(", src)))


def exported(lib):
    """sorted xai_* names the shared library at path `lib` defines"""
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    return sorted(l.split()[-1] for l in out.splitlines() if " T " in l and l.split()[-1].startswith("xai_"))


def built(key):
    """the path of the library LIBRARIES[key], built first where it is absent"""
    from xai_engine import _lib
    path = _lib.LIBRARIES[key].path
    if not os.path.exists(path):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j8"], check=True)
    return path


def exported_elsewhere(key):
    """[(other key, name)] of every name the libraries other than `key` export, each of them exporting exactly its own
    header's table: what a feature's "my symbols are in no other library" check reads"""
    from xai_engine import _lib
    names = []
    for other, rec in _lib.LIBRARIES.items():
        if other != key:
            got = exported(built(other))
            assert got == sorted(rec.signatures), other
            names += [(other, n) for n in got]
    assert len({o for o, _ in names}) == len(_lib.LIBRARIES) - 1
    return names
