"""ctypes binding of the C ABI libraries: lib/libxai_hip.so (include/xai_hip.h, frozen at ABI 1.11) and the extension libraries
lib/libxai_ext.so, libxai_ext2.so ... libxai_ext6.so (include/xai_hip_ext.h ... xai_hip_ext6.h), each holding the entry points
added after the header before it was frozen or pinned.  LIBRARIES lists them, one Library record each; OPEN_LIBRARIES lists, in the
same records, the library added since that table was pinned (lib/libxai_ext7.so, include/xai_hip_ext7.h) and LATER_LIBRARIES the ones
since that one was (lib/libxai_compact.so, include/xai_hip_compact.h); NEWER_LIBRARIES holds the one added after the count of those
three tables was pinned too (lib/libxai_slic.so, include/xai_hip_slic.h), and LATEST_LIBRARIES the one added after that table and
every_library() were pinned (lib/libxai_felz.so, include/xai_hip_felz.h); nothing else in Python does.

Each header is the one description of its ABI: the argument types, the return types and the two version numbers are read from
it at import (parse_header), nothing here repeats a prototype.  There is no CPU fallback: if a shared library is missing or a
tensor is not on a HIP device the call raises.  Build with `make -C image-classification-xai_amd/csrc`
(or `python -c "import __graft_entry__ as g; g.build()"`).
"""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(os.path.dirname(_HERE), "csrc")
_INCLUDE = os.path.normpath(os.path.join(_HERE, "..", "..", "include"))      # csrc/Makefile's -I../../include
ABI_DEFINES = ("XAI_ABI_VERSION", "XAI_ABI_MINOR")


class XaiHipError(RuntimeError):
    pass


_SCALAR = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
           "xai_stream_t": C.c_void_p}
_POINTER = re.compile(r"(const )?(float|double|void|int32_t|int64_t|uint64_t|uint8_t)\*( const\*)?")
_RETURN = {"int": C.c_int, "size_t": C.c_size_t, "const char*": C.c_char_p}
_PROTOTYPE = re.compile(r"(int|size_t|const char\*) (xai_[a-z0-9_]+)\(([^()]*)\)")
_LAUNCH = ("_f32", "_f64", "_i32", "_u64")            # the entries that launch: they return a code and end in the caller's stream


def parse_header(text, defines=ABI_DEFINES):
    """The text of include/xai_hip.h -> ({name: argtypes}, {name: restype}, (XAI_ABI_VERSION, XAI_ABI_MINOR)).  Strict: comments,
    preprocessor lines, the extern "C" braces and the stream typedef aside, every statement must be `<ret> xai_<name>(<params>)` in
    the types listed above; anything else raises XaiHipError quoting the statement, nothing gets a default type.
    `defines`: the names of the header's two version defines (a Library's `defines`)."""
    major_name, minor_name = defines
    found, body = {}, []
    for line in re.sub(r"/\*.*?\*/", " ", text, flags=re.S).splitlines():
        if line.rstrip().endswith("\\"):
            raise XaiHipError(f"continued line: {line.strip()!r}")
        if not line.lstrip().startswith("#"):
            body.append(line)
            continue
        m = re.fullmatch(rf"\s*#\s*define ({major_name}|{minor_name}) (\d+)\s*", line)
        if m:
            if m.group(1) in found:
                raise XaiHipError(f"defined twice: {line.strip()!r}")
            found[m.group(1)] = int(m.group(2))
    if len(found) != 2:
        raise XaiHipError(f"no `#define {major_name} <n>` and `#define {minor_name} <n>`")
    m = re.fullmatch(r'\s*extern "C" \{(.*)\}\s*', "\n".join(body), flags=re.S)
    if not m:
        raise XaiHipError('the declarations are not inside one `extern "C" { ... }`')
    *statements, rest = (" ".join(s.split()) for s in m.group(1).split(";"))
    if rest:
        raise XaiHipError(f"not a statement: {rest!r}")
    if statements.count("typedef void* xai_stream_t") != 1:
        raise XaiHipError("no single `typedef void* xai_stream_t;`")
    statements.remove("typedef void* xai_stream_t")
    argtypes, restypes = {}, {}
    for st in statements:
        m = _PROTOTYPE.fullmatch(st)
        if not m or m.group(2) in argtypes:
            raise XaiHipError(f"not a prototype this binding can read, or a second one of its name: {st!r}")
        ret, name, params = m.groups()
        types = []
        for p in ([] if params == "void" else params.split(",")):
            ctype, _, ident = p.strip().rpartition(" ")
            if not re.fullmatch(r"[A-Za-z_]\w*", ident) or not (ctype in _SCALAR or _POINTER.fullmatch(ctype)):
                raise XaiHipError(f"parameter {p.strip()!r} has no known type: {st!r}")
            types.append(ctype)
        streams = [i for i, t in enumerate(types) if t == "xai_stream_t"]
        launch = name.endswith(_LAUNCH)
        if streams != ([len(types) - 1] if launch else []) or launch and ret != "int":
            raise XaiHipError(f"a launch entry (*{', *'.join(_LAUNCH)}) returns int and takes the stream last, no other takes one: {st!r}")
        argtypes[name] = [_SCALAR.get(t, C.c_void_p) for t in types]      # not in _SCALAR: one of _POINTER's spellings, checked above
        restypes[name] = _RETURN[ret]
    return argtypes, restypes, (found[major_name], found[minor_name])


class Library:
    """One C ABI library: lib/libxai_<key>.so, the header that declares it, what parse_header read from that header at import
    (`signatures`: name -> argument types, `restypes`, and the `version`.`minor` its two defines give) and, once load() has
    accepted the file, its `handle`.  The record is the state: redirect `path` or raise `minor` here, nowhere else."""

    def __init__(self, key, header, defines):
        stem = "xai" if key == "hip" else f"xai_{key}"
        self.key = key
        self.path = os.path.join(_HERE, "lib", f"libxai_{key}.so")
        self.header_path = os.path.join(_INCLUDE, header)
        self.defines = defines
        self.version_entries = (f"{stem}_version", f"{stem}_version_minor")
        self.handle = None
        self.signatures, self.restypes, (self.version, self.minor) = self.read_header()

    def read_header(self):
        try:
            with open(self.header_path) as f:
                return parse_header(f.read(), self.defines)
        except (OSError, XaiHipError) as e:
            raise XaiHipError(f"{self.header_path}: the C ABI cannot be bound from its header: {e}") from e

    def load(self):
        """Load the library once: absent -> XaiHipError, the version pair first, then every prototype of the header
        (AttributeError if the .so is stale).  Never falls back, and a refused file is not cached."""
        if self.handle is not None:
            return self.handle
        if not os.path.exists(self.path):
            raise XaiHipError(f"{self.path} not found: the HIP extension is not built. Run `make -C {_CSRC}` (needs hipcc, "
                              "targets gfx950). There is deliberately no CPU fallback.")
        lib = C.CDLL(self.path)
        # version first, by the two symbols every build of the library has had or that say "older" by their absence
        major_entry, minor_entry = self.version_entries
        getattr(lib, major_entry).restype = C.c_int
        major, minor = getattr(lib, major_entry)(), 0
        if hasattr(lib, minor_entry):
            getattr(lib, minor_entry).restype = C.c_int
            minor = getattr(lib, minor_entry)()
        if major != self.version or minor < self.minor:
            raise XaiHipError(f"{self.path} has ABI {major}.{minor}, this package needs {self.version}.{self.minor} or a later minor "
                              f"(include/{os.path.basename(self.header_path)}); rebuild with `make -C {_CSRC}`")
        for name, argtypes in self.signatures.items():
            fn = getattr(lib, name)          # AttributeError if the .so is stale
            fn.argtypes = argtypes
            fn.restype = self.restypes[name]
        self.handle = lib
        return lib


# the one list of the libraries, in the order in which their headers were frozen; csrc/Makefile's LIBS is its build-side twin
LIBRARIES = {lib.key: lib for lib in (
    Library("hip", "xai_hip.h", ABI_DEFINES),
    Library("ext", "xai_hip_ext.h", ("XAI_EXT_VERSION", "XAI_EXT_MINOR")),
    Library("ext2", "xai_hip_ext2.h", ("XAI_EXT2_VERSION", "XAI_EXT2_MINOR")),
    Library("ext3", "xai_hip_ext3.h", ("XAI_EXT3_VERSION", "XAI_EXT3_MINOR")),
    Library("ext4", "xai_hip_ext4.h", ("XAI_EXT4_VERSION", "XAI_EXT4_MINOR")),
    Library("ext5", "xai_hip_ext5.h", ("XAI_EXT5_VERSION", "XAI_EXT5_MINOR")),
    Library("ext6", "xai_hip_ext6.h", ("XAI_EXT6_VERSION", "XAI_EXT6_MINOR")),
)}
# The libraries added after the table above was pinned to its seven keys by tests (tests/test_cpu_abi_libs.py), which a feature may
# not edit: the same records, the same loader.  A refactor that may touch those tests folds this table into LIBRARIES.
OPEN_LIBRARIES = {lib.key: lib for lib in (
    Library("ext7", "xai_hip_ext7.h", ("XAI_EXT7_VERSION", "XAI_EXT7_MINOR")),
)}
# ... and the libraries added after OPEN_LIBRARIES was pinned to its one key in turn (tests/test_cpu_kmeans.py): lib/libxai_compact.so,
# include/xai_hip_compact.h, the compact-layout BN/ReLU kernels.  No test names this table's keys, so the next library is a line here.
LATER_LIBRARIES = {lib.key: lib for lib in (
    Library("compact", "xai_hip_compact.h", ("XAI_COMPACT_VERSION", "XAI_COMPACT_MINOR")),
)}
# ... and the library added after the number of records in the three tables above was pinned (tests/test_cpu_compact_abi.py):
# lib/libxai_slic.so, include/xai_hip_slic.h, SLIC superpixels.  load() resolves it, every_library() lists it, all_libraries() stays
# the three tables.
NEWER_LIBRARIES = {lib.key: lib for lib in (
    Library("slic", "xai_hip_slic.h", ("XAI_SLIC_VERSION", "XAI_SLIC_MINOR")),
)}
# ... and the library added after NEWER_LIBRARIES was pinned to its one key and every_library() to the four tables
# (tests/test_cpu_slic.py): lib/libxai_felz.so, include/xai_hip_felz.h, Felzenszwalb segmentation.  load() resolves it and
# latest_libraries() lists it; no test pins this table's length, so the next library is a line here.
LATEST_LIBRARIES = {lib.key: lib for lib in (
    Library("felz", "xai_hip_felz.h", ("XAI_FELZ_VERSION", "XAI_FELZ_MINOR")),
)}
# the main library's fields under the names they have always had, for readers: aliases read at import, the record is the state
_HIP = LIBRARIES["hip"]
LIB_PATH, HEADER_PATH, SIGNATURES, ABI_VERSION, ABI_MINOR = _HIP.path, _HIP.header_path, _HIP.signatures, _HIP.version, _HIP.minor


def load(key="hip"):
    """The loaded handle of the record of `key` in LIBRARIES, OPEN_LIBRARIES, LATER_LIBRARIES, NEWER_LIBRARIES or LATEST_LIBRARIES
    (cached by the record); raises, never falls back, when the file is absent or refused."""
    return latest_libraries()[key].load()


def all_libraries():
    """Every Library record by key, the three tables in the order their headers were written."""
    return {**LIBRARIES, **OPEN_LIBRARIES, **LATER_LIBRARIES}


def every_library():
    """Every Library record by key, all four tables in the order their headers were written."""
    return {**all_libraries(), **NEWER_LIBRARIES}


def latest_libraries():
    """Every Library record by key, all five tables in the order their headers were written: what load() resolves."""
    return {**every_library(), **LATEST_LIBRARIES}


def check(code, what):
    if code != 0:
        msg = load().xai_strerror(code).decode()
        raise XaiHipError(f"{what} failed with code {code}: {msg}")
