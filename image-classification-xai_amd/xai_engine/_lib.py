"""ctypes binding of the C ABI libraries.  LIBRARIES is the one table of them, a Library record per key: lib/libxai_<key>.so,
declared by include/xai_hip_<key>.h (or the header its record names) with the version defines XAI_<KEY>_VERSION and XAI_<KEY>_MINOR.
The main library, key "hip", is the one exception: include/xai_hip.h, XAI_ABI_VERSION and XAI_ABI_MINOR, frozen at ABI 1.11; new
entry points go into a library of their own.

The rule.  A new library is: its header under include/; one record in LIBRARIES; the same key in csrc/Makefile's LIBS with a
SRCS_<key> line, plus a header override there and a `header=` here if its header is not xai_hip_<key>.h; and its literal version pair
in tests/abi_libs.py's PINNED (cm2ib's is registered there by tests/test_cpu_m2ib.py at import).  A feature's own test file holds only what is particular to its entries; it never asserts a complete
list of keys or the absence of its key from somewhere.  The completeness checks live in tests/test_cpu_abi_libs.py and read the tree.

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
_LAUNCH = ("_f32", "_f64", "_i32", "_u64", "_f16")          # the entries that launch: they return a code and end in the caller's stream


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

    def __init__(self, key, header=None):
        stem = "xai" if key == "hip" else f"xai_{key}"
        self.key = key
        self.path = os.path.join(_HERE, "lib", f"libxai_{key}.so")
        self.header_path = os.path.join(_INCLUDE, header or ("xai_hip.h" if key == "hip" else f"xai_hip_{key}.h"))
        self.defines = ABI_DEFINES if key == "hip" else (f"XAI_{key.upper()}_VERSION", f"XAI_{key.upper()}_MINOR")
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


# the one list of the libraries, in the order in which their headers were written; csrc/Makefile's LIBS is its build-side twin.
# `header=`: the five whose header is include/xai_<key>.h (their sources are under csrc/clip/ and csrc/conv/).
LIBRARIES = {rec.key: rec for rec in (
    Library("hip"), Library("ext"), Library("ext2"), Library("ext3"), Library("ext4"), Library("ext5"), Library("ext6"), Library("ext7"),
    Library("compact"), Library("slic"), Library("felz"),
    Library("clip", header="xai_clip.h"), Library("conv", header="xai_conv.h"), Library("convw", header="xai_convw.h"),
    Library("cattn", header="xai_cattn.h"), Library("csurg", header="xai_csurg.h"), Library("cm2ib"))}
# the main library's fields under the names they have always had, for readers: aliases read at import, the record is the state
_HIP = LIBRARIES["hip"]
LIB_PATH, HEADER_PATH, SIGNATURES, ABI_VERSION, ABI_MINOR = _HIP.path, _HIP.header_path, _HIP.signatures, _HIP.version, _HIP.minor


def load(key="hip"):
    """The loaded handle of LIBRARIES[key] (cached by the record); raises, never falls back, when the file is absent or refused."""
    return LIBRARIES[key].load()


def check(code, what):
    if code != 0:
        msg = load().xai_strerror(code).decode()
        raise XaiHipError(f"{what} failed with code {code}: {msg}")
