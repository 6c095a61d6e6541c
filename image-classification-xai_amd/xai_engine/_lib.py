"""ctypes binding of libxai_hip.so (C ABI: include/xai_hip.h) and of the extension libraries libxai_ext.so
(include/xai_hip_ext.h: the entry points added after xai_hip.h was frozen at ABI 1.11) and libxai_ext2.so
(include/xai_hip_ext2.h: the ones added after xai_hip_ext.h was frozen too) and libxai_ext3.so (include/xai_hip_ext3.h: the ones
added after xai_hip_ext2.h was pinned at 1.1) and libxai_ext4.so (include/xai_hip_ext4.h: the ones added after xai_hip_ext3.h was pinned
at 1.0) and libxai_ext5.so (include/xai_hip_ext5.h: the ones added after xai_hip_ext4.h was pinned at 1.0) and libxai_ext6.so
(include/xai_hip_ext6.h: the ones added after xai_hip_ext5.h was pinned at 1.0).

Each header is the one description of its ABI: the argument types, the return types and the two version numbers below are read
from it at import (parse_header), nothing here repeats a prototype.  There is no CPU fallback: if a shared library is missing
or a tensor is not on a HIP device the call raises.  Build with `make -C image-classification-xai_amd/csrc`
(or `python -c "import __graft_entry__ as g; g.build()"`).
"""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libxai_hip.so")
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "xai_hip.h"))     # csrc/Makefile's -I../../include
EXT_LIB_PATH = os.path.join(_HERE, "lib", "libxai_ext.so")
EXT_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "xai_hip_ext.h")
ABI_DEFINES = ("XAI_ABI_VERSION", "XAI_ABI_MINOR")
EXT_DEFINES = ("XAI_EXT_VERSION", "XAI_EXT_MINOR")
EXT2_LIB_PATH = os.path.join(_HERE, "lib", "libxai_ext2.so")
EXT2_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "xai_hip_ext2.h")
EXT2_DEFINES = ("XAI_EXT2_VERSION", "XAI_EXT2_MINOR")
EXT3_LIB_PATH = os.path.join(_HERE, "lib", "libxai_ext3.so")
EXT3_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "xai_hip_ext3.h")
EXT3_DEFINES = ("XAI_EXT3_VERSION", "XAI_EXT3_MINOR")
EXT4_LIB_PATH = os.path.join(_HERE, "lib", "libxai_ext4.so")
EXT4_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "xai_hip_ext4.h")
EXT4_DEFINES = ("XAI_EXT4_VERSION", "XAI_EXT4_MINOR")
EXT5_LIB_PATH = os.path.join(_HERE, "lib", "libxai_ext5.so")
EXT5_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "xai_hip_ext5.h")
EXT5_DEFINES = ("XAI_EXT5_VERSION", "XAI_EXT5_MINOR")
EXT6_LIB_PATH = os.path.join(_HERE, "lib", "libxai_ext6.so")
EXT6_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), "xai_hip_ext6.h")
EXT6_DEFINES = ("XAI_EXT6_VERSION", "XAI_EXT6_MINOR")

_lib = None
_ext = None
_ext2 = None
_ext3 = None
_ext4 = None
_ext5 = None
_ext6 = None


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
    `defines`: the names of the header's two version defines (EXT_DEFINES for include/xai_hip_ext.h)."""
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


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            return parse_header(f.read())
    except (OSError, XaiHipError) as e:
        raise XaiHipError(f"{HEADER_PATH}: the C ABI cannot be bound from its header: {e}") from e


def _read_ext_header():
    try:
        with open(EXT_HEADER_PATH) as f:
            return parse_header(f.read(), EXT_DEFINES)
    except (OSError, XaiHipError) as e:
        raise XaiHipError(f"{EXT_HEADER_PATH}: the extension ABI cannot be bound from its header: {e}") from e


def _read_ext2_header():
    try:
        with open(EXT2_HEADER_PATH) as f:
            return parse_header(f.read(), EXT2_DEFINES)
    except (OSError, XaiHipError) as e:
        raise XaiHipError(f"{EXT2_HEADER_PATH}: the second extension ABI cannot be bound from its header: {e}") from e


def _read_ext3_header():
    try:
        with open(EXT3_HEADER_PATH) as f:
            return parse_header(f.read(), EXT3_DEFINES)
    except (OSError, XaiHipError) as e:
        raise XaiHipError(f"{EXT3_HEADER_PATH}: the third extension ABI cannot be bound from its header: {e}") from e


def _read_ext4_header():
    try:
        with open(EXT4_HEADER_PATH) as f:
            return parse_header(f.read(), EXT4_DEFINES)
    except (OSError, XaiHipError) as e:
        raise XaiHipError(f"{EXT4_HEADER_PATH}: the fourth extension ABI cannot be bound from its header: {e}") from e


def _read_ext5_header():
    try:
        with open(EXT5_HEADER_PATH) as f:
            return parse_header(f.read(), EXT5_DEFINES)
    except (OSError, XaiHipError) as e:
        raise XaiHipError(f"{EXT5_HEADER_PATH}: the fifth extension ABI cannot be bound from its header: {e}") from e


def _read_ext6_header():
    try:
        with open(EXT6_HEADER_PATH) as f:
            return parse_header(f.read(), EXT6_DEFINES)
    except (OSError, XaiHipError) as e:
        raise XaiHipError(f"{EXT6_HEADER_PATH}: the sixth extension ABI cannot be bound from its header: {e}") from e


# name -> argument types / return type of every prototype, and the XAI_ABI_VERSION / XAI_ABI_MINOR the header declares
SIGNATURES, _RESTYPE, (ABI_VERSION, ABI_MINOR) = _read_header()
# the same for the extension header and its XAI_EXT_VERSION / XAI_EXT_MINOR
EXT_SIGNATURES, _EXT_RESTYPE, (EXT_VERSION, EXT_MINOR) = _read_ext_header()
# and for the second extension header and its XAI_EXT2_VERSION / XAI_EXT2_MINOR
EXT2_SIGNATURES, _EXT2_RESTYPE, (EXT2_VERSION, EXT2_MINOR) = _read_ext2_header()
# and for the third extension header and its XAI_EXT3_VERSION / XAI_EXT3_MINOR
EXT3_SIGNATURES, _EXT3_RESTYPE, (EXT3_VERSION, EXT3_MINOR) = _read_ext3_header()
# and for the fourth extension header and its XAI_EXT4_VERSION / XAI_EXT4_MINOR
EXT4_SIGNATURES, _EXT4_RESTYPE, (EXT4_VERSION, EXT4_MINOR) = _read_ext4_header()
# and for the fifth extension header and its XAI_EXT5_VERSION / XAI_EXT5_MINOR
EXT5_SIGNATURES, _EXT5_RESTYPE, (EXT5_VERSION, EXT5_MINOR) = _read_ext5_header()
# and for the sixth extension header and its XAI_EXT6_VERSION / XAI_EXT6_MINOR
EXT6_SIGNATURES, _EXT6_RESTYPE, (EXT6_VERSION, EXT6_MINOR) = _read_ext6_header()


def load():
    """Load the library once; raises (never falls back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise XaiHipError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `make -C "
            f"{os.path.join(os.path.dirname(_HERE), 'csrc')}` (needs hipcc, targets gfx950). "
            "There is deliberately no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    # version first, by the two symbols every build of the library has had or that say "older" by their absence
    lib.xai_version.restype = C.c_int
    major = lib.xai_version()
    minor = 0
    if hasattr(lib, "xai_version_minor"):
        lib.xai_version_minor.restype = C.c_int
        minor = lib.xai_version_minor()
    if major != ABI_VERSION or minor < ABI_MINOR:
        raise XaiHipError(f"{LIB_PATH} has ABI {major}.{minor}, this package needs {ABI_VERSION}.{ABI_MINOR} or a later minor "
                          f"(include/xai_hip.h); rebuild with `make -C {os.path.join(os.path.dirname(_HERE), 'csrc')}`")
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the .so is stale
        fn.argtypes = argtypes
        fn.restype = _RESTYPE[name]
    _lib = lib
    return lib


def load_ext():
    """Load the extension library once, as strictly as `load()`: absent -> XaiHipError, the version pair first, then every
    prototype of include/xai_hip_ext.h (AttributeError if the .so is stale).  Never falls back."""
    global _ext
    if _ext is not None:
        return _ext
    csrc = os.path.join(os.path.dirname(_HERE), "csrc")
    if not os.path.exists(EXT_LIB_PATH):
        raise XaiHipError(f"{EXT_LIB_PATH} not found: the HIP extension library is not built. Run `make -C {csrc}` (needs hipcc, "
                          "targets gfx950). There is deliberately no CPU fallback.")
    lib = C.CDLL(EXT_LIB_PATH)
    lib.xai_ext_version.restype = lib.xai_ext_version_minor.restype = C.c_int
    major, minor = lib.xai_ext_version(), lib.xai_ext_version_minor()
    if major != EXT_VERSION or minor < EXT_MINOR:
        raise XaiHipError(f"{EXT_LIB_PATH} has ABI {major}.{minor}, this package needs {EXT_VERSION}.{EXT_MINOR} or a later minor "
                          f"(include/xai_hip_ext.h); rebuild with `make -C {csrc}`")
    for name, argtypes in EXT_SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the .so is stale
        fn.argtypes = argtypes
        fn.restype = _EXT_RESTYPE[name]
    _ext = lib
    return lib


def load_ext2():
    """Load the second extension library once, as strictly as `load_ext()`: absent -> XaiHipError, the version pair first, then
    every prototype of include/xai_hip_ext2.h (AttributeError if the .so is stale).  Never falls back."""
    global _ext2
    if _ext2 is not None:
        return _ext2
    csrc = os.path.join(os.path.dirname(_HERE), "csrc")
    if not os.path.exists(EXT2_LIB_PATH):
        raise XaiHipError(f"{EXT2_LIB_PATH} not found: the second HIP extension library is not built. Run `make -C {csrc}` (needs "
                          "hipcc, targets gfx950). There is deliberately no CPU fallback.")
    lib = C.CDLL(EXT2_LIB_PATH)
    lib.xai_ext2_version.restype = lib.xai_ext2_version_minor.restype = C.c_int
    major, minor = lib.xai_ext2_version(), lib.xai_ext2_version_minor()
    if major != EXT2_VERSION or minor < EXT2_MINOR:
        raise XaiHipError(f"{EXT2_LIB_PATH} has ABI {major}.{minor}, this package needs {EXT2_VERSION}.{EXT2_MINOR} or a later minor "
                          f"(include/xai_hip_ext2.h); rebuild with `make -C {csrc}`")
    for name, argtypes in EXT2_SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the .so is stale
        fn.argtypes = argtypes
        fn.restype = _EXT2_RESTYPE[name]
    _ext2 = lib
    return lib


def load_ext3():
    """Load the third extension library once, as strictly as `load_ext2()`: absent -> XaiHipError, the version pair first, then
    every prototype of include/xai_hip_ext3.h (AttributeError if the .so is stale).  Never falls back."""
    global _ext3
    if _ext3 is not None:
        return _ext3
    csrc = os.path.join(os.path.dirname(_HERE), "csrc")
    if not os.path.exists(EXT3_LIB_PATH):
        raise XaiHipError(f"{EXT3_LIB_PATH} not found: the third HIP extension library is not built. Run `make -C {csrc}` (needs "
                          "hipcc, targets gfx950). There is deliberately no CPU fallback.")
    lib = C.CDLL(EXT3_LIB_PATH)
    lib.xai_ext3_version.restype = lib.xai_ext3_version_minor.restype = C.c_int
    major, minor = lib.xai_ext3_version(), lib.xai_ext3_version_minor()
    if major != EXT3_VERSION or minor < EXT3_MINOR:
        raise XaiHipError(f"{EXT3_LIB_PATH} has ABI {major}.{minor}, this package needs {EXT3_VERSION}.{EXT3_MINOR} or a later minor "
                          f"(include/xai_hip_ext3.h); rebuild with `make -C {csrc}`")
    for name, argtypes in EXT3_SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the .so is stale
        fn.argtypes = argtypes
        fn.restype = _EXT3_RESTYPE[name]
    _ext3 = lib
    return lib


def load_ext4():
    """Load the fourth extension library once, as strictly as `load_ext3()`: absent -> XaiHipError, the version pair first, then
    every prototype of include/xai_hip_ext4.h (AttributeError if the .so is stale).  Never falls back."""
    global _ext4
    if _ext4 is not None:
        return _ext4
    csrc = os.path.join(os.path.dirname(_HERE), "csrc")
    if not os.path.exists(EXT4_LIB_PATH):
        raise XaiHipError(f"{EXT4_LIB_PATH} not found: the fourth HIP extension library is not built. Run `make -C {csrc}` (needs "
                          "hipcc, targets gfx950). There is deliberately no CPU fallback.")
    lib = C.CDLL(EXT4_LIB_PATH)
    lib.xai_ext4_version.restype = lib.xai_ext4_version_minor.restype = C.c_int
    major, minor = lib.xai_ext4_version(), lib.xai_ext4_version_minor()
    if major != EXT4_VERSION or minor < EXT4_MINOR:
        raise XaiHipError(f"{EXT4_LIB_PATH} has ABI {major}.{minor}, this package needs {EXT4_VERSION}.{EXT4_MINOR} or a later minor "
                          f"(include/xai_hip_ext4.h); rebuild with `make -C {csrc}`")
    for name, argtypes in EXT4_SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the .so is stale
        fn.argtypes = argtypes
        fn.restype = _EXT4_RESTYPE[name]
    _ext4 = lib
    return lib


def load_ext5():
    """Load the fifth extension library once, as strictly as `load_ext4()`: absent -> XaiHipError, the version pair first, then
    every prototype of include/xai_hip_ext5.h (AttributeError if the .so is stale).  Never falls back."""
    global _ext5
    if _ext5 is not None:
        return _ext5
    csrc = os.path.join(os.path.dirname(_HERE), "csrc")
    if not os.path.exists(EXT5_LIB_PATH):
        raise XaiHipError(f"{EXT5_LIB_PATH} not found: the fifth HIP extension library is not built. Run `make -C {csrc}` (needs "
                          "hipcc, targets gfx950). There is deliberately no CPU fallback.")
    lib = C.CDLL(EXT5_LIB_PATH)
    lib.xai_ext5_version.restype = lib.xai_ext5_version_minor.restype = C.c_int
    major, minor = lib.xai_ext5_version(), lib.xai_ext5_version_minor()
    if major != EXT5_VERSION or minor < EXT5_MINOR:
        raise XaiHipError(f"{EXT5_LIB_PATH} has ABI {major}.{minor}, this package needs {EXT5_VERSION}.{EXT5_MINOR} or a later minor "
                          f"(include/xai_hip_ext5.h); rebuild with `make -C {csrc}`")
    for name, argtypes in EXT5_SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the .so is stale
        fn.argtypes = argtypes
        fn.restype = _EXT5_RESTYPE[name]
    _ext5 = lib
    return lib


def load_ext6():
    """Load the sixth extension library once, as strictly as `load_ext5()`: absent -> XaiHipError, the version pair first, then
    every prototype of include/xai_hip_ext6.h (AttributeError if the .so is stale).  Never falls back."""
    global _ext6
    if _ext6 is not None:
        return _ext6
    csrc = os.path.join(os.path.dirname(_HERE), "csrc")
    if not os.path.exists(EXT6_LIB_PATH):
        raise XaiHipError(f"{EXT6_LIB_PATH} not found: the sixth HIP extension library is not built. Run `make -C {csrc}` (needs "
                          "hipcc, targets gfx950). There is deliberately no CPU fallback.")
    lib = C.CDLL(EXT6_LIB_PATH)
    lib.xai_ext6_version.restype = lib.xai_ext6_version_minor.restype = C.c_int
    major, minor = lib.xai_ext6_version(), lib.xai_ext6_version_minor()
    if major != EXT6_VERSION or minor < EXT6_MINOR:
        raise XaiHipError(f"{EXT6_LIB_PATH} has ABI {major}.{minor}, this package needs {EXT6_VERSION}.{EXT6_MINOR} or a later minor "
                          f"(include/xai_hip_ext6.h); rebuild with `make -C {csrc}`")
    for name, argtypes in EXT6_SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the .so is stale
        fn.argtypes = argtypes
        fn.restype = _EXT6_RESTYPE[name]
    _ext6 = lib
    return lib


def check(code, what):
    if code != 0:
        msg = load().xai_strerror(code).decode()
        raise XaiHipError(f"{what} failed with code {code}: {msg}")
