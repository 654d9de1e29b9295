"""ctypes binding of librcmvs_hip.so (C ABI declared in include/rcmvs.h).

The library is built in-tree by ``__graft_entry__.build()`` (hipcc --offload-arch=gfx950).
There is no fallback: if the shared object is missing or a call fails, an exception is raised.
"""
import ast
import ctypes
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librcmvs_hip.so")
CSRC = os.path.join(_HERE, "csrc")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "rcmvs.h")
EXT_HEADERS = (os.path.join(CSRC, "pc_register.h"), os.path.join(CSRC, "view_select.h"), os.path.join(CSRC, "undistort.h"),
               os.path.join(CSRC, "tsdf_mesh.h"), os.path.join(CSRC, "tsdf_sparse.h"), os.path.join(CSRC, "mesh_clean.h"),
               os.path.join(CSRC, "mesh_decimate.h"), os.path.join(CSRC, "mesh_holes.h"),
               os.path.join(CSRC, "mesh_render.h"), os.path.join(CSRC, "mesh_normals.h"),
               os.path.join(CSRC, "mesh_texture.h"), os.path.join(CSRC, "mesh_simplify.h"),
               os.path.join(CSRC, "fusion_dyn.h"), os.path.join(CSRC, "cloud_knn.h"),
               os.path.join(CSRC, "poisson.h"))                                          # entry-point families declared next to their kernels (same grammar as HEADER)

_lib = None


class RcmvsError(RuntimeError):
    pass


# The header is the binding's only table: every `<ret> rcmvs_name(<params>);` it declares becomes a row of SIGNATURES, every
# `#define RCMVS_<NAME> <integer>` an entry of CONSTANTS.  The C types of the ABI are a closed set; anything else is an error, never a guess.
_CTYPES = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "long long": ctypes.c_longlong}


def _const_expr(text):
    """Value of a #define's expression: integer literals, <<, parentheses -- nothing else."""
    def ev(node):
        if isinstance(node, ast.Constant) and type(node.value) is int:
            return node.value
        if isinstance(node, ast.BinOp) and isinstance(node.op, ast.LShift):
            return ev(node.left) << ev(node.right)
        raise ValueError(text)
    return ev(ast.parse(text.strip(), mode="eval").body)


def _ctype(decl, what, c_type):
    if c_type not in _CTYPES:
        raise RcmvsError(f"{HEADER}: `{decl}`: {what} type `{c_type}` is outside the ABI's types ({', '.join(_CTYPES)}, pointers)")
    return _CTYPES[c_type]


def parse_header(text):
    """The text of include/rcmvs.h -> (SIGNATURES name -> argtypes, _RESTYPES name -> restype where it is not int, CONSTANTS)."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    signatures, restypes, constants, code = {}, {}, {}, []
    for line in text.splitlines():
        if not line.lstrip().startswith("#"):
            code.append(line)
            continue
        m = re.match(r"\s*#\s*define\s+(RCMVS_\w+)\s+(\S.*)", line)          # a macro without a value (the include guard) is no constant
        if m:
            try:
                value = _const_expr(m.group(2))
            except (ValueError, SyntaxError):
                raise RcmvsError(f"{HEADER}: `{line.strip()}`: not an integer expression of literals, << and parentheses") from None
            if m.group(1) in constants:
                raise RcmvsError(f"{HEADER}: {m.group(1)} is defined twice")
            constants[m.group(1)] = value
    for decl in re.sub(r'extern\s+"C"\s*\{', " ", "\n".join(code)).split(";"):
        decl = " ".join(decl.split())
        if "rcmvs_" not in decl:
            continue
        m = re.fullmatch(r"([\w\s*]+?)\s*\b(rcmvs_\w+)\s*\(([^()]*)\)", decl)
        if not m:
            raise RcmvsError(f"{HEADER}: `{decl}` is not a complete `<type> rcmvs_name(<parameters>);` declaration")
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        if name in signatures:
            raise RcmvsError(f"{HEADER}: {name} is declared twice")
        if ret.replace("const", "").replace(" ", "") == "char*":
            restypes[name] = ctypes.c_char_p
        elif ret != "int":
            restypes[name] = _ctype(decl, "return", ret)
        argtypes = []
        for param in ([] if params == "void" else params.split(",")):
            if "*" in param:
                argtypes.append(ctypes.c_void_p)
                continue
            words = [w for w in param.split() if w != "const"]
            if len(words) < 2 or not words[-1].isidentifier():
                raise RcmvsError(f"{HEADER}: `{decl}`: parameter `{param.strip()}` is not `<type> <name>`")
            argtypes.append(_ctype(decl, "parameter", " ".join(words[:-1])))
        signatures[name] = argtypes
    return signatures, restypes, constants


def _read_header():
    try:
        with open(HEADER) as f:
            return f.read()
    except FileNotFoundError:
        raise RcmvsError(f"{HEADER} is missing: the ctypes binding is derived from the C header, which was expected there "
                         "(include/rcmvs.h next to the rc_mvsnet_amd package)") from None


# name -> argtypes (restype is int unless listed in _RESTYPES), and the header's integer macros
SIGNATURES, _RESTYPES, CONSTANTS = parse_header(_read_header())
REQUIRED_VERSION = CONSTANTS["RCMVS_VERSION"]      # the RCMVS_VERSION of the header this binding is derived from


def _read_extensions():
    """EXT_HEADERS -> (name -> argtypes, name -> restype); their integer macros join CONSTANTS.  A name the primary header already has is an error."""
    signatures, restypes = {}, {}
    for path in EXT_HEADERS:
        try:
            with open(path) as f:
                sig, res, const = parse_header(f.read())
        except FileNotFoundError:
            raise RcmvsError(f"{path} is missing: the binding of its entry points is derived from it") from None
        for table, add in ((signatures, sig), (CONSTANTS, const)):
            clash = [k for k in add if k in table or k in SIGNATURES]
            if clash:
                raise RcmvsError(f"{path}: {clash[0]} is already declared")
            table.update(add)
        restypes.update(res)
    return signatures, restypes


# the extension headers' tables; SIGNATURES stays the primary header's alone
EXT_SIGNATURES, _EXT_RESTYPES = _read_extensions()


def sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))


def build(force=False, verbose=False):
    """Compile every HIP source into librcmvs_hip.so for gfx950 (cross-compiles without a GPU).  One object per source
    (csrc/_obj/*.o, rebuilt when the source or any header is newer), compiled in parallel, then one link step."""
    from concurrent.futures import ThreadPoolExecutor
    srcs = sources()
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + [HEADER]
    if not force and os.path.exists(LIB_PATH) and all(os.path.getmtime(LIB_PATH) >= os.path.getmtime(d) for d in srcs + hdrs):
        return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = os.path.join(_HERE, "_obj")
    os.makedirs(objdir, exist_ok=True)
    hdr_time = max(os.path.getmtime(h) for h in hdrs)
    jobs, objs = [], []
    for src in srcs:
        obj = os.path.join(objdir, os.path.basename(src)[:-4] + ".o")
        objs.append(obj)
        if force or not os.path.exists(obj) or os.path.getmtime(obj) < max(os.path.getmtime(src), hdr_time):
            jobs.append([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", src, "-o", obj])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        list(ex.map(run, jobs))
    run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_PATH] + objs)
    return LIB_PATH


def bind(lib):
    """Give every declared entry point of `lib` (the primary header's and the extension headers') its argtypes and restype."""
    for table, restypes in ((SIGNATURES, _RESTYPES), (EXT_SIGNATURES, _EXT_RESTYPES)):
        for name, argtypes in table.items():
            fn = getattr(lib, name)          # AttributeError if the symbol is not exported
            fn.argtypes = argtypes
            fn.restype = restypes.get(name, ctypes.c_int)


def load():
    """Load the shared library (raises RcmvsError when it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("RCMVS_LIB") or LIB_PATH       # RCMVS_LIB: another build of the same ABI (developer A/B of kernel variants, tools/dev/build_variant.sh)
    if not os.path.exists(path):
        raise RcmvsError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                         "(hipcc --offload-arch=gfx950). There is no CPU / eager fallback.")
    lib = ctypes.CDLL(path)
    bind(lib)
    if lib.rcmvs_version() < REQUIRED_VERSION:
        raise RcmvsError(f"librcmvs_hip.so (version {lib.rcmvs_version()}) is older than this package needs ({REQUIRED_VERSION}): rebuild it")
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().rcmvs_last_error_string()
        raise RcmvsError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")


def call(name, *args):
    """Call the status-returning entry point `name` (the full exported name, e.g. "rcmvs_conv3d_fwd") of the loaded library; a non-zero status
    raises RcmvsError with the library's message.  The function is looked up on the current handle at every call."""
    rc = getattr(_lib or load(), name)(*args)
    if rc:
        check(rc, name[len("rcmvs_"):])
