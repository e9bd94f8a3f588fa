"""ctypes binding of libreidmi.so (the C ABI in include/reidmi.h).

This is the product's only route to compute: there is no CPU or PyTorch fallback.
If the library is missing or no GPU is present, calls raise loudly.

The headers are the one written copy of the ABI: every entry point's argtypes / restype and
every struct's ctypes.Structure are read from include/reidmi.h (and reidmi_tools.h).
build_lib.manifest_matches() ties a loaded library to those same header files.
"""
import ctypes
import functools
import os
import re

import torch

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, "libreidmi.so")
TOOLS_LIB_PATH = os.path.join(PKG, "libreidmi_tools.so")  # tests / A-B tools only (reidmi_tools.h)

_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
            "double": ctypes.c_double, "uint16_t": ctypes.c_uint16}
_POINTEES = ("void", "char", "uint8_t", "uint64_t")  # known only behind a pointer
_RESULTS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "char*": ctypes.c_char_p}

_LIB = None
_TOOLS = None


class ReidmiError(RuntimeError):
    pass


def _ctype(ctype, types, where):
    """Scalars by value; a pointer to a header struct is POINTER(its class); every other pointer
    (to a scalar, void, char, a handle) is c_void_p, so callers pass data_ptr() ints and byref()."""
    base = re.sub(r"\bconst\b|\*|\s+", "", ctype)
    stars = ctype.count("*")
    known = types.get(base)
    if stars == 0 and known is not None:
        return known
    if stars == 1 and isinstance(known, type) and issubclass(known, ctypes.Structure):
        return ctypes.POINTER(known)
    if stars >= 1 and (known is not None or base in _POINTEES):
        return ctypes.c_void_p
    raise ReidmiError(f"reidmi header: unknown type `{ctype.strip()}` in `{where}`")


def parse_header(text, types=None):
    """(types, prototypes) of a header in the style of include/reidmi.h, read as C.
    types: {C name: ctypes type} of the scalars, each `typedef struct NAME {...} NAME;` (a
    ctypes.Structure with the header's field names) and each opaque handle typedef, on top of the
    `types` of an included header.  prototypes: {name: (restype, argtypes)}.  Whatever it does not
    know raises ReidmiError naming the declaration: nothing is guessed and nothing skipped."""
    types = dict(_SCALARS if types is None else types)
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#ifdef __cplusplus\n.*?^[ \t]*#endif[^\n]*$", " ", text, flags=re.S | re.M)
    text = re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M)

    def struct(m):
        name, body = m.group(1), m.group(2)
        if m.group(3) != name:
            raise ReidmiError(f"reidmi header: typedef struct {name} is named {m.group(3)}")
        fields = []
        for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
            f = re.fullmatch(r"(.+?[\s*])\s*(\w+(?:\[\d+\])?(?:\s*,\s*\w+(?:\[\d+\])?)*)", decl)
            if not f or ("*" in f.group(1) and "," in f.group(2)):
                raise ReidmiError(f"reidmi header: cannot parse field `{decl}` of {name}")
            ctype = _ctype(f.group(1), types, f"{name}: {decl}")
            for d in re.split(r"\s*,\s*", f.group(2)):
                field, _, dim = d.rstrip("]").partition("[")
                fields.append((field, ctype * int(dim) if dim else ctype))
        types[name] = type(name, (ctypes.Structure,), {"_fields_": fields})
        return " "

    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    protos = {}
    for decl in filter(None, (" ".join(d.split()) for d in text.split(";"))):
        handle = re.fullmatch(r"typedef struct \w+ ?\* ?(\w+)", decl)
        if handle:
            types[handle.group(1)] = ctypes.c_void_p
            continue
        p = re.fullmatch(r"(.+?[\s*])\s*(reidmi_\w+) ?\(([^()]*)\)", decl)
        if not p:
            raise ReidmiError(f"reidmi header: cannot parse declaration `{decl}`")
        restype = _RESULTS.get(re.sub(r"\bconst\b|\s+", "", p.group(1)))
        if restype is None:
            raise ReidmiError(f"reidmi header: unknown result type `{p.group(1).strip()}` in `{decl}`")
        argtypes = []
        for arg in ([] if p.group(3).strip() == "void" else p.group(3).split(",")):
            a = re.fullmatch(r"(.+?[\s*])\s*\w+", arg.strip())
            if not a:
                raise ReidmiError(f"reidmi header: cannot parse argument `{arg.strip()}` in `{decl}`")
            argtypes.append(_ctype(a.group(1), types, decl))
        protos[p.group(2)] = (restype, argtypes)
    return types, protos


@functools.lru_cache(maxsize=None)
def _abi():
    from . import build_lib

    def read(name):
        with open(os.path.join(build_lib.INCLUDE, name)) as f:
            return f.read()
    ftypes, _ = parse_header(read("reidmi_filter.h"))  # reidmi.h includes it
    types, product = parse_header(read("reidmi.h"), ftypes)
    _, tools = parse_header(read("reidmi_tools.h"), types)
    return types, product, tools, ftypes


def declarations(tools=False):
    """{entry point: (restype, argtypes)} of include/reidmi.h, with reidmi_tools.h's for tools."""
    _, product, extra, _ = _abi()
    return dict(product, **extra) if tools else dict(product)


def structs(header="reidmi.h"):
    """{C struct name: its ctypes.Structure} of the structs include/<header> itself defines:
    reidmi.h (the model's weight and source structs) or reidmi_filter.h, which reidmi.h includes
    (reidmi_search_filter)."""
    types, _, _, ftypes = _abi()
    if header not in ("reidmi.h", "reidmi_filter.h"):
        raise ReidmiError(f"structs: no such header `{header}`")
    own = ftypes if header == "reidmi_filter.h" else {n: t for n, t in types.items() if n not in ftypes}
    return {n: t for n, t in own.items() if isinstance(t, type) and issubclass(t, ctypes.Structure)}


def bind(cdll, tools=False):
    """Type every entry point the header(s) declare on an opened library (a missing one raises)."""
    for name, (restype, argtypes) in declarations(tools).items():
        fn = getattr(cdll, name)
        fn.restype, fn.argtypes = restype, argtypes
    return cdll


def _open(path, tools):
    if not os.path.exists(path):
        raise ReidmiError(f"{path} is not built: run `python __graft_entry__.py build` "
                          "(there is no CPU fallback)")
    from . import build_lib
    if not build_lib.manifest_matches(tools):
        raise ReidmiError(f"{path} was not built from the sources next to it (its manifest differs): "
                          "run `python __graft_entry__.py build`")
    return bind(ctypes.CDLL(path), tools)


def load():
    """Load libreidmi.so (torch's HIP runtime is already loaded by `import torch`, so the
    library's libamdhip64.so.7 dependency resolves to that same runtime)."""
    global _LIB
    if _LIB is None:
        _LIB = _open(LIB_PATH, False)
    return _LIB


def load_tools():
    """libreidmi_tools.so: the product entry points plus reidmi_tools.h's forced variants (tests
    and A/B tools only; its static state — errors, timing hooks — is its own)."""
    global _TOOLS
    if _TOOLS is None:
        _TOOLS = _open(TOOLS_LIB_PATH, True)
    return _TOOLS


def call(name, *args, tools=False):
    L = load_tools() if tools else load()
    rc = getattr(L, name)(*args)
    if rc != 0:
        raise ReidmiError(f"{name} failed ({rc}): {L.reidmi_last_error().decode()}")


def call_tools(name, *args):
    call(name, *args, tools=True)


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream(device=None):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise ReidmiError("libreidmi operates on device tensors (got a CPU tensor)")
