"""ctypes binding of libgomatching_hip.so, derived from the C ABI's one statement: include/gomatching_hip.h.

The header is parsed when this module is imported: its declarations become `SIGNATURES`, its `#define GOM_* <integer>` lines
`CONSTANTS`, its struct typedefs the ctypes `Structure` classes in `STRUCTS`.  Nothing of the ABI is restated here.

The product path has NO fallback: if the shared library is missing or cannot be loaded, importing
the ops raises.  torch is used for device memory and streams only.
"""
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GOM_LIB_PATH") or os.path.join(HERE, "libgomatching_hip.so")   # (override: same-box A/B of two builds)
HEADER_PATH = os.path.join(HERE, "..", "include", "gomatching_hip.h")


class GomError(RuntimeError):
    pass


_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double,
            "unsigned": ctypes.c_uint, "unsigned int": ctypes.c_uint, "unsigned long long": ctypes.c_ulonglong}
_TYPE_WORDS = {"const", "void", "char", "short", "signed", "struct"}.union(*(k.split() for k in _SCALARS))


def _ctype(words, returned=False):
    """ctypes type of the C type spelled by `words` (`*` a word of its own): an argument's, a field's or (`returned`) a return
    type; None for a type outside the mapping."""
    if words[-1:] == ["*"]:                                  # any T*, const or not, is a plain address
        return ctypes.c_char_p if returned and words == ["const", "char", "*"] else ctypes.c_void_p
    return _SCALARS.get(" ".join(words))


def _named(decl, symbol):
    """`type name` (an argument of `symbol`, a field of the struct `symbol`) -> (name, ctypes type).  The name is the last word."""
    words = decl.replace("*", " * ").split()
    ctype = _ctype(words[:-1]) if len(words) > 1 and words[-1].isidentifier() and words[-1] not in _TYPE_WORDS else None
    if ctype is None:
        raise GomError("%s: `%s` is not `type name` with a type that has a ctypes mapping" % (symbol, " ".join(decl.split())))
    return words[-1], ctype


def parse_header(text):
    """The C ABI stated by header text -> (signatures, structs, constants):
      signatures  name -> (restype, argtypes) for every `ret gom_name(args);`
      structs     name -> ctypes.Structure class for every `typedef struct gom_x { ... } gom_x;`, fields in the header's order
      constants   NAME -> int for every `#define GOM_NAME <integer>`
    by the type mapping of `_SCALARS`, every pointer a c_void_p (`const char*` as a return type: c_char_p), `void` as a return
    type None.  A statement or a type outside that raises GomError and names the symbol: nothing is skipped or guessed."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#[ \t]*ifdef[ \t]+__cplusplus\b.*?^[ \t]*#[ \t]*endif\b[^\n]*", "", text, flags=re.S | re.M)   # not C++ here
    constants = {}
    for line in re.findall(r"^[ \t]*#[^\n]*", text, flags=re.M):
        m = re.fullmatch(r"#\s*(\w+)\s*(\w*)\s*(.*?)\s*", line.strip())
        if not m or m.group(1) not in ("define", "include", "ifndef", "endif"):
            raise GomError("header: cannot follow the directive `%s`" % line.strip())
        if m.group(1) == "define" and m.group(2).startswith("GOM_") and re.fullmatch(r"-?(0|[1-9]\d*|0[xX][0-9a-fA-F]+)", m.group(3)):
            constants[m.group(2)] = int(m.group(3), 0)
    text = re.sub(r"^[ \t]*#[^\n]*", "", text, flags=re.M)
    structs = {}

    def struct(m):
        fields = [_named(f, m.group(1)) for f in m.group(2).split(";") if f.strip()]
        structs[m.group(1)] = type(m.group(1), (ctypes.Structure,), {"_fields_": fields})
        return ""
    text = re.sub(r"\btypedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", struct, text, flags=re.S)
    signatures = {}
    for stmt in text.split(";"):
        if not stmt.strip():
            continue
        m = re.fullmatch(r"\s*([\w\s*]+?)\s*\b(gom_\w+)\s*\(([^()]*)\)\s*", stmt)
        if not m:
            raise GomError("header: cannot read `%s` as a declaration `ret gom_name(args)`" % " ".join(stmt.split()))
        ret, name, args = m.groups()
        res = _ctype(ret.replace("*", " * ").split(), returned=True)
        if res is None and ret.split() != ["void"]:          # (`void` as a return type IS restype None)
            raise GomError("%s: no ctypes mapping for the return type `%s`" % (name, " ".join(ret.split())))
        argtypes = [] if args.split() == ["void"] else [_named(a, name)[1] for a in args.split(",")]
        signatures[name] = (res, argtypes)
    return signatures, structs, constants


def _parse_file(path):
    try:
        with open(path) as f:
            return parse_header(f.read())
    except OSError as e:
        raise GomError("the C ABI header is missing: %s (%s)" % (path, e.strerror))


# SIGNATURES: name -> (restype, argtypes), one entry per symbol the header declares
SIGNATURES, STRUCTS, CONSTANTS = _parse_file(HEADER_PATH)
OptimTensor = STRUCTS["gom_optim_tensor"]         # one row of the clipped-AdamW table
MatcherLayer = STRUCTS["gom_matcher_layer"]       # the weights of one matcher transformer layer

GOM_OK = CONSTANTS["GOM_OK"]
_ERR_HIP_BASE = CONSTANTS["GOM_ERR_HIP_BASE"]
_ERR = {CONSTANTS["GOM_ERR_INVALID_ARG"]: "GOM_ERR_INVALID_ARG (violated precondition)",
        CONSTANTS["GOM_ERR_UNSUPPORTED"]: "GOM_ERR_UNSUPPORTED"}

_lib = None


def load():
    """Load the library once; raise loudly when it is absent (no CPU fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    # torch first: it ships its own libamdhip64; loading ours before it would put two HIP runtimes in the process
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise GomError("libgomatching_hip.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(expected at %s)" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != GOM_OK:
        msg = _ERR.get(rc, "HIP error %d" % (rc - _ERR_HIP_BASE) if rc >= _ERR_HIP_BASE else "error %d" % rc)
        raise GomError("%s failed: %s" % (what or "libgomatching_hip call", msg))
