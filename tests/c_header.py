"""The C prototypes of include/sympgpr_hip.h and include/sympgpr_probe.h as ctypes, for the tests that compare them with
sympgpr_amd._lib's SIGNATURES / PROBE_SIGNATURES.  A plain module: one parser and one type table for every such test."""
import ctypes as C
import fnmatch
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sympgpr_hip.h")
PROBE_HEADER = os.path.join(ROOT, "include", "sympgpr_probe.h")

_WORDS = {"int", "unsigned", "long", "double", "size_t", "void", "char", "sgpr_fit_t"}   # what a type is spelled with
_POINTEES = {"int": C.c_int, "unsigned": C.c_uint, "double": C.c_double, "size_t": C.c_size_t, "long": C.c_long,
             "long long": C.c_longlong, "unsigned long long": C.c_ulonglong, "void *": C.c_void_p, "sgpr_fit_t": C.c_void_p}
# the one table: the scalars, const char *, the pointers to the types above, and `double *const *`, a pointer to double *
CTYPES = {t: c for t, c in _POINTEES.items() if "long long" not in t}
CTYPES.update({(t + " *").replace("* *", "**"): C.POINTER(c) for t, c in _POINTEES.items()})
CTYPES.update({"const char *": C.c_char_p, "double **": C.POINTER(C.POINTER(C.c_double))})


def _type(decl):
    """`const double *x` -> `double *`, `T out[k]` -> `T *`, `double *const *C` -> `double **`; const stays on char only"""
    stars = decl.count("*") + decl.count("[")
    words = re.findall(r"[A-Za-z_]\w*", re.sub(r"\[[^\]]*\]", " ", decl))
    const = "const" in words
    words = [w for w in words if w != "const"]
    if len(words) > 1 and words[-1] not in _WORDS:
        words.pop()                                   # the parameter's name
    base = " ".join(words)
    return ("const " if const and base == "char" else "") + base + (" " + "*" * stars if stars else "")


def _parse(path):
    """(name, return type, [parameter declarations as written, blanks collapsed]) of every sgpr_* prototype: comments,
    preprocessor lines and the extern "C" brace are stripped, what is left is cut at the semicolons"""
    txt = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(path).read(), flags=re.S)
    txt = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*$", " ", txt, flags=re.M)
    for stmt in re.sub(r'extern\s+"C"\s*\{', " ", txt).split(";"):
        m = re.match(r"\s*(.*?)\b(sgpr_[a-z0-9_]+)\s*\((.*)\)\s*$", stmt, flags=re.S)
        if m:
            params = [" ".join(p.split()) for p in m.group(3).split(",")]
            yield m.group(2), _type(m.group(1) + " _"), [] if params == ["void"] else params


def prototypes(path=HEADER):
    """{name: (return type, [parameter types])} of every sgpr_* prototype of the header"""
    return {name: (ret, [_type(p) for p in params]) for name, ret, params in _parse(path)}


def ctypes_of(proto):
    """(restype, [argtypes]) of a prototype; a type the table does not know is a KeyError"""
    return CTYPES[proto[0]], [CTYPES[p] for p in proto[1]]


def comment_above(name, path=HEADER):
    """the comment in front of a prototype, blanks collapsed: where the header documents the entry"""
    hdr = open(path).read()
    m = re.search(r"\bint\s+%s\s*\(" % name, hdr)
    assert m, name + " is not declared"
    return " ".join(hdr[:m.start()].rsplit("*/", 1)[0].rsplit("/*", 1)[1].split())


def in_exports_map(name):
    """a global pattern of csrc/exports.map covers the name"""
    text = open(os.path.join(ROOT, "sympgpr_amd", "csrc", "exports.map")).read().split("local:")[0]
    return any(fnmatch.fnmatchcase(name, g) for g in re.findall(r"^\s*([A-Za-z_*]+);", text, flags=re.M))


def binding_errors(name, proto, row, fn=None):
    """How the table row (restype, argtypes) of `name` departs from its prototype, as a list of messages.  The one exception: in
    an entry whose name ends in _dev a pointer parameter may be bound as c_void_p -- device addresses are handed over as
    integers.  fn: the function of the loaded library, which must carry exactly the row."""
    res, args = ctypes_of(proto)
    errs = [] if row[0] is res else ["%s: restype %s, the header says %s" % (name, row[0], proto[0])]
    if len(row[1]) != len(args):
        return errs + ["%s: %d argtypes, the header has %d parameters" % (name, len(row[1]), len(args))]
    for i, (got, want, text) in enumerate(zip(row[1], args, proto[1])):
        if got is not want and not (name.endswith("_dev") and text.endswith("*") and got is C.c_void_p):
            errs.append("%s: argument %d bound as %s, the header says %s" % (name, i, got, text))
    if fn is not None and (fn.restype is not row[0] or list(fn.argtypes or []) != list(row[1])):
        errs.append("%s: the loaded library's function does not carry the table's row" % name)
    return errs


def assert_bound_as_declared(name, nargs=None, probe=False, restype=C.c_int):
    """One entry: declared once in its header with `restype` (and nargs parameters, if given), bound in _lib's table and in the
    loaded library as declared (binding_errors).  -> the parameter declarations as written, blanks collapsed."""
    from sympgpr_amd import _lib as L
    path, table = (PROBE_HEADER, L.PROBE_SIGNATURES) if probe else (HEADER, L.SIGNATURES)
    lib = L.load_probe_library() if probe else L.load_library()
    found = [params for n, _, params in _parse(path) if n == name]
    assert len(found) == 1 and name in table, "%s: declared %d times, in the table: %s" % (name, len(found), name in table)
    errs = binding_errors(name, prototypes(path)[name], table[name], getattr(lib, name))
    assert not errs and table[name][0] is restype and nargs in (None, len(found[0])), (errs, table[name][0], len(found[0]))
    return found[0]
