"""The tests' one parser of the public headers (include/mumpy_hip*.h): what a header declares, and how a C declaration and a ctypes
type compare.  tests/test_abi.py holds every record of lib.SURFACES to it; the feature tests use it for what only they know (pinned
argument names, the grouped entries' relation to their frozen siblings, the refusal sweeps).  A plain module: it imports neither
pytest nor torch, so the child scripts of the refusal sweeps can import it too."""
import ctypes
import functools
import os
import re
from typing import NamedTuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


class Decl(NamedTuple):
    ret: str            # "int", "int64_t" or "const char*"
    args: list          # the arguments as written: "const float* x", "int64_t n"


def header_text(header):
    with open(os.path.join(INCLUDE, header)) as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def decls(header):
    """-> {name: Decl} of every mumpy_* function the header declares, in the header's order."""
    src = re.sub(r"/\*.*?\*/", "", header_text(header), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(int64_t|int|const char\*)\s+(mumpy_\w+)\s*\(([^)]*)\)\s*;", src):
        out[m.group(2)] = Decl(m.group(1), [a.strip() for a in m.group(3).split(",") if a.strip() and a.strip() != "void"])
    return out


def define(header, macro):
    """The integer a `#define <macro> n` of the header gives, parentheses allowed; None when the header has no such line."""
    m = re.search(rf"#define\s+{macro}\s+\(?(-?\d+)\b", header_text(header))
    return None if m is None else int(m.group(1))


def kind(c):
    """ptr / int / i64 / f32 / f64 of a C argument as written ("const float* x", "int64_t n") or of a bare return type ("int")."""
    if "*" in c:
        return "ptr"
    return {"int": "int", "int64_t": "i64", "float": "f32", "double": "f64"}[c.replace("const ", "").split()[0]]


def ckind(t):
    """The same five words for a ctypes type of the binding."""
    if t is ctypes.c_void_p or t is ctypes.c_char_p or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
        return "ptr"
    return {ctypes.c_int: "int", ctypes.c_int64: "i64", ctypes.c_float: "f32", ctypes.c_double: "f64"}[t]


def arg_names(args):
    """["const float* x", "int64_t n"] -> ["x", "n"]"""
    return [a.replace("*", " ").split()[-1] for a in args]


def names_of(header):
    """-> {name: [argument names]} of everything the header declares: what a feature test pins in one comparison."""
    return {name: arg_names(d.args) for name, d in decls(header).items()}
