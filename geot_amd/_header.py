"""The one parser of include/geot_hip.h: its entry points and its integer constants.

Both bindings of the C ABI read the header through parse(): _lib.py derives the ctypes argtypes and the mirrored
constants from it at import, csrc_torch/gen_dispatch.py the compiled forwarders at build time.  Standard library only,
and nothing else of the package is imported, so the build can use it before anything is built.

A declaration the parser cannot type is an error (ValueError naming it), never an entry point left out of a binding.
"""
import ast
import collections
import operator
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "geot_hip.h")

# params: [(kind, declaration)], kind "ptr" or a scalar type in its canonical spelling; streamed: the last parameter
# is `void *stream`, i.e. the entry point launches on a stream and returns hipError_t
Entry = collections.namedtuple("Entry", "ret name params streamed")
SCALARS = {"int": "int", "float": "float", "double": "double", "long long": "long long", "unsigned": "unsigned",
           "unsigned int": "unsigned", "unsigned long long": "unsigned long long"}
_OPS = {ast.Add: operator.add, ast.Sub: operator.sub, ast.Mult: operator.mul}


def _constant(name, expr, known):
    """An integer expression over + - * and the names defined before it, by a walk of its ast (nothing is executed)."""
    def value(node):
        if isinstance(node, ast.Constant) and type(node.value) is int:
            return node.value
        if isinstance(node, ast.Name) and node.id in known:
            return known[node.id]
        if isinstance(node, ast.BinOp) and type(node.op) in _OPS:
            return _OPS[type(node.op)](value(node.left), value(node.right))
        raise ValueError("#define %s %s: not an integer expression over known names" % (name, expr))
    try:
        return value(ast.parse(expr, mode="eval").body)
    except SyntaxError:
        raise ValueError("#define %s %s: not an integer expression over known names" % (name, expr)) from None


def parse(text=None):
    """(entry points in header order, {GEOT_* constant: int}) of the header text (default: include/geot_hip.h)."""
    if text is None:
        with open(HEADER) as f:
            text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    entries = []
    for m in re.finditer(r"\b(int|long long|const char \*)\s*(geot_\w+)\s*\(([^;{}()]*)\)\s*;", text):
        ret, name, args = m.group(1), m.group(2), " ".join(m.group(3).split())
        params = []
        for a in (args.split(",") if args and args != "void" else []):
            a = a.strip()
            kind = "ptr" if "*" in a else SCALARS.get(a.rsplit(" ", 1)[0].strip())
            if kind is None:
                raise ValueError("%s: parameter %r has no known scalar type" % (name, a))
            params.append((kind, a))
        streamed = bool(params) and params[-1][1].replace(" ", "") == "void*stream"
        entries.append(Entry(ret, name, params, streamed))
    unparsed = set(re.findall(r"\b(geot_[a-z0-9_]+)\s*\(", text)).symmetric_difference(e.name for e in entries)
    if unparsed:
        raise ValueError("declarations that do not parse: %s" % sorted(unparsed))
    constants = {}
    for name, expr in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(GEOT_\w+)(.*)$", text, flags=re.M):
        if expr.strip():         # (the include guard has no value)
            constants[name] = _constant(name, expr.strip(), constants)
    return entries, constants
