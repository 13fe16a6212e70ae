"""Reads include/pointgnn_hip.h: the header is the only statement of the C ABI,
and the ctypes binding (_lib.py) is derived from it when the library loads.

This is a reader for that one header's style, not a C parser.  Pure Python: it
imports neither torch nor the shared library.  What does not fit raises
HeaderError and names the place; nothing is guessed.  The header must keep to:
  - comments are /* */ or //; no string or character literal holds either;
  - the only directives are #include, #define, the include guard and
    #ifdef __cplusplus ... #endif (whose lines are skipped), one per line;
  - #define PGNN_X <integers, earlier PGNN_ names, ( ) - << + *>;
  - typedef struct T { ... } T;  fields are `[const] type [*]name[dim][dim]`,
    several declarators after one type are allowed, a dimension is an integer
    expression as above, `type` a scalar of _SCALARS or an earlier struct;
  - everything else is a prototype `ret pgnn_name(params);`, every parameter
    named, `(void)` for none; no arrays, function pointers or structs by value.
Pointers bind as c_void_p except `const char *` (c_char_p), `void **`
(POINTER(c_void_p)) and `[const] S *` for a struct S of the header
(POINTER(S)).
"""
import ast
import ctypes
import functools
import os
import re

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(_ROOT, "include", "pointgnn_hip.h")   # build.py's INCLUDE

_SCALARS = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32,
            "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
            "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t,
            "double": ctypes.c_double, "float": ctypes.c_float}
_BINOPS = {ast.LShift: int.__lshift__, ast.Add: int.__add__,
           ast.Sub: int.__sub__, ast.Mult: int.__mul__}


class HeaderError(ValueError):
    pass


def _int_expr(text, names, where):
    """Value of an integer expression of the header (no eval)."""
    def walk(n):
        if isinstance(n, ast.Constant) and type(n.value) is int:
            return n.value
        if isinstance(n, ast.Name) and n.id in names:
            return names[n.id]
        if isinstance(n, ast.UnaryOp) and isinstance(n.op, ast.USub):
            return -walk(n.operand)
        if isinstance(n, ast.BinOp) and type(n.op) in _BINOPS:
            return _BINOPS[type(n.op)](walk(n.left), walk(n.right))
        raise HeaderError("%s: not an integer expression: %r" % (where, text))
    try:
        return walk(ast.parse(text.strip(), mode="eval").body)
    except SyntaxError:
        raise HeaderError("%s: not an integer expression: %r" % (where, text))


def _ctype(decl, structs, where):
    """ctypes type of `[const] base [*...]` (a return type, or a parameter or
    field without its name)."""
    tokens = re.findall(r"\w+|\*|[^\w\s*]+", decl)
    stars = tokens.count("*")
    base = [t for t in tokens if t not in ("const", "*")]
    if len(base) != 1 or not re.match(r"[A-Za-z_]\w*$", base[0]):
        raise HeaderError("%s: unknown type %r" % (where, decl.strip()))
    base = base[0]
    if not stars:
        if base not in _SCALARS:
            raise HeaderError("%s: unknown type %r" % (where, decl.strip()))
        return _SCALARS[base]
    if tokens == ["const", "char", "*"]:
        return ctypes.c_char_p
    if tokens == ["void", "*", "*"]:
        return ctypes.POINTER(ctypes.c_void_p)
    if stars == 1 and base in structs and tokens[-1] == "*":
        return ctypes.POINTER(structs[base])
    return ctypes.c_void_p


def _struct(name, body, structs, consts):
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        where = "%s field %r" % (name, " ".join(decl.split()))
        m = re.match(r"((?:const\s+)?(\w+))\s*(.*)$", decl, re.S)
        for d in m.group(3).split(",") if m else [""]:
            f = re.match(r"\s*(\*?)\s*(\w+)\s*((?:\[[^\]]+\]\s*)*)$", d)
            if not f:
                raise HeaderError(where + ": cannot place it")
            if f.group(1):
                t = ctypes.c_void_p
            elif m.group(2) in structs:
                t = structs[m.group(2)]
            else:
                t = _ctype(m.group(1), structs, where)
            for dim in reversed(re.findall(r"\[([^\]]+)\]", f.group(3))):
                t = t * _int_expr(dim, consts, where)
            fields.append((f.group(2), t))
    return type(name, (ctypes.Structure,), {"_fields_": fields})


def parse(text):
    """(functions, structs, constants) of a header in the style above."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts, lines, skip = {}, [], False
    for line in text.split("\n"):
        d = re.match(r"\s*#\s*(\w+)\s*(.*?)\s*$", line)
        if not d:
            if not skip:
                lines.append(line)
            continue
        kind, rest = d.groups()
        if rest.endswith("\\"):
            raise HeaderError("continued directive: " + line.strip())
        if kind == "ifdef" and rest == "__cplusplus":
            skip = True
        elif kind == "endif":
            skip = False
        elif kind == "define" and rest.startswith("PGNN_"):
            m = re.match(r"(\w+)(.*)$", rest)
            consts[m.group(1)] = _int_expr(m.group(2), consts,
                                           "#define " + m.group(1))
        elif not (kind == "include" or
                  kind in ("ifndef", "define") and rest.endswith("_H_")):
            raise HeaderError("directive outside the header's style: " +
                              line.strip())
    text, structs = "\n".join(lines), {}

    def take_struct(m):
        if m.group(1) != m.group(3):
            raise HeaderError("struct %s typedef'd as %s" % m.group(1, 3))
        structs[m.group(3)] = _struct(m.group(3), m.group(2), structs, consts)
        return ""
    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;",
                  take_struct, text)
    functions = {}
    for stmt in filter(None, (s.strip() for s in text.split(";"))):
        m = re.match(r"([\w\s*]+?)\b(pgnn_\w+)\s*\(([^()]*)\)$", stmt)
        if not m:
            raise HeaderError("not a pgnn_* prototype: %r" %
                              " ".join(stmt.split())[:80])
        ret, name, params = m.groups()
        args = []
        if params.strip() != "void":
            for p in params.split(","):
                where = "%s parameter %r" % (name, " ".join(p.split()))
                t = re.match(r"(.*[\s*])(\w+)\s*$", p, re.S)
                if not t:
                    raise HeaderError(where + ": unknown type (no name?)")
                args.append(_ctype(t.group(1), structs, where))
        if name in functions:
            raise HeaderError(name + ": declared twice")
        functions[name] = (_ctype(ret, structs, name + " return"), args)
    return functions, structs, consts


@functools.lru_cache(maxsize=None)
def _parsed():
    with open(HEADER) as f:
        return parse(f.read())


def functions():
    """name -> (restype, [argtypes]) of every pgnn_* prototype."""
    return _parsed()[0]


def structs():
    """name -> ctypes.Structure subclass of every typedef struct."""
    return _parsed()[1]


def constants():
    """name -> value of every #define PGNN_X <integer expression>."""
    return _parsed()[2]
