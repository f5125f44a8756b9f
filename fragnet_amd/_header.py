"""Reader of include/fragnet_hip.h: the header's integer constants, structs and prototypes as ctypes objects.

The header is the single statement of the C-ABI; _lib.py derives its whole binding from what ``parse`` returns.  The reader
knows the plain C the header is written in and nothing more: text it does not understand raises FragnetHipError, naming the
text -- it is never skipped.
"""
from __future__ import annotations

import ctypes as C
import re
from typing import NamedTuple


class FragnetHipError(RuntimeError):
    pass


class Header(NamedTuple):
    constants: dict     # "FN_X" -> int
    structs: dict       # "fn_x" -> ctypes.Structure subclass, in the header's order
    functions: dict     # "fn_x" -> (restype, [argtypes]), in the header's order


SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float,
           "double": C.c_double}
_POINTED_TO = {"void", "char", "int8_t", "uint8_t", "uint32_t"}     # only ever behind a pointer, and every such pointer is a c_void_p
_DEFINE = re.compile(r"\s*#\s*define\s+(\w+)(\(?)(.*)")
_INT = re.compile(r"\(?\s*(-?)\s*(0[xX][0-9a-fA-F]+|\d+)\s*\)?")
_DECLARATOR = re.compile(r"((?:\*\s*)*)(\w+)\s*(?:\[\s*(\w+)\s*\])?")


def _fail(what, text):
    raise FragnetHipError(f"include/fragnet_hip.h: {what}: `{' '.join(text.split())}`")


def _split(decl, h, forward, what):
    """`const struct fn_x *a, *b[4]` -> ("fn_x", "*a, *b[4]"); the base type must be one the reader maps."""
    m = re.fullmatch(r"(?:struct\s+)?(\w+)\b\s*(.+)", re.sub(r"\bconst\b", " ", decl).strip(), re.S)
    if not m:
        _fail(what + " not understood", decl)
    if m.group(1) not in SCALARS and m.group(1) not in h.structs and m.group(1) not in forward | _POINTED_TO | {"fn_stream_t"}:
        _fail(f"{what} of unknown type `{m.group(1)}`", decl)
    return m.groups()


def _fields(body, h, forward):
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        base, rest = _split(decl, h, forward, "member")
        for d in rest.split(","):
            m = _DECLARATOR.fullmatch(d.strip()) or _fail("member not understood", decl)
            stars, name, dim = m.groups()
            t = C.c_void_p if stars else SCALARS.get(base) or h.structs.get(base) or _fail(f"member of type `{base}` by value", decl)
            if dim is not None:
                if not (dim.isdigit() or dim in h.constants):
                    _fail(f"array bound `{dim}` is neither a literal nor a defined constant", decl)
                t = t * (int(dim) if dim.isdigit() else h.constants[dim])
            fields.append((name, t))
    return fields


def _argtype(arg, h, forward):
    base, rest = _split(arg, h, forward, "argument")
    m = _DECLARATOR.fullmatch(rest.strip())
    if not m or m.group(3) is not None:
        _fail("argument not understood", arg)
    stars = m.group(1).replace(" ", "")
    if not stars:
        return C.c_void_p if base == "fn_stream_t" else SCALARS.get(base) or _fail(f"argument of type `{base}` by value", arg)
    if stars == "*" and base in h.structs:
        return C.POINTER(h.structs[base])
    return C.POINTER(C.c_int) if stars == "*" and base == "int" else C.c_void_p


def _restype(ret):
    words = re.sub(r"\bconst\b", " ", ret).replace("*", " * ").split()
    if words == ["char", "*"]:
        return C.c_char_p
    if len(words) == 1 and words[0] in ("int", "int64_t", "uint64_t"):
        return SCALARS[words[0]]
    _fail("return type without a mapping", ret)


def camel(name):
    return "".join(w.capitalize() for w in name[len("fn_"):].split("_"))


def parse(text) -> Header:
    h, forward, code = Header({}, {}, {}), set(), []
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    for line in text.replace("\\\n", " ").split("\n"):
        m = _DEFINE.match(line)
        if m and not m.group(2) and m.group(3).strip():          # a function-like macro is no constant; nor is an include guard
            lit = _INT.fullmatch(m.group(3).strip()) if m.group(1).startswith("FN_") else None
            h.constants[m.group(1)] = int(lit.group(1) + lit.group(2), 0) if lit else _fail("define that is no FN_* integer literal", line)
        elif not line.lstrip().startswith("#"):
            code.append(line)
        elif not re.match(r"\s*#\s*(include|ifndef|ifdef|endif|define)\b", line):
            _fail("preprocessor directive the reader does not understand", line)
    text = "\n".join(code)
    wrapped = re.fullmatch(r'\s*extern\s+"C"\s*\{(.*)\}\s*', text, re.S)
    text = wrapped.group(1) if wrapped else text

    def forward_declaration(m):
        forward.add(m.group(1))
        return " "

    def struct(m):
        if m.group(1) != m.group(3):
            _fail("struct tag and typedef name differ", m.group(0))
        h.structs[m.group(1)] = type(camel(m.group(1)), (C.Structure,), {"_fields_": _fields(m.group(2), h, forward)})
        return " "

    def function(m):
        args = [a.strip() for a in m.group(3).split(",")]
        h.functions[m.group(2)] = (_restype(m.group(1)), [] if args == ["void"] else [_argtype(a, h, forward) for a in args])
        return " "

    text = re.sub(r"\btypedef\s+void\s*\*\s*fn_stream_t\s*;", " ", text)
    text = re.sub(r"\bstruct\s+(fn_\w+)\s*;", forward_declaration, text)
    text = re.sub(r"\btypedef\s+struct\s+(fn_\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    text = re.sub(r"([\w\s\*]+?)\b(fn_\w+)\s*\(([^()]*)\)\s*;", function, text)
    if text.strip():
        _fail("text the reader does not understand", text.strip()[:200])
    return h
