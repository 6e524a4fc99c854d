"""include/mvp_hip.h read as data, for tests/test_abi.py: every argument struct, export prototype and integer #define, with C types
mapped to the ctypes type a binding must use.  Handles what the header contains and nothing more; any other type or statement raises,
so that a new kind of field is added to the map below on purpose."""
import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mvp_hip.h")
SCALARS = {"int": C.c_int, "float": C.c_float, "int64_t": C.c_int64}


def _fields(body, mirrors):
    """`const T* a; int B, C; char s[64]; mvp_x_args g;` -> [(name, ctypes type), ...] in declaration order."""
    out = []
    for stmt in filter(None, (s.strip() for s in body.split(";"))):
        base, rest = re.fullmatch(r"(?:const\s+)?(\w+)\b(.*)", stmt, flags=re.S).groups()
        for decl in rest.split(","):
            star, name, n = re.fullmatch(r"\s*(\*?)\s*(\w+)\s*(?:\[(\d+)\])?\s*", decl).groups()
            if star:
                kind = C.c_void_p
            elif base == "char" and n:
                kind = C.c_char * int(n)
            elif not n and base in SCALARS:
                kind = SCALARS[base]
            elif not n and base in mirrors:  # a struct held by value
                kind = mirrors[base]
            else:
                raise ValueError(f"mvp_hip.h: no ctypes type for the field `{stmt}`")
            out.append((name, kind))
    return out


def _param(text, mirrors):
    """One prototype parameter or return type (`const mvp_x_args*`, `void* stream`, `int M`, `const char*`) -> ctypes type."""
    const, base, star = re.fullmatch(r"\s*(const\s+)?(\w+)\s*(\*?)\s*\w*\s*", text).groups()
    if not star and not const and base in SCALARS:
        return SCALARS[base]
    if star and base == "void" and not const:
        return C.c_void_p
    if star and base == "char" and const:
        return C.c_char_p
    if star and base in mirrors:
        return C.POINTER(mirrors[base])
    raise ValueError(f"mvp_hip.h: no ctypes type for `{text.strip()}`")


def parse(mirrors):
    """(structs, prototypes, defines) of the header.  ``mirrors``: C struct name -> ctypes class (mvp.lib.STRUCTS), for structs held by
    value or pointed to by a prototype.
      structs     {c_name: [(field, ctypes type), ...]}
      prototypes  {export: (ctypes restype, [ctypes argtypes])}
      defines     {name: int}"""
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+(\w+)\s+\(?(-?\d+)\)?\s*$", text, flags=re.M)}
    text = re.sub(r"^\s*#[^\n]*", " ", text, flags=re.M).replace('extern "C" {', " ")
    struct_re = r"typedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;|struct\s+(\w+)\s*\{([^{}]*)\}\s*;"
    structs = {}
    for m in re.finditer(struct_re, text):
        structs[m.group(2) or m.group(3)] = _fields(m.group(1) or m.group(4), mirrors)
    prototypes = {}
    for stmt in filter(None, (s.strip() for s in re.sub(struct_re, " ", text).split(";"))):
        if stmt.startswith("typedef ") or stmt == "}":  # `typedef uint16_t mvp_bf16`, `typedef struct mvp_x mvp_x`, the end of extern "C"
            continue
        ret, name, params = re.fullmatch(r"(.+?)\b(mvp_\w+)\s*\(([^()]*)\)", stmt, flags=re.S).groups()
        prototypes[name] = (_param(ret, mirrors), [_param(p, mirrors) for p in params.split(",")])
    return structs, prototypes, defines
