"""include/ltxmi.h -> ctypes: the struct classes, the integer constants and every prototype's (restype, argtypes).

Needs nothing but ``re`` and ``ctypes``.  It reads exactly the C the header is written in and raises ``HeaderError`` with the
declaration on anything else -- nothing is guessed, and no unknown type turns into a ``c_void_p``:
  - /* */ comments; #include / #if* / #endif (skipped); ``#define NAME <integer | "string">``; ``extern "C" { }``;
  - ``typedef enum N { A = <integer>, ... } N;``
  - ``typedef struct N { <type> a, b[DEFINE]; ... } N;`` with N in the caller's struct-name map;
  - ``<type> name(<type> [name], ...);``
where <type> is int / int32_t (c_int32), int64_t, float, a pointer to one of those, to void or to uint32_t (c_void_p), a
pointer to a struct declared above or handed in as known (POINTER(Struct)) and, as a return type, ``const char*`` (c_char_p).
"""
import ctypes
import re
from collections import namedtuple

Abi = namedtuple("Abi", "structs constants strings signatures")     # structs: Python name -> class; the rest by C name
SCALARS = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
POINTEES = set(SCALARS) | {"void", "uint32_t"}

_TOP = re.compile(r"""\s*(?: typedef\s+enum\s+(?P<enum>\w+)\s*\{(?P<ebody>[^{}]*)\}\s*(?P=enum)\s*;
                           | typedef\s+struct\s+(?P<struct>\w+)\s*\{(?P<sbody>[^{}]*)\}\s*(?P=struct)\s*;
                           | (?P<ret>[\w\s*]+?)\b(?P<fn>\w+)\s*\((?P<params>[^(){}]*)\)\s*;
                           | extern\s+"C"\s*\{ | \} )""", re.X)
_DEFINE = re.compile(r'#\s*define\s+(\w+)(?:\s+(?:(-?\d+)|"([^"]*)"))?\s*')
_TYPE = r"(?:const\s+)?(\w+)\s*"
_DECLARATOR = re.compile(r"(\*?)\s*(\w+)\s*(?:\[\s*(\w+)\s*\])?")


class HeaderError(ValueError):
    pass


def parse(text, struct_names, known_structs=None):
    """``text``: the header; ``struct_names``: C struct name -> Python class name, one entry per struct of the header;
    ``known_structs``: C struct name -> class, the structs of the headers this one includes that its prototypes may point to."""
    structs, by_c_name, constants, strings, signatures = {}, dict(known_structs or {}), {}, {}, {}

    def ctype(base, star, decl, ret=False):
        if not star and base in SCALARS:
            return SCALARS[base]
        if star and base in by_c_name:
            return ctypes.POINTER(by_c_name[base])
        if star and base in POINTEES:
            return ctypes.c_void_p
        if star and ret and base == "char":
            return ctypes.c_char_p
        raise HeaderError(f"ltxmi.h: type `{base}{star}` is outside the accepted subset in `{decl}`")

    def fields(body):
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            m = re.match(_TYPE, decl)
            for d in decl[m.end() if m else 0:].split(","):
                f = m and _DECLARATOR.fullmatch(d.strip())
                if not f:
                    raise HeaderError(f"ltxmi.h: cannot read the declarator `{d.strip()}` in `{decl}`")
                t = ctype(m.group(1), f.group(1), decl)
                if f.group(3) is not None:
                    if not f.group(3).isdigit() and f.group(3) not in constants:
                        raise HeaderError(f"ltxmi.h: array length `{f.group(3)}` is no integer #define in `{decl}`")
                    t = t * int(constants.get(f.group(3), f.group(3)))
                yield f.group(2), t

    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for line in re.findall(r"^[ \t]*#.*$", text, flags=re.M):
        m = _DEFINE.fullmatch(line.strip())
        if m and m.group(2) is not None:
            constants[m.group(1)] = int(m.group(2))
        elif m and m.group(3) is not None:
            strings[m.group(1)] = m.group(3)
        elif not m and not re.match(r"\s*#\s*(include|ifdef|ifndef|endif)\b", line):
            raise HeaderError(f"ltxmi.h: preprocessor line outside the accepted subset: `{line.strip()}`")
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M).rstrip()
    pos = 0
    while pos < len(text):
        m = _TOP.match(text, pos)
        if not m:
            raise HeaderError(f"ltxmi.h: declaration outside the accepted subset: `{' '.join(text[pos:].split(';')[0].split())};`")
        pos, decl = m.end(), " ".join(m.group(0).split())
        if m.group("enum"):
            for item in filter(None, (i.strip() for i in m.group("ebody").split(","))):
                e = re.fullmatch(r"(\w+)\s*=\s*(-?\d+)", item)
                if not e:
                    raise HeaderError(f"ltxmi.h: enum constant without an integer value: `{item}` in {m.group('enum')}")
                constants[e.group(1)] = int(e.group(2))
        elif m.group("struct"):
            name = m.group("struct")
            if name not in struct_names:
                raise HeaderError(f"ltxmi.h: struct {name} has no Python name in the struct-name map")
            cls = type(struct_names[name], (ctypes.Structure,), {"_fields_": list(fields(m.group("sbody")))})
            structs[struct_names[name]] = by_c_name[name] = cls
        elif m.group("fn"):
            r = re.fullmatch(_TYPE + r"(\*?)\s*", m.group("ret"))
            params = [p.strip() for p in m.group("params").split(",")]
            args = [] if params == ["void"] else [re.fullmatch(_TYPE + r"(\*?)\s*(\w+)?", p) for p in params]
            if not r or None in args:
                raise HeaderError(f"ltxmi.h: cannot read the prototype `{decl}`")
            signatures[m.group("fn")] = (ctype(r.group(1), r.group(2), decl, ret=True),
                                         [ctype(a.group(1), a.group(2), decl) for a in args])
    return Abi(structs, constants, strings, signatures)
