"""Reads include/focnerf.h into ctypes: the `#define FOC_*` integers, one Structure per `typedef struct`, one signature per `foc_*`
declaration. It knows the forms that header uses and nothing else; whatever it does not recognise raises ImportError with the offending
text — it never guesses a type and never skips a declaration (tests/test_abi.py feeds it the refusals)."""
import ctypes
import re

SCALARS = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "int": ctypes.c_int,
           "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
POINTEES = set(SCALARS) | {"void", "uint8_t"}       # what a pointer that travels as c_void_p may point to (or a struct declared above it)

_DIRECTIVE = re.compile(r"^[ \t]*#[ \t]*(.*?)[ \t]*$", re.M)
_KNOWN_DIRECTIVE = re.compile(r"(ifndef|ifdef|define)\s+\w+|endif|include\s*<[\w.]+>")
_DEFINE = re.compile(r"define\s+(FOC_\w+)\s+(\S.*)")
_ITEM = re.compile(r'\s*(?:(extern\s+"C"\s*\{)|(\})|typedef\s+struct\s+\w+\s*\{([^{}]*)\}\s*(\w+)\s*;|([^;{}()]*?)\b(foc_\w+)\s*\(([^;{}()]*)\)\s*;)')
_SPEC = re.compile(r"\s*(const\s+)?(\w+)(?:\s+const)?\s*(.*?)\s*$", re.S)          # `const float` | the declarators
_DECLARATOR = re.compile(r"((?:\*\s*(?:const\s*)?)*)(\w+)$")                       # `*const *name`
_STRUCT_DOC = ("include/focnerf.h `%s`, read from the header at import (tests/test_abi.py compares its size and every field offset with what "
               "gcc gives the header's struct).")


def _refuse(what, text):
    raise ImportError(f"focnerf_amd: include/focnerf.h: {what}: {' '.join(text.split())[:120]!r}")


def _declare(text, structs, where=None):
    """`const float *a, *b` -> [("a", c_void_p), ("b", c_void_p)]; `where`: the text a refusal shows, if not `text`"""
    const, base, declarators = (_SPEC.match(text) or _refuse("not a declaration", where or text)).groups()
    out = []
    for d in declarators.split(","):
        m = _DECLARATOR.match(d.strip()) or _refuse("not a declaration", where or text)
        stars = m.group(1).count("*")
        if stars == 0 and base in SCALARS:
            ctype = SCALARS[base]
        elif stars == 1 and base == "char" and const:
            ctype = ctypes.c_char_p
        elif stars == 1 and base in structs:
            ctype = ctypes.POINTER(structs[base])
        elif stars and (base in POINTEES or base in structs):
            ctype = ctypes.c_void_p
        else:
            _refuse(f"unknown type {base + ' ' + '*' * stars!r}", where or text)
        out.append((m.group(2), ctype))
    return out


def parse(text):
    """(DEFINES name -> int, STRUCTS name -> ctypes.Structure subclass, SIGNATURES name -> (restype, [argtypes])), each in header order."""
    defines, structs, signatures = {}, {}, {}
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    for line in _DIRECTIVE.findall(text):
        m = _DEFINE.fullmatch(line)
        if m:
            try:
                defines[m.group(1)] = int(m.group(2), 0)
            except ValueError:
                _refuse("not an integer", "#" + line)
        elif not _KNOWN_DIRECTIVE.fullmatch(line):
            _refuse("unknown preprocessor line", "#" + line)
    text, pos, depth = _DIRECTIVE.sub("", text).rstrip(), 0, 0
    while pos < len(text):
        m = _ITEM.match(text, pos) or _refuse("unrecognised text", text[pos:])
        pos = m.end()
        extern, close, body, struct, restype, fn, args = m.groups()
        if extern or close:
            depth += 1 if extern else -1
            if depth < 0:
                _refuse("unrecognised text", "}")
        elif struct:
            fields = [f for decl in body.split(";") if decl.strip() for f in _declare(decl, structs)]
            structs[struct] = type(struct, (ctypes.Structure,), {"_fields_": fields, "__doc__": _STRUCT_DOC % struct})
        else:
            argtypes = [] if args.strip() == "void" else [_declare(a, structs, m.group())[0][1] for a in args.split(",")]
            signatures[fn] = (_declare(restype + " r", structs, m.group())[0][1], argtypes)
    if depth:
        _refuse("unrecognised text", 'extern "C" { is never closed')
    return defines, structs, signatures


def read(path):
    with open(path) as f:
        return parse(f.read())
