"""Reader of include/icpmi.h: the header is the one description of the C ABI, and the ctypes binding is read from it.

``read(text)`` returns three tables: the integer constants ``{NAME: int}`` of every ``#define ICPMI_<NAME> <integer>``, a
``ctypes.Structure`` subclass for every ``typedef struct icpmi_x { ... } icpmi_x;`` (keyed by the C name) and
``{name: (restype, argtypes)}`` for every prototype.  The reader is strict, which is what makes the header safe to lean
on: it accounts for every character outside comments, and whatever it does not recognise — a declaration of another
shape, a type it has no ctypes type for, a ``#define`` whose body is not one integer — raises ``HeaderError`` with the
line.  Nothing is skipped, and no type falls back to ``c_void_p``.  No HIP, no torch.
"""
import collections
import ctypes as C
import keyword
import re

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
           "size_t": C.c_size_t, "double": C.c_double, "float": C.c_float}
# what a pointer may point to besides a scalar above or a struct of the header (char: c_char_p; the rest: c_void_p)
POINTEES = {"void", "char", "int8_t", "uint8_t", "int16_t", "uint16_t"}

Header = collections.namedtuple("Header", "constants structs functions")


class HeaderError(ValueError):
    pass


_COMMENT = re.compile(r"/\*.*?\*/|//[^\n]*", re.S)
_SPACE = re.compile(r"\s*")
# the include guard, the two includes and the extern "C" guard: the only lines that are none of the three constructs
_FIXED = re.compile(r'(?:#ifndef ICPMI_H|#define ICPMI_H|#include <stddef\.h>|#include <stdint\.h>|#ifdef __cplusplus|'
                    r'extern "C" \{|\}|#endif)[ \t]*$', re.M)
_DEFINE = re.compile(r"#define[ \t]+ICPMI_(\w+)[ \t]+(.*)$", re.M)
_INTEGER = r"-?(?:0[xX][0-9a-fA-F]+|0|[1-9][0-9]*)"
_BODY = re.compile(rf"({_INTEGER})|\(\s*({_INTEGER})\s*\)")
_TYPE = r"(?:const\s+)?\w+\s*\*?"
_STRUCT = re.compile(r"typedef\s+struct\s+(icpmi_\w+)\s*\{([^{}]*)\}\s*\1\s*;")
_FIELDS = re.compile(rf"({_TYPE})\s*(\w+(?:\s*,\s*\w+)*)")
_PROTOTYPE = re.compile(rf"({_TYPE})\s*(icpmi_\w+)\s*\(([^()]*)\)\s*;")
_DECLARATION = re.compile(r"(?:const\s+)?(\w+)\s*(\*?)\s*\w*")


def read(text, reserved=()):
    """The tables of a header's text.  ``reserved``: names a constant may not take (the importing module's own)."""
    text = _COMMENT.sub(lambda m: "\n" * m.group().count("\n"), text)         # line numbers stay
    constants, structs, functions = {}, {}, {}

    def fail(at, why):
        line = text.count("\n", 0, at)
        raise HeaderError(f"include/icpmi.h line {line + 1}: {why}: {text.splitlines()[line].strip()!r}")

    def pieces(m, group, separator):
        """(piece, where it starts) of a match's group split at a separator; blank pieces included."""
        at = m.start(group)
        for piece in m.group(group).split(separator):
            yield piece.strip(), at + len(piece) - len(piece.lstrip())
            at += len(piece) + 1

    def ctype(declaration, at):
        """The ctypes type of ``[const] base[*] [name]``: a result type, a parameter or the type of a struct's fields."""
        m = _DECLARATION.fullmatch(declaration)
        base, pointer = (m.group(1), m.group(2)) if m else (None, None)
        if base in SCALARS and not pointer:
            return SCALARS[base]
        if base == "char" and pointer:
            return C.c_char_p
        if base in structs and pointer:
            return C.POINTER(structs[base])
        if (base in SCALARS or base in POINTEES) and pointer:
            return C.c_void_p
        fail(at, f"no ctypes type for {declaration!r}")

    pos = 0
    while True:
        pos = _SPACE.match(text, pos).end()
        if pos == len(text):
            return Header(constants, structs, functions)
        if pos and text[pos - 1] != "\n":
            fail(pos, "a declaration starts in column 0")
        if m := _FIXED.match(text, pos):
            pass
        elif m := _DEFINE.match(text, pos):
            name, body = m.group(1), _BODY.fullmatch(m.group(2).strip())
            if not body:
                fail(pos, "the body of a #define ICPMI_* must be one integer")
            if name in reserved or name in constants:
                fail(pos, f"the name {name} is taken")
            constants[name] = int(body.group(1) or body.group(2), 0)
        elif m := _STRUCT.match(text, pos):
            fields = []
            for declaration, at in pieces(m, 2, ";"):
                f = _FIELDS.fullmatch(declaration)
                if f:
                    fields += [(n + "_" * keyword.iskeyword(n), ctype(f.group(1), at)) for n in re.split(r"\s*,\s*", f.group(2))]
                elif declaration:                                             # blank: what follows the last `;`
                    fail(at, "not a field declaration")
            camel = "".join(part.capitalize() for part in m.group(1).split("_")[1:])
            structs[m.group(1)] = type(camel, (C.Structure,), {"_fields_": fields, "__doc__": f"{m.group(1)} (include/icpmi.h)"})
        elif m := _PROTOTYPE.match(text, pos):
            args = [] if m.group(3).strip() == "void" else [ctype(a, at) for a, at in pieces(m, 3, ",")]
            functions[m.group(2)] = (ctype(m.group(1).strip(), pos), args)
        else:
            fail(pos, "not a #define ICPMI_<NAME> <integer>, a typedef struct icpmi_x { ... } icpmi_x; or a prototype")
        pos = m.end()
