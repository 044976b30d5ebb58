"""The Python binding is read from include/icpmi.h (no GPU): the reader on a small header with one of each form it knows;
what it refuses, with the line; the real header accounted for to the last character; the struct classes against the C
compiler's sizeof and offsetof; and ``bind`` on a second handle of the built library."""
import ctypes as C
import keyword
import os
import subprocess

import pytest

from conftest import REPO
from test_host_cpu import declared_symbols

HEADER = os.path.join(REPO, "include", "icpmi.h")

SMALL = """\
/* a block comment with ( and ; over two lines
#define ICPMI_NOT_THIS 1 */
#ifndef ICPMI_H
#define ICPMI_H
#include <stddef.h>
#define ICPMI_PLAIN 7          // a line comment with ( and ; and #define ICPMI_NOR_THIS 2
#define ICPMI_NEGATIVE (-2)    /* ( */
#define ICPMI_HEX 0x1F
typedef struct icpmi_small_thing {
    const double* rows;        /* [count]; */
    int32_t pass, count;
    size_t bytes;
    float scale;
} icpmi_small_thing;
const char* icpmi_name(void);
int icpmi_say(const char* text, uint64_t seed);
size_t icpmi_size(const icpmi_small_thing* thing,
                  const int32_t* off,   /* ( */
                  int64_t n, uint32_t step, double x, void* stream);
#endif /* ICPMI_H */
"""


def test_reader_on_one_of_each_form():
    from icpmi import _header
    h = _header.read(SMALL)
    assert h.constants == {"PLAIN": 7, "NEGATIVE": -2, "HEX": 31}
    assert list(h.structs) == ["icpmi_small_thing"]
    thing = h.structs["icpmi_small_thing"]
    assert thing.__name__ == "SmallThing" and issubclass(thing, C.Structure)
    assert thing._fields_ == [("rows", C.c_void_p), ("pass_", C.c_int32), ("count", C.c_int32), ("bytes", C.c_size_t),
                              ("scale", C.c_float)]
    assert h.functions == {
        "icpmi_name": (C.c_char_p, []),
        "icpmi_say": (C.c_int, [C.c_char_p, C.c_uint64]),
        "icpmi_size": (C.c_size_t, [C.POINTER(thing), C.c_void_p, C.c_int64, C.c_uint32, C.c_double, C.c_void_p]),
    }
    assert list(h.functions) == ["icpmi_name", "icpmi_say", "icpmi_size"]                 # header order


@pytest.mark.parametrize("bad, names", [
    ("int icpmi_count(unsigned n);", r"line 4: no ctypes type for 'unsigned n'.*icpmi_count"),          # an unknown scalar type
    ("int icpmi_long(int32_t a,\n                 doubel* b);", r"line 5: no ctypes type for 'doubel\* b'"),   # ... pointee, 2nd line
    ("#define ICPMI_X (1 << 4)", r"line 4: .*one integer.*ICPMI_X \(1 << 4\)"),                       # not an integer
    ("#define ICPMI_X 010", r"line 4: .*one integer"),                                                  # octal: not read as 10
    ("extern int icpmi_x;", r"line 4: not a #define.*'extern int icpmi_x;'"),                           # a stray declaration
    ("int icpmi_open(int32_t n)", r"line 4: not a #define.*'int icpmi_open\(int32_t n\)'"),             # no `;`
    ("#define ICPMI_LIB_PATH 1", r"line 4: the name LIB_PATH is taken"),                                # a name of _lib's
    ("#define ICPMI_FIRST 1", r"line 4: the name FIRST is taken"),                                      # defined twice
    ("typedef struct icpmi_s { double *a, *b; } icpmi_s;", r"line 4: not a field declaration"),
    ("  int icpmi_indented(void);", r"line 4: a declaration starts in column 0"),
])
def test_reader_refuses_and_names_the_line(bad, names):
    from icpmi import _header, _lib
    assert {"LIB_PATH", "CSRC", "EXPORTS", "INFO_SLOTS", "_SIGS", "IcpmiError", "bind", "check"} <= _lib.OWN_NAMES
    text = "#define ICPMI_FIRST 0\n/* a comment\n   over two lines */\n%s\nint icpmi_last(void);\n"
    assert set(_header.read(text % "", reserved=_lib.OWN_NAMES).functions) == {"icpmi_last"}    # the frame itself is fine
    with pytest.raises(_header.HeaderError, match=names):
        _header.read(text % bad, reserved=_lib.OWN_NAMES)


def test_real_header_is_fully_accounted_for(tmp_path, monkeypatch):
    from icpmi import _header, _lib
    h = _header.read(open(HEADER).read(), reserved=_lib.OWN_NAMES)         # raises on anything it does not recognise
    assert sorted(h.functions) == declared_symbols() and _lib.EXPORTS == tuple(h.functions)
    spelled = lambda sigs: {n: (r.__name__, [a.__name__ for a in args]) for n, (r, args) in sigs.items()}   # noqa: E731
    assert spelled(_lib._SIGS) == spelled(h.functions)                     # (a second reading makes its own struct classes)
    assert h.constants and all(getattr(_lib, n) == v for n, v in h.constants.items())
    assert (_lib.OK, _lib.ERR_ARG, _lib.ERR_WORKSPACE, _lib.ERR_HIP, _lib.ERR_UNSUPPORTED) == (0, -1, -2, -3, -4)
    assert [c.__name__ for c in h.structs.values()] == ["IcpParams", "NnPlan", "History", "FeatureStore", "GridPlan"]
    assert all(issubclass(getattr(_lib, c.__name__), C.Structure) and getattr(_lib, c.__name__)._fields_ == c._fields_
               for c in h.structs.values())
    # a missing header is an error with the path, as a missing library is: there is no table to fall back on
    monkeypatch.setattr(_lib, "HEADER_PATH", str(tmp_path / "include" / "icpmi.h"))
    with pytest.raises(_lib.IcpmiError, match=r"include/icpmi\.h cannot be read"):
        _lib._read_header()


def test_struct_layout_against_the_c_compiler(tmp_path):
    """sizeof and offsetof of every field of every struct, as the host compiler lays the header out, against ctypes."""
    from icpmi import _header, _lib
    table = _header.read(open(HEADER).read()).structs                          # C name -> class; checked: the classes _lib uses
    c_name = {getattr(_lib, cls.__name__): name for name, cls in table.items()}
    structs = list(c_name)
    assert len(structs) == 5
    c_field = lambda f: f[:-1] if f.endswith("_") and keyword.iskeyword(f[:-1]) else f          # noqa: E731
    lines = ["#include <stdio.h>", '#include "icpmi.h"', "int main(void) {"]
    for cls in structs:
        lines.append(f'    printf("{c_name[cls]} %zu\\n", sizeof({c_name[cls]}));')
        lines += [f'    printf("{c_name[cls]}.{f} %zu\\n", offsetof({c_name[cls]}, {c_field(f)}));' for f, _ in cls._fields_]
    lines += ["    return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines) + "\n")
    cc = os.environ.get("CC", "gcc")                                           # oracle/Makefile's host compiler
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), "-o", str(tmp_path / "layout"),
                    str(tmp_path / "layout.c")], check=True, capture_output=True, text=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    compiler = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    binding = {}
    for cls in structs:
        binding[c_name[cls]] = C.sizeof(cls)
        binding.update({f"{c_name[cls]}.{f}": getattr(cls, f).offset for f, _ in cls._fields_})
    assert binding == compiler
    assert len(_lib.History._fields_) == 19 and len(_lib.FeatureStore._fields_) == 13 and C.sizeof(_lib.IcpParams) == 32


def test_bind_sets_the_types_on_a_second_handle(monkeypatch):
    import icpmi
    from icpmi import _lib
    icpmi.build()
    first = icpmi.lib()                                                        # torch first, then the library
    second = _lib.bind(_lib.LIB_PATH)
    assert second is not first and second.icpmi_version().decode().startswith("icpmi")
    # a size beyond 32 bits: a handle without the types returns it as a C int
    want = first.icpmi_grid_workspace_bytes(30000, 30000)
    assert want > 2 ** 32 and second.icpmi_grid_workspace_bytes(30000, 30000) == want
    assert second.icpmi_grid_workspace_bytes.restype is C.c_size_t
    assert C.CDLL(_lib.LIB_PATH).icpmi_grid_workspace_bytes(30000, 30000) != want

    cdll = C.CDLL

    class Older:
        """A build from before icpmi_pf_predict."""

        def __init__(self, path):
            self.handle = cdll(path)

        def __getattr__(self, name):
            if name == "icpmi_pf_predict":
                raise AttributeError(name)
            return getattr(self.handle, name)

    monkeypatch.setattr(_lib.C, "CDLL", Older)
    with pytest.raises(AttributeError, match="icpmi_pf_predict"):             # the product library: stale
        _lib.bind(_lib.LIB_PATH)
    older = _lib.bind(_lib.LIB_PATH, exported_only=True)                       # another build: what it exports
    assert older.icpmi_pf_workspace_bytes.restype is C.c_size_t
