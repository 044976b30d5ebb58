"""ctypes binding of libicpmi.so, derived from include/icpmi.h (read once, at import, by icpmi/_header.py).

Every ``#define ICPMI_<NAME>`` of the header is the module attribute ``<NAME>`` here, every struct a ``ctypes.Structure``
class (``icpmi_icp_params`` -> ``IcpParams``) and every prototype an entry of ``_SIGS``: nothing of the header is
restated by hand.

There is no CPU fallback: if the shared library is missing or a call fails the
caller gets an exception, never a silently different code path.
"""
import ctypes as C
import os
import subprocess

from . import _header

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(_PKG, "csrc")
LIB_PATH = os.path.join(_PKG, "lib", "libicpmi.so")
HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "icpmi.h")

# names of the slots INFO_H .. INFO_STATUS of an information record, for the Python layer's dictionaries (not in the header)
INFO_SLOTS = ("H_tt", "H_tx", "H_ty", "H_xx", "H_xy", "H_yy", "g_t", "g_x", "g_y", "sse", "inliers", "rows", "status")


class IcpmiError(RuntimeError):
    pass


def build(verbose=False):
    """Compile the HIP sources for gfx950 into lib/libicpmi.so (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "-j4", "all"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise IcpmiError("building libicpmi.so failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
    if verbose:
        print(r.stdout)
    return LIB_PATH


def bind(path, exported_only=False):
    """CDLL(path) with the header's restype and argtypes on every entry.  A name the library lacks raises AttributeError
    (the .so is stale) unless ``exported_only``: then what it exports is bound and the rest left out (an older build)."""
    L = C.CDLL(path)
    for name, (res, args) in _SIGS.items():
        if exported_only and not hasattr(L, name):
            continue
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    return L


_lib = None


def lib():
    """The loaded library; raises IcpmiError when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise IcpmiError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                             "(or `make -C iterative-closest-point-avmi_amd/csrc`). There is no CPU fallback.")
        # torch first: it ships its own HIP runtime (libamdhip64 inside the wheel), and the process must hold ONE — the
        # streams and allocations torch hands us have to belong to the runtime our launches go through.  Loaded before
        # torch, libicpmi.so would bring in /opt/rocm's copy and torch its own beside it: every launch then fails with
        # a HIP runtime error (seen: build() followed by smoke() in one process).
        import torch  # noqa: F401
        _lib = bind(LIB_PATH)
        why = runtime_problem()
        if why:
            _lib = None
            raise IcpmiError(why)
    return _lib


def runtime_problem():
    """'' or what icpmi_runtime_check found: two copies of libamdhip64 mapped into this process (every launch would fail)."""
    if _lib is None:
        return ""
    buf = C.create_string_buffer(1024)
    return buf.value.decode() if _lib.icpmi_runtime_check(buf, len(buf)) != OK else ""


def check(code, what):
    if code != OK:
        hint = runtime_problem() if code == ERR_HIP else ""
        raise IcpmiError(f"{what}: {lib().icpmi_strerror(code).decode()} ({code})" + (f" [{hint}]" if hint else ""))


def set_option(name, value):
    """icpmi_set_option: change one of the library's ICPMI_* switches after it has read the environment (None unsets)."""
    check(lib().icpmi_set_option(name.encode(), None if value is None else str(value).encode()), f"set_option({name})")


def shutdown():
    """icpmi_shutdown: destroy the side streams and events the library made (made again on demand)."""
    if _lib is not None:
        check(_lib.icpmi_shutdown(), "shutdown")


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            return f.read()
    except OSError as e:
        raise IcpmiError(f"{HEADER_PATH} cannot be read ({e.strerror}): the binding is derived from it, and there is "
                         "no table to fall back on.") from None


# Last, so that every name this module owns is there to be refused to a constant of the header.  Published: OK, ERR_*,
# ST_*, RES_*, GM_*, ...; IcpParams, NnPlan, History, FeatureStore, GridPlan; _SIGS, {name: (restype, argtypes)}, and EXPORTS.
OWN_NAMES = frozenset(globals()) | {"OWN_NAMES", "EXPORTS", "_SIGS"}
_constants, _structs, _SIGS = _header.read(_read_header(), reserved=OWN_NAMES)
EXPORTS = tuple(_SIGS)
globals().update(_constants)
globals().update({cls.__name__: cls for cls in _structs.values()})
