"""ctypes binding of libfragnet_hip.so (C-ABI in include/fragnet_hip.h).

The binding is read from the header at import (_header.py): every struct, constant and signature below is what the header says,
nothing is restated here.  There is no fallback: if the library or the header is missing or a call fails, this raises.  The
shared object is built in-tree by ``__graft_entry__.build()`` / ``python -m fragnet_amd.build`` into fragnet_amd/lib/.
"""
from __future__ import annotations

import ctypes as C
import os

from ._header import FragnetHipError, camel, parse
from .build import HEADERS

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libfragnet_hip.so")


def _read_header():
    try:
        with open(HEADERS[0]) as f:
            return parse(f.read())
    except OSError as e:
        raise FragnetHipError(f"the binding is read from the library's header, looked for at {HEADERS[0]}: {e}") from e


HEADER = _read_header()
# every #define FN_X <integer> under both spellings in use: FN_D, FN_MAX_PART, ... and ABI_VERSION, STAGE_ROWS, ACT_RELU, TUNE_MOL_TAIL, ...
globals().update({key: v for name, v in HEADER.constants.items() for key in (name, name[len("FN_"):])})
# every typedef struct fn_x as the class X: CsrTask, GatPlan, Encoder, ...
globals().update({camel(name): cls for name, cls in HEADER.structs.items()})
LAYER_FIELDS = tuple(name for name, _ in HEADER.structs["fn_layer_weights"]._fields_)
# name -> argtypes; the return types (int: 0 ok / <0 argument error / >0 hipError_t, unless declared otherwise) are set in load()
SIGNATURES = {name: argtypes for name, (_, argtypes) in HEADER.functions.items()}

_lib = None


def load():
    """Loads the shared library once; raises FragnetHipError (never falls back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FragnetHipError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). fragnet_amd has no CPU/PyTorch fallback for its kernels.")
    # a library older than its sources is refused, not used: the digest of the .hip / .inc / .h files is stored next to it
    from . import build
    if os.path.isdir(os.path.join(build.HERE, "csrc")) and build.stale():
        raise FragnetHipError(
            f"{LIB_PATH} does not match the sources it was built from (content digest differs): rebuild it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or fragnet_amd.build.build_lib()).")
    # torch ships its own libamdhip64; it must be the HIP runtime this library binds to (same streams,
    # same allocations), so torch is imported before the dlopen.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in HEADER.functions.items():
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch
        fn.argtypes, fn.restype = argtypes, restype
    if lib.fn_abi_version() != HEADER.constants["FN_ABI_VERSION"]:
        raise FragnetHipError(f"ABI version mismatch: library {lib.fn_abi_version()}, "
                              f"binding {HEADER.constants['FN_ABI_VERSION']}")
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().fn_last_error()
        raise FragnetHipError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")


def call(name: str, *args):
    check(getattr(load(), name)(*args), name)
