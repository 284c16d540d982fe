"""ctypes binding of libl4p_hip.so (C ABI declared in include/l4p_hip.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C l4p_amd/csrc`` into
``l4p_amd/lib/``.  There is no fallback: if the shared object is missing or a symbol cannot be
resolved, importing the engine raises.

Nothing of the ABI is restated here: the constants, the five structs and the 100-odd signatures are read from the header by
``_header`` (the C-to-ctypes mapping is stated there).  A new ABI function is declared in the header and bound from it; only
``ABI_VERSION`` is a literal, because the header states that number in a comment.  Pointers to plain data are ``c_void_p``
whether they point into device or host memory - the header does not tell them apart - so a host out-parameter takes
``byref(...)``, a ctypes array, ``None`` or an address, and ctypes does not check its pointee type.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

from . import _header

ABI_VERSION = 26  # what l4p_abi_version() of the library this binding was written against returns (include/l4p_hip.h)

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "l4p_hip.h")
# L4P_HIP_LIB: another build of the same library (tuning aid: A/B of two builds inside one GPU call)
LIB_PATH = os.environ.get("L4P_HIP_LIB") or os.path.join(_HERE, "lib", "libl4p_hip.so")

# The header is read once per process, here: a declaration its reader does not understand fails the import.
with open(HEADER_PATH) as _fh:
    HEADER = _header.parse(_fh.read())
_binding = _header.bind(HEADER)

# Every #define by its header name (L4P_F16: IEEE half storage / f16 MFMA, the arithmetic class of the reference's "16-mixed");
# the epilogue, activation and ground-truth field codes also without the prefix (EPI_DENSE, ACT_GELU, GT_BILINEAR, ...).
globals().update(HEADER.constants)
globals().update({k[4:]: v for k, v in HEADER.constants.items() if k.startswith(("L4P_EPI_", "L4P_ACT_", "L4P_GT_"))})

# The classes the prototypes point to: byref(GemmDesc()) is what l4p_gemm's argtypes ask for.
GemmDesc = _binding.structs["l4p_gemm_desc"]
EncoderCfg = _binding.structs["l4p_encoder_cfg"]
DptCfg = _binding.structs["l4p_dpt_cfg"]
TrackCfg = _binding.structs["l4p_track_cfg"]
GtField = _binding.structs["l4p_gt_field"]

SIGNATURES = _binding.signatures  # name -> (restype, argtypes) of every function the header declares

_lib: Optional[C.CDLL] = None


class L4PHipError(RuntimeError):
    pass


def load() -> C.CDLL:
    """Load libl4p_hip.so and bind every declared symbol.  Raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise L4PHipError(
            f"{LIB_PATH} not found — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C l4p_amd/csrc`. There is no CPU/eager fallback."
        )
    # PyTorch-ROCm bundles its own libamdhip64 and must be the FIRST to load one: the library then binds to that runtime
    # by soname.  Loaded the other way round (our /opt/rocm copy first, torch's afterwards) the process holds two HIP
    # runtimes and hipSetDevice in ours reports "no ROCm-capable device" (measured: build() followed by smoke()).
    import torch  # noqa: F401

    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    have = int(lib.l4p_abi_version())
    if have != ABI_VERSION:
        raise L4PHipError(f"{LIB_PATH} reports ABI version {have}, this package binds version {ABI_VERSION}: "
                          "stale library - rebuild it with `make -C l4p_amd/csrc`")
    _lib = lib
    return lib


def kernel_tree_hash() -> str:
    """sha1 over the kernel sources and the C header (file names + contents, sorted): ties a measurement artefact (the PMC traffic
    file under profiles/) to the kernels it was taken on - bench.py attaches `roofline.traffic` only when the hashes agree."""
    import hashlib

    files = sorted(os.path.join(_HERE, "csrc", f) for f in os.listdir(os.path.join(_HERE, "csrc"))
                   if f.endswith((".hip", ".hpp", ".inc")))
    files.append(HEADER_PATH)
    h = hashlib.sha1()
    for f in files:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


knob_epoch = 0  # bumped by set_knob: what was derived from the knobs (Engine's tracker workspace sizes) is stale when it moved


def set_knob(name: str, value: int) -> None:
    """Dispatch knob of the native launchers (include/l4p_hip.h: "conv_halo", "gemm_4w", "track_fold_i2t", ...)."""
    global knob_epoch
    check(load().l4p_set_knob(name.encode(), int(value)), f"l4p_set_knob({name})")
    knob_epoch += 1


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().l4p_last_error().decode("utf-8", "replace")
        raise L4PHipError(f"{what or 'l4p_hip call'} failed (rc={rc}): {msg}")
