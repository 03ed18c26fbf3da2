"""ctypes loader for librwkv7_hip.so (C ABI: include/rwkv7_hip.h).

The header is the single source of truth: its prototypes are parsed once and every entry point gets its
`restype` and `argtypes` at load, so call sites pass plain Python ints and floats and a 64-bit count, a float
or the Philox seed arrives as what the C side reads.

There is deliberately NO fallback: if the library is missing or a call fails, the caller gets an
exception.  Nothing in this package routes through oracle/ or through a CPU/eager re-implementation.
"""
import ctypes
import os
import re

# torch must be imported BEFORE librwkv7_hip.so is dlopen'ed: the .so needs libamdhip64.so.7, and the process
# must end up with exactly one HIP runtime -- the one PyTorch-ROCm bundles (torch/lib/libamdhip64.so, same
# SONAME).  Loaded the other way round, /opt/rocm's runtime gets in first, torch's libraries bind to it, and
# launches fail with hipErrorNoDevice (seen on the GPU box).
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("RWKV7_HIP_SO") or os.path.join(_HERE, "lib", "librwkv7_hip.so")   # override: A/B builds
HEADER = os.path.join(_HERE, "..", "include", "rwkv7_hip.h")

_ERR = {-1: "RWKV7_EINVAL: null pointer or non-positive size",
        -2: "RWKV7_ECHUNK: T must be a multiple of 16 (reference assert, wkv7_cuda.cu:136)",
        -3: "RWKV7_EHEAD: H*64 != C (reference assert, rwkv7_state_fwd_fp16.cu:61)",
        -4: "RWKV7_ESHAPE: unsupported size for a fused elementwise op"}

_CTYPES = {"int": ctypes.c_int, "long": ctypes.c_long, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
           "unsigned long long": ctypes.c_ulonglong, "rwkv7_stream_t": ctypes.c_void_p}

_lib = None
_protos = None


class Rwkv7HipError(RuntimeError):
    pass


def _ctype(decl, name):
    """The ctypes type of a return type or of one NAMED parameter.  Every pointer (struct pointers and `const T *const *`
    included) is a c_void_p, which takes None, an address, a ctypes array or byref(struct)."""
    if "*" in decl:
        return ctypes.c_void_p
    words = [w for w in decl.split() if w != "const"]
    try:
        return _CTYPES[" ".join(words)]
    except KeyError:
        raise Rwkv7HipError(f"{name}: no ctypes type for `{decl.strip()}`") from None


def parse_prototypes(text):
    """{name: (restype, [argtypes])} of every `rwkv7_*(...)` prototype in a header's text.  A prototype whose types cannot all be
    mapped, or one the pattern below does not take apart, raises: nothing declared is ever left untyped."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    protos = {}
    for ret, name, params in re.findall(r"([\w\s*]+?)\b(rwkv7_\w+)\s*\(([^()]*)\)\s*;", text):
        restype = ctypes.c_char_p if ret.split() == ["const", "char", "*"] else _ctype(ret, name)
        params = [] if params.strip() == "void" else params.split(",")
        # a parameter is `type name`: drop the name (the last identifier) before looking the type up
        protos[name] = (restype, [_ctype(re.sub(r"\w+\s*$", "", p), name) for p in params])
    declared = set(re.findall(r"\b(rwkv7_\w+)\s*\(", text))
    if declared != set(protos):
        raise Rwkv7HipError(f"prototypes not understood: {sorted(declared - set(protos))}")
    return protos


def prototypes():
    """parse_prototypes of include/rwkv7_hip.h."""
    global _protos
    if _protos is None:
        with open(HEADER) as f:
            _protos = parse_prototypes(f.read())
    return _protos


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise Rwkv7HipError(
                f"{SO_PATH} is missing: build it with `python -m rwkvtts_amd.build` "
                "(hipcc --offload-arch=gfx950).  There is no CPU/eager fallback for the HIP ops.")
        so = ctypes.CDLL(SO_PATH)
        for name, (restype, argtypes) in prototypes().items():
            fn = getattr(so, name, None)
            if fn is None:
                raise Rwkv7HipError(f"{SO_PATH} does not export {name}, which include/rwkv7_hip.h declares")
            fn.restype, fn.argtypes = restype, argtypes
        _lib = so
    return _lib


def version() -> str:
    return lib().rwkv7_version().decode()


def check(rc: int, what: str):
    if rc == 0:
        return
    if rc < 0:
        raise ValueError(f"{what}: {_ERR.get(rc, f'error {rc}')}")
    raise Rwkv7HipError(f"{what}: HIP error {rc} at launch")


def call(name, ref, *args):
    """Launch entry point `name` on the current stream of ref's device (ref: a tensor, or the torch.device itself) and raise unless
    it returns 0.  args: everything but the trailing stream; tensors go by address, None is NULL, ints and floats are converted by
    the argtypes."""
    fn = getattr(_lib or lib(), name)
    args = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    guard, dev = (torch.cuda.device_of(ref), ref.device) if isinstance(ref, torch.Tensor) else (torch.cuda.device(ref), ref)
    with guard:
        rc = fn(*args, torch.cuda.current_stream(dev).cuda_stream)
    if rc:
        check(rc, name)


def ptr_array(ts):
    """HOST array of the tensors' device addresses (None: NULL), for the `void *const *` parameters."""
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def exported_symbols():
    """Names declared in include/rwkv7_hip.h (parsed, so the header stays the single source of truth)."""
    return sorted(prototypes())
