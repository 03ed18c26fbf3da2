"""CPU: the C-ABI library builds for gfx950, loads without a GPU, exports every symbol that
include/rwkv7_hip.h declares, and rejects bad arguments before launching anything."""
import ctypes
import os
import subprocess

import pytest
import torch

from rwkvtts_amd import _lib, build


def test_library_builds_and_loads(hip_lib):
    assert os.path.exists(build.SO)
    v = _lib.version()
    assert v.startswith("rwkv7_hip") and "gfx950" in v


def test_every_declared_symbol_is_exported(hip_lib):
    names = _lib.exported_symbols()
    assert "rwkv7_wkv_fwd_bf16" in names and "rwkv7_wkv_bwd_bf16" in names and "rwkv7_wkv_state_fwd_bf16" in names
    for n in names:
        assert hasattr(hip_lib, n), f"{n} declared in include/rwkv7_hip.h but not exported"


def test_code_object_is_gfx950(hip_lib):
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", build.SO], capture_output=True, text=True)
    if out.returncode != 0:
        pytest.skip("llvm-readelf unavailable")
    blob = open(build.SO, "rb").read()
    assert b"gfx950" in blob


def test_argument_errors_do_not_launch(hip_lib):
    one = ctypes.c_void_p(16)  # never dereferenced: the checks fire first
    # T % 16 != 0 -> RWKV7_ECHUNK (reference: assert at wkv7_cuda.cu:136)
    assert hip_lib.rwkv7_wkv_fwd_bf16(1, 15, 1, one, one, one, one, one, one, one, one, one, None) == -2
    assert hip_lib.rwkv7_wkv_bwd_bf16(1, 17, 1, *([one] * 15), None) == -2
    # null pointer -> RWKV7_EINVAL
    assert hip_lib.rwkv7_wkv_fwd_f32(1, 16, 1, None, one, one, one, one, one, one, None, None, None) == -1
    # s without sa -> RWKV7_EINVAL
    assert hip_lib.rwkv7_wkv_fwd_f32(1, 16, 1, one, one, one, one, one, one, one, one, None, None) == -1
    # H*64 != C -> RWKV7_EHEAD (reference: assert at rwkv7_state_fwd_fp16.cu:61)
    assert hip_lib.rwkv7_wkv_state_fwd_bf16(1, 1, 100, 2, one, one, one, one, one, one, one, one, None) == -3
    assert hip_lib.rwkv7_wkv_state_fwd_bf16(0, 1, 128, 2, one, one, one, one, one, one, one, one, None) == -1
    # the row-split backward and the fused stages validate the same way
    two = (ctypes.c_void_p * 2)(16, 16)
    assert hip_lib.rwkv7_wkv_bwd_split_bf16(1, 24, 1, *([one] * 9), two, two, two, one, two, two, None) == -2
    bad = (ctypes.c_void_p * 2)(16, None)
    assert hip_lib.rwkv7_wkv_bwd_split_bf16(1, 16, 1, *([one] * 9), two, bad, two, one, two, two, None) == -1
    assert hip_lib.rwkv7_add_ln_fwd_bf16(ctypes.c_long(4), 100, one, None, one, None, ctypes.c_float(1e-5), None, one, one,
                                         one, 4, None) == -4          # D % 64 != 0 -> RWKV7_ESHAPE


def test_workspace_query(hip_lib):
    s, sa = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip_lib.rwkv7_wkv_workspace_bytes(8, 4096, 16, ctypes.byref(s), ctypes.byref(sa)) == 0
    assert s.value == 8 * 16 * 256 * 64 * 64 * 4 and sa.value == 8 * 4096 * 16 * 64 * 4   # 512 MiB / 128 MiB, SURVEY 8(a) a1
    assert hip_lib.rwkv7_wkv_workspace_bytes(8, 4097, 16, ctypes.byref(s), ctypes.byref(sa)) == -2


def test_reference_op_namespaces_exist_and_refuse_cpu():
    from rwkvtts_amd import ops
    for ns, name in (("wind_backstepping", "forward"), ("wind_backstepping", "backward"),
                     ("rwkv7_state_fwd_fp16", "forward"), ("wkv7s", "forward")):
        assert hasattr(getattr(torch.ops, ns), name)
    x = torch.zeros(1, 16, 1, 64, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError):  # CUDA(HIP)-only dispatch, as in wkv7_op.cpp:26-29
        ops.WindBackstepping.apply(x, x, x, x, x, x)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "SO_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.Rwkv7HipError):
        _lib.lib()


# ---- typed bindings: every prototype of the header is applied to the loaded library -------------------------------------------
_HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "rwkv7_hip.h")
_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
            "unsigned long long": ctypes.c_ulonglong, "rwkv7_stream_t": ctypes.c_void_p}


def _header_text():
    import re
    return re.sub(r"/\*.*?\*/", " ", open(_HEADER).read(), flags=re.S)


def test_every_declared_function_is_fully_typed(hip_lib):
    """Counted from the header's text, not through _lib's parser: each declared function carries one argtype per declared parameter
    (pointers and the stream as c_void_p, scalars as the header's own type) and the declared restype."""
    import re
    decls = re.findall(r"([\w \t*]+?)\b(rwkv7_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", _header_text())
    names = sorted(set(re.findall(r"\b(rwkv7_[a-z0-9_]+)\s*\(", _header_text())))
    assert names == _lib.exported_symbols() == sorted(d[1] for d in decls) and len(names) >= 110
    for ret, name, params in decls:
        fn = getattr(hip_lib, name)
        params = [] if params.strip() == "void" else [" ".join(p.replace("const", " ").split()) for p in params.split(",")]
        want = [ctypes.c_void_p if "*" in p else _SCALARS[p.rsplit(" ", 1)[0]] for p in params]
        assert list(fn.argtypes) == want, name
        ret = " ".join(ret.split())
        assert fn.restype is (ctypes.c_char_p if ret == "const char *" else _SCALARS[ret]), name


def test_parser_refuses_what_it_cannot_type():
    good = "/* int rwkv7_in_a_comment(double x); */\nint rwkv7_ok(long n, const void *const *p, rwkv7_stream_t stream);\n"
    assert _lib.parse_prototypes(good) == {"rwkv7_ok": (ctypes.c_int, [ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p])}
    for bad in ("int rwkv7_bad(int n, double x, rwkv7_stream_t stream);",      # a parameter type outside the table
                "short rwkv7_bad(int n);",                                     # a return type outside the table
                "int rwkv7_bad(int n, int (*cb)(int));",                       # a shape the pattern does not take apart
                "int rwkv7_bad(int, float x);"):                               # an unnamed parameter
        with pytest.raises(_lib.Rwkv7HipError):
            _lib.parse_prototypes(good + bad)


def test_wrong_argument_types_are_refused(hip_lib):
    one = ctypes.c_void_p(16)  # never dereferenced: the checks fire first
    f = hip_lib.rwkv7_wkv_fwd_bf16
    assert f(1, 15, 1, *([one] * 9), None) == -2
    for T in ("15", 15.0, ctypes.c_long(15)):
        with pytest.raises(ctypes.ArgumentError):
            f(1, T, 1, *([one] * 9), None)
    with pytest.raises(ctypes.ArgumentError):
        hip_lib.rwkv7_add_ln_fwd_bf16(4, 100, one, None, one, None, "1e-5", None, one, one, one, 4, None)   # a str for a float


def test_64_bit_counts_arrive_whole(hip_lib):
    big, small = hip_lib.rwkv7_grad_sumsq_workspace_bytes(2 ** 33), hip_lib.rwkv7_grad_sumsq_workspace_bytes(2 ** 31 - 1)
    assert big > 0 and big >= small > 0


def test_ptr_array():
    a, b = torch.zeros(3), torch.zeros(2)
    arr = _lib.ptr_array([a, None, b])
    assert list(arr) == [a.data_ptr(), None, b.data_ptr()] and ctypes.sizeof(arr) == 3 * ctypes.sizeof(ctypes.c_void_p)


def _header_structs():
    """{struct name: [field names in order]} of every `typedef struct` in the header."""
    import re
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s+\w+\s*\{(.*?)\}\s*(\w+)\s*;", _header_text(), flags=re.S):
        out[name] = [re.search(r"(\w+)\s*(?:\[\w+\])?\s*$", d).group(1) for decl in body.split(";") for d in decl.split(",") if d.strip()]
    return out


def test_struct_mirrors_match_the_compiler(tmp_path):
    """The five ctypes.Structure classes against what a C compiler makes of the header: same field names in the same order, same
    offsets, same field sizes, same total size.  The field list comes from the header's text, so a new field cannot be left out."""
    import shutil
    from rwkvtts_amd import continuous, continuous_cosy, continuous_xy, decode, sampling
    mirrors = {"rwkv7_decode_dims": decode._Dims, "rwkv7_sample_tail": sampling.SampleTail, "rwkv7_slot_state": continuous.SlotState,
               "rwkv7_xy_slot_state": continuous_xy.XYSlotState, "rwkv7_ras_slot_state": continuous_cosy.RasSlotState}
    structs = _header_structs()
    assert sorted(structs) == sorted(mirrors), "a struct of the header has no checked Python mirror (or the other way round)"
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "rwkv7_hip.h"', "int main(void) {"]
    for s, fields in structs.items():
        lines.append(f'  printf("{s} . %zu 0\\n", sizeof({s}));')
        lines += [f'  printf("{s} {f} %zu %zu\\n", offsetof({s}, {f}), sizeof((({s} *)0)->{f}));' for f in fields]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/lib/llvm/bin/clang"
    subprocess.run([cc, "-I", os.path.dirname(_HEADER), str(src), "-o", str(exe)], check=True, capture_output=True)
    c_side = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n"):
        if line:
            s, f, off, size = line.split()
            c_side.setdefault(s, []).append((f, int(off), int(size)))
    for s, cls in mirrors.items():
        py_side = [(".", ctypes.sizeof(cls), 0)] + [(n, getattr(cls, n).offset, getattr(cls, n).size) for n, *_ in cls._fields_]
        assert py_side == c_side[s], s
