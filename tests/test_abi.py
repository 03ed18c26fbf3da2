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


# ---- the fused row stages: what every entry refuses before a launch ------------------------------------------------------------
# One line per entry, parameters in the header's order as name:kind.  Kinds: P required pointer, O pointer that may be NULL on its
# own, Q pointer that may be NULL only together with others (the cases are spelled out per entry), N count that must be positive,
# D row width (a multiple of 64, at most 4096), M nmix, G host array of nmix gradient pointers, S15 / S19 host array gsum, E element
# count of relusq (positive multiple of 8), T32 row count that must be a positive multiple of 32, F float.
_PREP_IN = "rows:N D:D w_pre:P k:P v:P a_pre:P v_pre:Q v_first:Q mask:O k_k:P k_a:P"
_PREP_OUT = "d_wpre:P d_k:P d_v:P d_apre:P d_vpre:Q d_vfirst:Q"
_POST_IN = "rows:N D:D dout:P y:P r:P k:P v:P g:P gn_w:P gn_b:P r_k:P eps:F"
_LN_MIX = "B:N T:N D:D nmix:M x:P branch:Q gamma:P beta:O eps:F mask:O params:P x_out:Q out:P"
_FUSED_ENTRIES = {
    "mix_fwd": "B:N T:N D:D nmix:M x:P x_prev:O mask:O params:P out:P nblocks:N",
    "mix_bwd": "B:N T:N D:D nmix:M g:G x:P x_prev:O mask:O params:P dx:P dpart:P nblocks:N run_len:N",
    "tmix_prepare_fwd": _PREP_IN + " w:P k2:P v2:P ain:P bin:P nblocks:N",
    "tmix_prepare_bwd": _PREP_IN + " d_w:P d_k2:P d_v2:P d_ain:P d_bin:P " + _PREP_OUT + " dpart:P nblocks:N",
    "tmix_prepare_bwd_sum": _PREP_IN + " gsum:S15 " + _PREP_OUT + " d_r:P dpart:P nblocks:N",
    "tmix_prepare_bwd_sum_compact": _PREP_IN + " gsum:S19 " + _PREP_OUT + " d_r:P dpart:P nblocks:N",
    "add_ln_fwd": "rows:N D:D x:P branch:Q gamma:P beta:O eps:F x_out:Q h:P mean:P rstd:P nblocks:N",
    "add_ln_bwd": "rows:N D:D dh:P d_resid:O x1:P mean:P rstd:P gamma:P dx:P dpart:P nblocks:N",
    "add_ln_mix_fwd": _LN_MIX + " mean:P rstd:P nblocks:N run_len:N",
    "add_ln_mix_fwd_h": _LN_MIX + " h:P mean:P rstd:P nblocks:N run_len:N",
    "mix_add_ln_bwd": "B:N T:N D:D nmix:M g:G d_resid:O x1:P mean:P rstd:P gamma:P beta:O mask:O params:P dx:P dpart:P "
                      "nblocks:N run_len:N",
    "tmix_post_fwd": "rows:N D:D y:P r:P k:P v:P g:P gn_w:P gn_b:P r_k:P eps:F out:P nblocks:N",
    "tmix_post_bwd": _POST_IN + " d_y:P d_r:P d_k:P d_v:P d_g:P dpart:P nblocks:N",
    "tmix_post_bwd_compact": _POST_IN + " d_y:P dt:P d_g:P hscal:P dpart:P nblocks:N",
    "relusq_fwd": "n:E x:P y:P",
    "relusq_bwd": "n:E x:P dy:P dx:P",
    "relusq_bwd_s": "n:E s:P dy:P dx:P",
    "add_ln_mix_rows_fwd": "T:T32 D:D nmix:M x:P branch:Q gamma:P beta:O eps:F mask:O params:P prev_src:P last_dst:P x_prev_rd:O "
                           "x_prev:P x_out:Q out:P nblocks:N run_len:N",
}
# nmix values an entry has no kernel for, beside 2 (no entry has one), 0 and 7
_NO_NMIX = {"mix_add_ln_bwd": (3,), "add_ln_mix_rows_fwd": (3,)}
# gsum slots that must be set; every other slot may be NULL (include/rwkv7_hip.h: the second partials, d_vfirst_in, and for the
# compact entry the post tensors 4, 6, 13)
_GSUM_REQUIRED = {"S15": (0, 2, 4, 5, 6, 7, 9, 11, 13), "S19": (0, 2, 5, 7, 9, 11, 15, 16, 17, 18)}
_EINVAL, _ESHAPE = -1, -4
_BAD_D = 72   # the one broken rule of the cases that show a NULL is accepted: were the NULL refused too, the entry would answer -1


def _fused_cases(name, params):
    """[(label, {parameter: value}, expected code)]: each case breaks exactly one rule of a call that is otherwise valid."""
    kinds = dict(params)
    cases = []
    for p, kind in params:
        if kind == "P":
            cases.append((f"{p} NULL", {p: None}, _EINVAL))
        elif kind == "O":
            cases.append((f"{p} NULL is allowed", {p: None, "D": _BAD_D}, _ESHAPE))
        elif kind in ("N", "E", "T32"):
            cases += [(f"{p} = {v}", {p: v}, _EINVAL) for v in (0, -1)]
            if kind == "E":
                cases.append((f"{p} % 8 != 0", {p: 12}, _ESHAPE))
            if kind == "T32":
                cases.append((f"{p} % 32 != 0", {p: 48}, _ESHAPE))
        elif kind == "D":
            cases += [(f"{p} = {v}", {p: v}, _ESHAPE) for v in (0, 72, 4160)]
        elif kind == "M":
            cases += [(f"{p} = {v}", {p: v}, _ESHAPE) for v in (2, 0, 7) + _NO_NMIX.get(name, ())]
        elif kind == "G":
            cases.append((f"{p} NULL", {p: None}, _EINVAL))
            for i in range(6):
                arr = (ctypes.c_void_p * 6)(*([16] * 6))
                arr[i] = None
                cases.append((f"{p}[{i}] NULL, nmix = 6", {p: arr, "nmix": 6}, _EINVAL))
        elif kind in _GSUM_REQUIRED:
            n = int(kind[1:])
            cases.append((f"{p} NULL", {p: None}, _EINVAL))
            for i in range(n):
                arr = (ctypes.c_void_p * n)(*([16] * n))
                arr[i] = None
                if i in _GSUM_REQUIRED[kind]:
                    cases.append((f"{p}[{i}] NULL", {p: arr}, _EINVAL))
                else:
                    cases.append((f"{p}[{i}] NULL is allowed", {p: arr, "D": _BAD_D}, _ESHAPE))
    if "branch" in kinds:
        cases += [("branch without x_out", {"x_out": None}, _EINVAL),
                  ("x_out without branch is allowed", {"branch": None, "D": _BAD_D}, _ESHAPE),
                  ("neither branch nor x_out is allowed", {"branch": None, "x_out": None, "D": _BAD_D}, _ESHAPE)]
    if "v_pre" in kinds:
        absent = {"v_pre": None, "v_first": None}
        cases += [("v_pre without v_first", {"v_first": None}, _EINVAL), ("v_first without v_pre", {"v_pre": None}, _EINVAL)]
        if "d_vpre" in kinds:
            absent.update(d_vpre=None, d_vfirst=None)
            cases += [("v_pre without d_vpre", {"d_vpre": None}, _EINVAL), ("v_pre without d_vfirst", {"d_vfirst": None}, _EINVAL),
                      ("d_vpre and d_vfirst without v_pre are allowed", {"v_pre": None, "v_first": None, "D": _BAD_D}, _ESHAPE)]
        cases.append(("layer 0 (no value residual) is allowed", dict(absent, D=_BAD_D), _ESHAPE))
    return cases


def _fused_valid(kind):
    one = ctypes.c_void_p(16)  # never dereferenced: every case is refused before a launch
    if kind in ("P", "O", "Q"):
        return one
    if kind == "G":
        return (ctypes.c_void_p * 6)(*([16] * 6))
    if kind in _GSUM_REQUIRED:
        return (ctypes.c_void_p * int(kind[1:]))(*([16] * int(kind[1:])))
    return {"N": 4, "D": 64, "M": 1, "E": 64, "T32": 32, "F": 1e-5}[kind]


@pytest.mark.parametrize("name,sfx", [(n, s) for n in sorted(_FUSED_ENTRIES) for s in ("bf16", "f32")
                                      if (n, s) != ("add_ln_mix_rows_fwd", "f32")])   # the packed-rows entry exists in bf16 only
def test_fused_stage_entries_refuse_before_launch(hip_lib, name, sfx):
    """Every fused row-stage entry, one broken rule per call, answers the code include/rwkv7_hip.h gives for that rule: RWKV7_EINVAL
    (-1) for a missing pointer or a count below 1, RWKV7_ESHAPE (-4) for a size no kernel exists for.  Nothing is launched."""
    fn = getattr(hip_lib, f"rwkv7_{name}_{sfx}")
    params = [tuple(p.split(":")) for p in _FUSED_ENTRIES[name].split()]
    assert len(fn.argtypes) == len(params) + 1, "the table's parameter list is not the header's"
    cases = _fused_cases(name, params)
    assert len({label for label, _, _ in cases}) == len(cases)
    wrong = []
    for label, change, want in cases:
        assert set(change) <= {p for p, _ in params}
        args = [change[p] if p in change else _fused_valid(kind) for p, kind in params]
        got = fn(*args, None)
        if got != want:
            wrong.append(f"{label}: {got}, expected {want}")
    assert not wrong, f"rwkv7_{name}_{sfx}: " + "; ".join(wrong)
