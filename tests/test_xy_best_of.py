"""CPU: best-of-n in the XY engine, the pieces that need no device -- the C ABI of rwkv7_xy_slots_draw_lp_f32 and
rwkv7_xy_slots_frame_lp_bf16 (declared in include/rwkv7_hip.h, typed from it, exported, rwkv7_xy_slot_logprob's Python mirror
against the compiler's layout, RWKV7_EINVAL / RWKV7_ESHAPE before any launch), ContinuousXYDecoder's new interface and its argument
checks, the shared fan-out helper, and GroupScheduler driven with the requests the XY engine queues."""
import ctypes
import inspect
import os
import shutil
import subprocess

import pytest

from rwkvtts_amd import _lib
from rwkvtts_amd import continuous, continuous_cosy
from rwkvtts_amd import continuous_xy as cx
from rwkvtts_amd.continuous import GroupScheduler, candidate_seed

DRAW, FRAME = "rwkv7_xy_slots_draw_lp_f32", "rwkv7_xy_slots_frame_lp_bf16"
LP_FIELDS = ["ch_lp", "frame_lp", "cum_lp", "n_lp"]


# ---------------------------------------------------------------------------------------------------------------- 1. ABI
def test_header_declares_the_entries_and_the_struct():
    text = open(_lib.HEADER).read()
    assert DRAW in _lib.exported_symbols() and FRAME in _lib.exported_symbols()
    assert "struct rwkv7_xy_slot_logprob {" in text and "typedef struct rwkv7_xy_slot_logprob rwkv7_xy_slot_logprob;" in text


def test_library_exports_the_entries_with_the_headers_types(hip_lib):
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    protos = _lib.prototypes()
    # rows, logits, ld, row_slot, seg_off, seg_len, allow_lo, allow_hi, max_domain, st, lp, stream
    assert protos[DRAW] == (ctypes.c_int, [I, P, L, P, P, P, P, P, I, P, P, P])
    # rows, row_slot, st, lp, stream
    assert protos[FRAME] == (ctypes.c_int, [I, P, P, P, P])
    for name, plain in ((DRAW, "rwkv7_xy_slots_draw_f32"), (FRAME, "rwkv7_xy_slots_frame_bf16")):
        restype, argtypes = protos[name]
        assert argtypes[:-2] == protos[plain][1][:-1]                      # the plain entry's arguments, then lp, then the stream
        fn = getattr(hip_lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes


def test_xy_slot_logprob_mirror_matches_the_compiler(tmp_path):
    assert [n for n, _ in cx.XYSlotLogprob._fields_] == LP_FIELDS
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "rwkv7_hip.h"', "int main(void) {",
             '  printf(". %zu 0\\n", sizeof(rwkv7_xy_slot_logprob));']
    lines += [f'  printf("{f} %zu %zu\\n", offsetof(rwkv7_xy_slot_logprob, {f}), sizeof(((rwkv7_xy_slot_logprob *)0)->{f}));'
              for f in LP_FIELDS]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    cc_ = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/lib/llvm/bin/clang"
    subprocess.run([cc_, "-I", os.path.dirname(os.path.abspath(_lib.HEADER)), str(src), "-o", str(exe)], check=True, capture_output=True)
    c_side = [(f, int(off), int(size)) for f, off, size in
              (line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n") if line)]
    py_side = [(".", ctypes.sizeof(cx.XYSlotLogprob), 0)] + [(n, getattr(cx.XYSlotLogprob, n).offset, getattr(cx.XYSlotLogprob, n).size)
                                                             for n in LP_FIELDS]
    assert py_side == c_side


def test_argument_errors_do_not_launch(hip_lib):
    one = 16   # never dereferenced: the checks fire first
    p = ctypes.c_void_p
    per_slot = ("step", "limit", "seed", "inv_temp", "top_k", "top_p", "do_sample", "live", "needs", "nt", "row", "seq", "x")

    def state(**kw):
        st = cx.XYSlotState()
        for f in per_slot:
            setattr(st, f, one)
        st.seq_ld, st.D, st.C, st.slots, st.top_k_max = 8, 128, 4, 32, 64
        for c in range(16):
            st.tables[c] = one
        st.text_shift, st.speech_vocab, st.pad, st.eos0, st.eos_list, st.n_eos = 100, 16, 15, -1, None, 0
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    all_lp = (one,) * 4
    ref = lambda x: None if x is None else ctypes.byref(x)
    lp_ref = lambda lp: None if lp is None else ctypes.byref(cx.XYSlotLogprob(*lp))

    def draw(st, lp=all_lp, rows=1, logits=one, seg=one, lo=one, hi=one, dom=16):
        return getattr(hip_lib, DRAW)(rows, p(logits), ctypes.c_long(64), None, p(seg), p(seg), p(lo), p(hi), dom, ref(st), lp_ref(lp), None)

    def frame(st, lp=all_lp, rows=1):
        return getattr(hip_lib, FRAME)(rows, None, ref(st), lp_ref(lp), None)

    EINVAL, ESHAPE = -1, -4
    # the new argument: a null lp and each null member, for both entries
    assert draw(state(), lp=None) == EINVAL and frame(state(), lp=None) == EINVAL
    for k in range(4):
        lp = tuple(None if i == k else one for i in range(4))
        assert draw(state(), lp=lp) == EINVAL and frame(state(), lp=lp) == EINVAL, LP_FIELDS[k]
    assert draw(state(), lp=None, dom=15361) == EINVAL and frame(state(C=17), lp=None) == EINVAL   # ... looked at before the shapes
    # every case the plain entries refuse
    assert draw(None) == EINVAL and frame(None) == EINVAL
    assert draw(state(), rows=0) == EINVAL and frame(state(), rows=0) == EINVAL
    assert draw(state(), logits=None) == EINVAL and draw(state(), seg=None) == EINVAL and draw(state(), dom=0) == EINVAL
    assert draw(state(), lo=None) == EINVAL                      # allow_lo without allow_hi
    for name in per_slot:
        assert draw(state(**{name: None})) == EINVAL and frame(state(**{name: None})) == EINVAL, name
    for bad in (dict(seq_ld=0), dict(slots=0), dict(C=0), dict(D=0), dict(n_eos=1)):
        assert draw(state(**bad)) == EINVAL and frame(state(**bad)) == EINVAL, bad
    st = state()
    st.tables[3] = None
    assert draw(st) == EINVAL and frame(st) == EINVAL
    assert draw(state(), dom=15361) == ESHAPE
    assert draw(state(top_k_max=65)) == ESHAPE and draw(state(top_k_max=-1)) == ESHAPE
    assert draw(state(C=17)) == ESHAPE and frame(state(C=17)) == ESHAPE
    assert draw(state(D=100)) == ESHAPE and frame(state(D=100)) == ESHAPE


# ---------------------------------------------------------------------------------------------------------------- 2. engine interface
def _engine_shell(slots, logprobs=False, cap=64):
    """A ContinuousXYDecoder with nothing but what the argument checks read: they come before anything touches the device."""
    eng = object.__new__(cx.ContinuousXYDecoder)
    eng.slots, eng.cap, eng.logprobs, eng._lp_done = slots, cap, logprobs, {}
    eng.sched = cx.GroupScheduler(slots)
    return eng


def test_the_engine_has_submit_n_and_take_logprobs():
    eng = cx.ContinuousXYDecoder
    assert callable(eng.submit_n) and callable(eng.take_logprobs)
    sub, sub_n = inspect.signature(eng.submit).parameters, inspect.signature(eng.submit_n).parameters
    assert list(sub_n)[:2] == ["self", "n"] and set(sub) - {"self"} <= set(sub_n)          # submit()'s arguments, the seed included
    assert all(sub[k].default == sub_n[k].default for k in sub if k != "self")
    assert inspect.signature(eng.__init__).parameters["logprobs"].default is False
    assert eng.logprobs is False and eng.lp is None
    draw, frame = inspect.signature(cx.xy_slots_draw).parameters, inspect.signature(cx.xy_slots_frame).parameters
    assert draw["lp"].default is None and frame["lp"].default is None                      # the plain entries stay the default


def test_submit_n_and_take_logprobs_argument_checks():
    for n in (0, -1, 5):
        eng = _engine_shell(4)
        with pytest.raises(ValueError, match="slots"):
            eng.submit_n(n, None, seed=3)
        assert not eng.sched.pending, "a refused group leaves nothing in the queue"
    eng = _engine_shell(4)
    with pytest.raises(ValueError, match="seed"):
        eng.submit_n(2, None)                                                              # n > 1 without a seed
    with pytest.raises(ValueError, match="max_new_frames"):
        eng.submit_n(2, None, max_new_frames=65, seed=1)                                   # submit()'s checks, before anything is queued
    assert not eng.sched.pending
    with pytest.raises(ValueError, match="logprobs=True"):
        _engine_shell(4).take_logprobs(0)
    with pytest.raises(KeyError):
        _engine_shell(4, logprobs=True).take_logprobs(0)


def test_one_fan_out_for_the_three_engines():
    """the row copy of submit_n is continuous.fan_out_rows in every engine, not a copy per engine"""
    assert cx.fan_out_rows is continuous.fan_out_rows is continuous_cosy.fan_out_rows
    for eng in (continuous.ContinuousDecoder, continuous_cosy.ContinuousCosyDecoder, cx.ContinuousXYDecoder):
        assert "fan_out_rows(" in inspect.getsource(eng._fan_out), eng.__name__


# ---------------------------------------------------------------------------------------------------------------- 3. scheduler
def _xy_fields(budget=12):
    """What ContinuousXYDecoder queues for one prompt (its _request_fields), with a stand-in for the embeddings."""
    return dict(embeds=None, max_new_tokens=budget, do_sample=True, temperature=0.8, top_k=50, top_p=0.95)


def test_group_scheduler_with_xy_requests_admits_groups_whole_and_fifo():
    assert cx.GroupScheduler is GroupScheduler and cx.candidate_seed is candidate_seed     # the engine's scheduler and keys are the shared ones
    s = GroupScheduler(4)
    seeds = [candidate_seed((1 << 64) - 1, i) for i in range(3)]
    assert seeds == [(1 << 64) - 1, 0, 1]                                  # the keys wrap
    group = s.submit_group(3, seeds, **_xy_fields())
    took = s.admit()                                                       # 4 free slots: the group of 3, whole
    assert [r.handle for _, r in took] == group and [slot for slot, _ in took] == [0, 1, 2] and s.free == [3]
    assert [r.seed for _, r in took] == seeds
    assert [r.leader for _, r in took] == [None, group[0], group[0]] and all(r.group_size == 3 for _, r in took)
    assert all(r.top_k == 50 and r.temperature == 0.8 and r.top_p == 0.95 and r.do_sample for _, r in took)   # every candidate carries the request

    s = GroupScheduler(4)
    busy = [s.submit(seed=i, **_xy_fields(budget=4 + i)) for i in range(2)]
    assert [r.handle for _, r in s.admit()] == busy and s.free == [2, 3]   # plain submits: SlotScheduler's order
    group = s.submit_group(3, seeds, **_xy_fields())
    late = s.submit(seed=5, **_xy_fields())
    for _ in range(3):                                                     # 2 free slots: the group of 3 waits, nothing overtakes it
        assert s.admit() == [] and s.free == [2, 3] and [r.handle for r in s.pending] == group + [late]
        s.advance(1)
    assert s.due() == [0] and s.retire(0).handle == busy[0]
    took = s.admit()                                                       # slots 0, 2 and 3
    assert [r.handle for _, r in took] == group and [slot for slot, _ in took] == [0, 2, 3]
    assert [r.handle for r in s.pending] == [late] and s.admit() == []
