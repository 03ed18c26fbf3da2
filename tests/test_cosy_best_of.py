"""CPU: best-of-n utterances in the Cosy engine, the pieces that need no device -- the C ABI of rwkv7_ras_slots_lp_f32 (declared in
include/rwkv7_hip.h, typed from it, exported, rwkv7_ras_slot_logprob's Python mirror against the compiler's layout, RWKV7_EINVAL
before any launch), ContinuousCosyDecoder's new interface and its argument checks, and GroupScheduler driven with the requests
the Cosy engine queues."""
import ctypes
import os
import shutil
import subprocess

import pytest

from rwkvtts_amd import _lib
from rwkvtts_amd import continuous_cosy as cc
from rwkvtts_amd.continuous import GroupScheduler, candidate_seed

NAME = "rwkv7_ras_slots_lp_f32"


# ---------------------------------------------------------------------------------------------------------------- 1. ABI
def test_header_declares_the_entry_and_the_struct():
    text = open(_lib.HEADER).read()
    assert NAME in _lib.exported_symbols()
    assert "struct rwkv7_ras_slot_logprob {" in text and "typedef struct rwkv7_ras_slot_logprob rwkv7_ras_slot_logprob;" in text


def test_library_exports_the_entry_with_the_headers_types(hip_lib):
    restype, argtypes = _lib.prototypes()[NAME]
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    # rows, V, logits, ld, row_slot, st, lp, stream
    assert restype is ctypes.c_int and argtypes == [I, I, P, L, P, P, P, P]
    # rwkv7_ras_slots_f32's arguments, then lp, then the stream
    assert argtypes[:-2] == _lib.prototypes()["rwkv7_ras_slots_f32"][1][:-1]
    fn = getattr(hip_lib, NAME)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == argtypes


def test_ras_slot_logprob_mirror_matches_the_compiler(tmp_path):
    fields = ["tok_lp", "cum_lp", "end_lp"]
    assert [n for n, _ in cc.RasSlotLogprob._fields_] == fields
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "rwkv7_hip.h"', "int main(void) {",
             '  printf(". %zu 0\\n", sizeof(rwkv7_ras_slot_logprob));']
    lines += [f'  printf("{f} %zu %zu\\n", offsetof(rwkv7_ras_slot_logprob, {f}), sizeof(((rwkv7_ras_slot_logprob *)0)->{f}));'
              for f in fields]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    cc_ = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/lib/llvm/bin/clang"
    subprocess.run([cc_, "-I", os.path.dirname(os.path.abspath(_lib.HEADER)), str(src), "-o", str(exe)], check=True, capture_output=True)
    c_side = [(f, int(off), int(size)) for f, off, size in
              (line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n") if line)]
    py_side = [(".", ctypes.sizeof(cc.RasSlotLogprob), 0)] + [(n, getattr(cc.RasSlotLogprob, n).offset, getattr(cc.RasSlotLogprob, n).size)
                                                              for n in fields]
    assert py_side == c_side


def test_argument_errors_do_not_launch(hip_lib):
    one = 16   # never dereferenced: the checks fire first
    per_slot = ("step", "limit", "n_ignore", "seed", "top_k", "top_p", "tau_r", "live", "recent", "ptr", "ids", "n_out", "seq")

    def state(**kw):
        st = cc.RasSlotState()
        for f in per_slot + ("emb", "x"):
            setattr(st, f, one)
        st.win_ld, st.seq_ld, st.D, st.slots, st.win_size, st.top_k_max, st.eos = 10, 8, 128, 32, 10, 128, 96
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    f = getattr(hip_lib, NAME)

    def call(st, lp=(one, one, one), rows=1, V=97, logits=one):
        lp = None if lp is None else ctypes.byref(cc.RasSlotLogprob(*lp))
        return f(rows, V, logits, V, None, ctypes.byref(st) if st is not None else None, lp, None)

    EINVAL, ESHAPE = -1, -4
    # the new argument
    assert call(state(), lp=None) == EINVAL
    for k in range(3):
        assert call(state(), lp=tuple(None if i == k else one for i in range(3))) == EINVAL, k
    assert call(state(), lp=None, V=15361) == EINVAL                      # ... and it is looked at before the shapes
    # every case rwkv7_ras_slots_f32 refuses
    assert call(None) == EINVAL and call(state(), rows=0) == EINVAL and call(state(), logits=None) == EINVAL
    for name in per_slot:
        assert call(state(**{name: None})) == EINVAL, name
    assert call(state(slots=0)) == EINVAL and call(state(seq_ld=0)) == EINVAL and call(state(x=None)) == EINVAL
    assert call(state(), V=15361) == ESHAPE
    for bad in (dict(win_size=0), dict(win_size=129, win_ld=200), dict(win_size=11), dict(top_k_max=0), dict(top_k_max=129), dict(D=100)):
        assert call(state(**bad)) == ESHAPE, bad


# ---------------------------------------------------------------------------------------------------------------- 2. engine interface
def _engine_shell(slots, logprobs=False):
    """A ContinuousCosyDecoder with nothing but what the argument checks read: they come before anything touches the device."""
    eng = object.__new__(cc.ContinuousCosyDecoder)
    eng.slots, eng.logprobs, eng._lp_done = slots, logprobs, {}
    eng.sched, eng._extra = cc.GroupScheduler(slots), {}
    return eng


def test_the_engine_has_submit_n_and_take_logprobs():
    import inspect
    eng = cc.ContinuousCosyDecoder
    assert callable(eng.submit_n) and callable(eng.take_logprobs)
    sub, sub_n = inspect.signature(eng.submit).parameters, inspect.signature(eng.submit_n).parameters
    assert list(sub_n)[:2] == ["self", "n"] and set(sub) - {"self"} <= set(sub_n)          # submit()'s arguments, tau_r and seed included
    assert inspect.signature(eng.__init__).parameters["logprobs"].default is False


def test_submit_n_and_take_logprobs_argument_checks():
    for n in (0, -1, 5):
        eng = _engine_shell(4)
        with pytest.raises(ValueError, match="slots"):
            eng.submit_n(n, text=[1, 2, 3])
        assert not eng.sched.pending and not eng._extra, "a refused group leaves nothing in the queue"
    with pytest.raises(ValueError, match="logprobs=True"):
        _engine_shell(4).take_logprobs(0)
    with pytest.raises(KeyError):
        _engine_shell(4, logprobs=True).take_logprobs(0)


# ---------------------------------------------------------------------------------------------------------------- 3. scheduler
def _cosy_fields(budget=12):
    """What ContinuousCosyDecoder queues for one utterance (its _request_fields), with a stand-in for the embeddings."""
    return dict(embeds=None, max_new_tokens=budget, min_new_tokens=3, do_sample=True, top_k=25, top_p=0.8)


def test_group_scheduler_with_cosy_requests_admits_groups_whole_and_fifo():
    assert cc.GroupScheduler is GroupScheduler and cc.candidate_seed is candidate_seed     # the engine's scheduler and keys are the shared ones
    s = GroupScheduler(4)
    seeds = [candidate_seed(7, i) for i in range(3)]
    group = s.submit_group(3, seeds, **_cosy_fields())
    took = s.admit()                                                       # 4 free slots: the group of 3, whole
    assert [r.handle for _, r in took] == group and [slot for slot, _ in took] == [0, 1, 2] and s.free == [3]
    assert [r.seed for _, r in took] == seeds == [7, 8, 9]
    assert [r.leader for _, r in took] == [None, group[0], group[0]] and all(r.group_size == 3 for _, r in took)
    assert all(r.top_k == 25 and r.min_new_tokens == 3 and r.do_sample for _, r in took)   # every candidate carries the request

    s = GroupScheduler(4)
    busy = [s.submit(seed=i, **_cosy_fields(budget=4 + i)) for i in range(2)]
    assert [r.handle for _, r in s.admit()] == busy and s.free == [2, 3]
    group = s.submit_group(3, seeds, **_cosy_fields())
    late = s.submit(seed=5, **_cosy_fields())
    for _ in range(3):                                                     # 2 free slots: the group of 3 waits, nothing overtakes it
        assert s.admit() == [] and s.free == [2, 3] and [r.handle for r in s.pending] == group + [late]
        s.advance(1)
    assert s.due() == [0] and s.retire(0).handle == busy[0]
    took = s.admit()                                                       # slots 0, 2 and 3
    assert [r.handle for _, r in took] == group and [slot for slot, _ in took] == [0, 2, 3]
    assert [r.handle for r in s.pending] == [late] and s.admit() == []
