"""CPU: best-of-n requests in the continuous decoder, the pieces that need no device -- the C ABI of rwkv7_sample_slots_lp_f32
(declared in include/rwkv7_hip.h, typed from it, exported, RWKV7_EINVAL / RWKV7_ESHAPE before any launch, rwkv7_slot_logprob's Python
mirror against the compiler's layout), GroupScheduler's all-or-nothing FIFO admission, candidate_seed, rank_candidates and the
argument checks of ContinuousDecoder.submit_n."""
import ctypes
import os
import random
import shutil
import subprocess

import pytest

from rwkvtts_amd import _lib
from rwkvtts_amd.continuous import (ContinuousDecoder, GroupScheduler, SlotLogprob, SlotScheduler, SlotState, candidate_seed,
                                    rank_candidates)

NAME = "rwkv7_sample_slots_lp_f32"


# ---------------------------------------------------------------------------------------------------------------- 1. ABI
def test_header_declares_the_entry_and_the_library_exports_it(hip_lib):
    assert NAME in _lib.exported_symbols()
    restype, argtypes = _lib.prototypes()[NAME]
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    # rows, logits, ld, row_slot, allow_lo, allow_hi, suppress, nsuppress, max_domain, st, lp, stream
    assert restype is ctypes.c_int and argtypes == [I, P, L, P, P, P, P, I, I, P, P, P]
    # rwkv7_sample_slots_f32's arguments, then lp, then the stream
    assert argtypes[:-2] == _lib.prototypes()["rwkv7_sample_slots_f32"][1][:-1]
    fn = getattr(hip_lib, NAME)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == argtypes


def test_slot_logprob_mirror_matches_the_compiler(tmp_path):
    fields = ["tok_lp", "cum_lp"]
    assert [n for n, _ in SlotLogprob._fields_] == fields
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "rwkv7_hip.h"', "int main(void) {",
             '  printf(". %zu 0\\n", sizeof(rwkv7_slot_logprob));']
    lines += [f'  printf("{f} %zu %zu\\n", offsetof(rwkv7_slot_logprob, {f}), sizeof(((rwkv7_slot_logprob *)0)->{f}));' for f in fields]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/lib/llvm/bin/clang"
    subprocess.run([cc, "-I", os.path.dirname(os.path.abspath(_lib.HEADER)), str(src), "-o", str(exe)], check=True, capture_output=True)
    c_side = [(f, int(off), int(size)) for f, off, size in
              (line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n") if line)]
    py_side = [(".", ctypes.sizeof(SlotLogprob), 0)] + [(n, getattr(SlotLogprob, n).offset, getattr(SlotLogprob, n).size) for n in fields]
    assert py_side == c_side


def _state(**kw):
    st = SlotState()
    for name in ("step", "limit", "min_until", "seed", "inv_temp", "top_k", "top_p", "do_sample", "live", "ids", "seq", "emb", "x"):
        setattr(st, name, 16)   # never dereferenced: the checks fire first
    st.seq_ld, st.D, st.slots, st.top_k_max, st.eos = 8, 64, 4, 64, -1
    for k, v in kw.items():
        setattr(st, k, v)
    return st


def test_argument_errors_do_not_launch(hip_lib):
    one = ctypes.c_void_p(16)
    f = getattr(hip_lib, NAME)

    def call(rows=4, st=None, max_domain=1024, nsuppress=0, suppress=None, allow=(None, None), logits=one, lp=(16, 16)):
        st = _state() if st is None else st
        lp = None if lp is None else ctypes.byref(SlotLogprob(*lp))
        return f(rows, logits, ctypes.c_long(1024), None, allow[0], allow[1], suppress, nsuppress, max_domain,
                 ctypes.byref(st) if st is not False else None, lp, None)

    # the new argument
    assert call(lp=None) == -1
    assert call(lp=(None, 16)) == -1                          # null tok_lp
    assert call(lp=(16, None)) == -1                          # null cum_lp
    assert call(lp=None, max_domain=15361) == -1              # ... and it is looked at before the shapes
    # every case rwkv7_sample_slots_f32 refuses (tests/test_continuous.py)
    assert call(rows=0) == -1
    assert call(rows=-3) == -1
    assert call(st=False) == -1                               # null st
    assert call(logits=None) == -1
    assert call(max_domain=0) == -1
    assert call(nsuppress=2) == -1                            # suppress count without the list
    assert call(allow=(one, None)) == -1                      # half an allowed range
    assert call(st=_state(step=None)) == -1
    assert call(st=_state(live=None)) == -1
    assert call(st=_state(seq_ld=0)) == -1
    assert call(st=_state(slots=0)) == -1
    assert call(st=_state(x=None)) == -1                      # emb without x
    assert call(st=_state(top_k_max=65)) == -4                # top_k out of range
    assert call(st=_state(top_k_max=-1)) == -4
    assert call(max_domain=15361) == -4
    assert call(nsuppress=257, suppress=one) == -4
    assert call(st=_state(D=100)) == -4                       # D % 8 != 0


# ---------------------------------------------------------------------------------------------------------------- 2. scheduler
def _handles(took):
    return [r.handle for _, r in took]


def test_a_group_waits_for_all_its_slots_and_nothing_overtakes_it():
    s = GroupScheduler(3)
    busy = s.submit(embeds=None, max_new_tokens=4)
    assert _handles(s.admit()) == [busy]                      # slot 0 is busy for 3 replays
    group = s.submit_group(3, [7, 8, 9], embeds=None, max_new_tokens=5)
    late = s.submit(embeds=None, max_new_tokens=2)            # behind the group
    assert group == [busy + 1, busy + 2, busy + 3]
    for _ in range(3):
        assert s.admit() == [], "two slots are free: the group of 3 must wait, and the single request behind it must not overtake"
        assert sorted(s.free) == [1, 2] and [r.handle for r in s.pending] == group + [late]
        s.advance(1)
    assert s.due() == [0] and s.retire(0).handle == busy
    took = s.admit()                                          # three free slots: the whole group, in candidate order
    assert _handles(took) == group and [slot for slot, _ in took] == [0, 1, 2]
    assert [r.seed for _, r in took] == [7, 8, 9]
    assert [r.leader for _, r in took] == [None, group[0], group[0]] and all(r.group_size == 3 for _, r in took)
    assert [r.handle for r in s.pending] == [late] and s.admit() == []
    s.advance(4)
    for slot in s.due():
        s.retire(slot)
    assert _handles(s.admit()) == [late]


def test_groups_admit_in_fifo_order_next_to_single_requests():
    s = GroupScheduler(4)
    a = s.submit(embeds=None, max_new_tokens=3)
    g2 = s.submit_group(2, [1, 2], embeds=None, max_new_tokens=3)
    g3 = s.submit_group(3, [1, 2, 3], embeds=None, max_new_tokens=3)
    b = s.submit(embeds=None, max_new_tokens=3)
    took = s.admit()                                          # a + the pair fit (3 of 4 slots); the triple does not, b waits behind it
    assert _handles(took) == [a] + g2 and s.free == [3]
    assert [r.handle for r in s.pending] == g3 + [b]
    s.advance(2)
    for slot in s.due():
        s.retire(slot)
    took = s.admit()
    assert _handles(took) == g3 + [b] and sorted(slot for slot, _ in took) == [0, 1, 2, 3]


def _trace(sched, submit, seed):
    """The submission pattern of tests/test_continuous.py::test_submit_during_a_run_and_every_handle_returns_once: every admission,
    retirement and replay count, as a list."""
    rng = random.Random(seed)
    log, replays, n_sub = [], 0, 0
    for _ in range(6):
        submit(sched, rng.randint(1, 20))
        n_sub += 1
    while not sched.idle:
        log += [("retire", slot, sched.retire(slot).handle, replays) for slot in sched.due()]
        log += [("admit", slot, req.handle, req.seed, req.leader, req.group_size, replays) for slot, req in sched.admit()]
        log += [("retire", slot, sched.retire(slot).handle, replays) for slot in sched.due()]
        if sched.busy:
            n = min(4, sched.replays_until_due())
            sched.advance(n)
            replays += n
        if n_sub < 20:
            submit(sched, rng.randint(1, 20))
            n_sub += 1
        log.append(("free", tuple(sched.free), len(sched.pending)))
    return log


@pytest.mark.parametrize("slots,seed", [(4, 3), (1, 5), (7, 11)])
def test_a_group_of_one_is_a_plain_request(slots, seed):
    plain = _trace(SlotScheduler(slots), lambda s, b: s.submit(embeds=None, max_new_tokens=b, seed=b), seed)
    group = _trace(GroupScheduler(slots), lambda s, b: s.submit_group(1, [b], embeds=None, max_new_tokens=b), seed)
    mixed = _trace(GroupScheduler(slots), lambda s, b: s.submit(embeds=None, max_new_tokens=b, seed=b), seed)
    assert plain == group == mixed and len(plain) > 20


def test_a_group_larger_than_the_engine_is_refused():
    s = GroupScheduler(3)
    with pytest.raises(ValueError):
        s.submit_group(4, [0, 1, 2, 3], embeds=None, max_new_tokens=5)
    with pytest.raises(ValueError):
        s.submit_group(0, [], embeds=None, max_new_tokens=5)
    with pytest.raises(ValueError):
        s.submit_group(2, [0], embeds=None, max_new_tokens=5)     # one seed per candidate
    with pytest.raises(ValueError):
        s.submit_group(2, [0, 1], embeds=None, max_new_tokens=0)
    assert not s.pending, "a refused group leaves nothing in the queue"
    assert len(s.submit_group(3, [0, 1, 2], embeds=None, max_new_tokens=5)) == 3 and len(s.pending) == 3


def _engine_shell(slots, admission):
    """A ContinuousDecoder with nothing but what submit_n's argument checks read: they come before anything touches the device."""
    eng = object.__new__(ContinuousDecoder)
    eng.slots, eng.admission = slots, admission
    return eng


def test_submit_n_argument_checks():
    with pytest.raises(ValueError, match="overlap"):
        _engine_shell(4, "overlap").submit_n(2, input_ids=[1, 2, 3])
    for admission in ("eager", "graph", "overlap"):
        for n in (5, 0, -1):
            with pytest.raises(ValueError, match="slots"):
                _engine_shell(4, admission).submit_n(n, input_ids=[1, 2, 3])


# ---------------------------------------------------------------------------------------------------------------- 3. host helpers
def test_candidate_seed_wraps_at_2_to_the_64():
    top = (1 << 64) - 1
    assert candidate_seed(5, 0) == 5 and candidate_seed(5, 3) == 8
    assert candidate_seed(top, 0) == top and candidate_seed(top, 1) == 0 and candidate_seed(top - 1, 4) == 2
    assert candidate_seed((1 << 63) - 1, 1) == 1 << 63        # through the sign bit of the device's int64 copy
    assert all(0 <= candidate_seed(top - 2, i) <= top for i in range(8))
    assert len({candidate_seed(top - 2, i) for i in range(8)}) == 8


def test_rank_candidates():
    import numpy as np
    import torch
    cum, lens = [-12.0, -6.0, -9.0, -30.0], [4, 3, 9, 10]     # means -3, -2, -1, -3
    assert rank_candidates(cum, lens) == [2, 1, 0, 3]         # by mean; the tie at -3 goes to the lower index
    assert rank_candidates(cum, lens, length_normalize=False) == [1, 2, 0, 3]
    assert rank_candidates(torch.tensor(cum, dtype=torch.float64), torch.tensor(lens)) == [2, 1, 0, 3]
    assert rank_candidates(np.array(cum), np.array(lens), length_normalize=False) == [1, 2, 0, 3]
    assert rank_candidates([-1.0, -1.0, -1.0], [1, 1, 1]) == [0, 1, 2]
    assert rank_candidates([-2.0, -1.0, -2.0, -1.0], [2, 1, 2, 1], length_normalize=False) == [1, 3, 0, 2]
    assert rank_candidates([float("-inf"), -5.0], [1, 5]) == [1, 0]
    assert rank_candidates([], []) == []
    with pytest.raises(ValueError):
        rank_candidates([-1.0], [1, 2])
    with pytest.raises(ValueError):
        rank_candidates([-1.0], [0])
