"""CPU: the device-free parts of serving from stored states -- prefill.plan with one `fresh` flag per sequence against layouts worked
out here, StateStore's bookkeeping and its save / load round trip on CPU tensors, the export and the argument checks of
rwkv7_cache_rows_seed_bf16, and the state arguments of the schedulers and of ContinuousDecoder.submit / submit_n."""
import ctypes

import pytest
import torch

from rwkvtts_amd import _lib
from rwkvtts_amd.continuous import ContinuousDecoder, GroupScheduler, OverlapScheduler, Request, SlotScheduler
from rwkvtts_amd.prefill import ROW_ZERO, SEED_ZERO, check_seed_rows, plan
from rwkvtts_amd.state_store import StateStore

C = 32
FIELDS = ("t_al", "seq_off", "state_row", "prev_src", "last_dst", "keep", "last_row", "pieces", "ends")


# ---------------------------------------------------------------------------------------------------------------- plan
def _expect(lens, rows, fresh, t_al, max_seqs):
    """The one replay of a pack that fits one bucket, from the layout rule alone: piece j ends on a chunk boundary behind 32 - n % 32
    masked rows; its first row carries -2 (fresh) or the row, its state entry the row with or without the zero bit."""
    seq_off, state_row, last_row = [0], [-1] * max_seqs, [0] * max_seqs
    prev_src, last_dst, keep = [-1] * t_al, [-1] * t_al, [False] * t_al
    pieces, ends, t = [], [], 0
    for j, (n, r, f) in enumerate(zip(lens, rows, fresh)):
        lo = t + C - n % C
        t = lo + n
        assert t % C == 0
        seq_off.append(t // C)
        state_row[j] = r + (1 << 30) if f else r
        prev_src[lo] = -2 if f else r
        last_dst[t - 1] = r
        last_row[j] = t - 1
        keep[lo:t] = [True] * n
        pieces.append((j, 0, n, lo))
        ends.append((j, j))
    seq_off[-1] = t_al // C                                   # the rounding's identity chunks belong to the last piece
    seq_off += [t_al // C] * (max_seqs + 1 - len(seq_off))
    return dict(t_al=t_al, seq_off=seq_off, state_row=state_row, prev_src=prev_src, last_dst=last_dst, keep=keep, last_row=last_row,
                pieces=pieces, ends=ends)


def _fields(rp):
    return {f: (getattr(rp, f).tolist() if isinstance(getattr(rp, f), torch.Tensor) else getattr(rp, f)) for f in FIELDS}


LENS, ROWS = (5, 70, 33), (2, 0, 1)


@pytest.mark.parametrize("fresh", [True, False])
def test_plan_with_a_bool_gives_the_replays_of_before(fresh):
    (rp,) = plan(LENS, ROWS, fresh, 4, 8, (64, 128, 256))
    assert rp.seq_off.dtype == rp.state_row.dtype == rp.prev_src.dtype == rp.last_dst.dtype == rp.last_row.dtype == torch.int32
    assert rp.keep.dtype == torch.bool
    got = _fields(rp)
    assert got == _expect(LENS, ROWS, [fresh] * 3, 256, 8)    # aligned lengths 32 + 96 + 64 = 192 rows: the 256 bucket
    # and the numbers themselves, by hand
    assert got["seq_off"] == [0, 1, 4, 8, 8, 8, 8, 8, 8] and got["last_row"] == [31, 127, 191, 0, 0, 0, 0, 0]
    z = ROW_ZERO if fresh else 0
    assert ROW_ZERO == 1 << 30 and got["state_row"] == [2 | z, 0 | z, 1 | z] + [-1] * 5
    assert [(t, v) for t, v in enumerate(got["prev_src"]) if v != -1] == ([(27, -2), (58, -2), (159, -2)] if fresh else [(27, 2), (58, 0), (159, 1)])
    assert [(t, v) for t, v in enumerate(got["last_dst"]) if v != -1] == [(31, 2), (127, 0), (191, 1)]
    assert [t for t, k in enumerate(got["keep"]) if k] == list(range(27, 32)) + list(range(58, 128)) + list(range(159, 192))
    assert got["pieces"] == [(0, 0, 5, 27), (1, 0, 70, 58), (2, 0, 33, 159)] and got["ends"] == [(0, 0), (1, 1), (2, 2)]


def test_plan_with_one_flag_per_sequence_mixes_the_two_entry_by_entry():
    flags = [True, False, True]
    (mix,) = plan(LENS, ROWS, flags, 4, 8, (64, 128, 256))
    (yes,) = plan(LENS, ROWS, True, 4, 8, (64, 128, 256))
    (no,) = plan(LENS, ROWS, False, 4, 8, (64, 128, 256))
    assert _fields(mix) == _expect(LENS, ROWS, flags, 256, 8)
    m, y, n = _fields(mix), _fields(yes), _fields(no)
    for f in ("t_al", "seq_off", "last_dst", "keep", "last_row", "pieces", "ends"):   # the layout does not depend on the flags
        assert m[f] == y[f] == n[f]
    for j, (seq, lo, hi, at) in enumerate(m["pieces"]):
        src = y if flags[seq] else n
        assert m["state_row"][j] == src["state_row"][j]
        assert m["prev_src"][at:at + hi - lo] == src["prev_src"][at:at + hi - lo]
    assert m["state_row"][3:] == [-1] * 5
    assert [v for v in m["prev_src"] if v != -1] == [-2, 0, -2]
    assert m["state_row"][:3] == [2 | ROW_ZERO, 0, 1 | ROW_ZERO]
    # tuples, and anything truthy per entry, are flags too; the wrong count is an error
    assert _fields(plan(LENS, ROWS, (1, 0, 1), 4, 8, (64, 128, 256))[0]) == m
    with pytest.raises(ValueError):
        plan(LENS, ROWS, [True, False], 4, 8, (64, 128, 256))


def test_a_long_continued_prompt_never_carries_the_zero_mark():
    rps = plan([300], [3], [False], 4, 8, (64, 128))          # 96-token pieces fill the 128 bucket; the last 108 tokens fit it too
    assert [rp.pieces for rp in rps] == [[(0, 0, 96, 32)], [(0, 96, 192, 32)], [(0, 192, 300, 20)]]
    for rp in rps:
        assert rp.state_row.tolist() == [3] + [-1] * 7        # no bit 30 anywhere
        assert [v for v in rp.prev_src.tolist() if v != -1] == [3]
        assert -2 not in rp.prev_src.tolist()
    assert [rp.ends for rp in rps] == [[], [], [(0, 0)]]
    # the fresh twin differs in its first piece only
    first = plan([300], [3], [True], 4, 8, (64, 128))
    assert first[0].state_row[0] == 3 | ROW_ZERO and first[0].prev_src[32] == -2
    for a, b in zip(first[1:], rps[1:]):
        assert _fields(a) == _fields(b)


# ---------------------------------------------------------------------------------------------------------------- store
def _cpu_model(L=2, D=128, seed=0):
    from rwkvtts_amd.spark_llm import RWKV7ForSpeech, RWKV7SpeechConfig
    cfg = RWKV7SpeechConfig(vocab_size=300, text_vocab_size=300, audio_global_vocab_size=64, hidden_size=D, num_hidden_layers=L,
                            decay_low_rank_dim=32, a_low_rank_dim=32, v_low_rank_dim=32, gate_low_rank_dim=64)
    return RWKV7ForSpeech(cfg).init_weights(seed).to(torch.bfloat16).eval()


@pytest.fixture(scope="module")
def cpu_model():
    return _cpu_model()


def _fill(store, row, seed):
    """Random BITS into one row of the store's (CPU) cache, NaN patterns included."""
    g = torch.Generator().manual_seed(seed)
    for s in store.cache.states:
        for t in (s.att_x_prev, s.ffn_x_prev):
            t[row] = torch.randint(-32768, 32768, t[row].shape, generator=g, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
        s.att_kv[row] = torch.randint(-2 ** 31, 2 ** 31, s.att_kv[row].shape, generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)


def _row_bits(store, row):
    return [(t[row].view(torch.int16) if t.dtype == torch.bfloat16 else t[row].view(torch.int32)).clone()
            for s in store.cache.states for t in (s.att_x_prev, s.att_kv, s.ffn_x_prev)]


def test_store_bookkeeping(cpu_model):
    st = StateStore(cpu_model, 3)
    assert st.capacity == 3 and st.names() == [] and "a" not in st and len(st.cache) == 2
    assert st.cache[0].att_kv.shape == (3, 2, 64, 64) and st.cache[0].att_x_prev.shape == (3, 128) and st.cache[0].att_x_prev.dtype == torch.bfloat16
    assert [st.reserve(n, t) for n, t in (("a", 10), ("b", 20), ("c", 30))] == [0, 1, 2]   # the lowest free row
    assert st.names() == ["a", "b", "c"] and "b" in st and st.row("c") == 2 and st.tokens == [10, 20, 30]
    with pytest.raises(RuntimeError, match="full"):
        st.reserve("d")
    assert st.reserve("b", 21) == 1 and st.tokens[1] == 21    # a stored name keeps its row
    st.evict("a")
    assert st.names() == ["b", "c"] and "a" not in st and st.tokens[0] == 0
    with pytest.raises(KeyError):
        st.evict("a")
    with pytest.raises(KeyError):
        st.row("a")
    assert st.reserve("d") == 0 and st.names() == ["b", "c", "d"]
    with pytest.raises(ValueError):
        StateStore(cpu_model, 0)
    with pytest.raises(ValueError):
        st.reserve("")


def test_a_pinned_name_cannot_be_evicted_or_replaced(cpu_model):
    st = StateStore(cpu_model, 2)
    st.reserve("v", 7)
    assert st.pin("v") == 0 and st.pin("v") == 0 and st.pinned("v") == 2
    with pytest.raises(RuntimeError, match="pinned"):
        st.evict("v")
    with pytest.raises(RuntimeError, match="pinned"):
        st.reserve("v")
    st.unpin("v")
    with pytest.raises(RuntimeError, match="pinned"):
        st.evict("v")
    st.unpin("v")
    with pytest.raises(RuntimeError):
        st.unpin("v")
    with pytest.raises(KeyError):
        st.pin("w")
    st.evict("v")
    assert st.names() == [] and st.pinned("v") == 0


def test_save_load_round_trip_is_bit_for_bit(cpu_model, tmp_path):
    st = StateStore(cpu_model, 4)
    for name, tok, seed in (("x", 3, 1), ("gone", 4, 2), ("y", 5, 3), ("z", 6, 4)):
        _fill(st, st.reserve(name, tok), seed)
    st.evict("gone")                                          # the used rows are 0, 2, 3
    path = tmp_path / "voices.pt"
    st.save(path)
    blob = torch.load(path, weights_only=True)                # tensors and plain data only
    assert blob["names"] == ["x", "y", "z"] and blob["tokens"] == [3, 5, 6]
    assert blob["fingerprint"] == {"format": 1, "layers": 2, "D": 128, "H": 2, "dtype": "torch.bfloat16"}
    assert blob["att_kv"].shape == (2, 3, 2, 64, 64) and blob["att_x_prev"].shape == blob["ffn_x_prev"].shape == (2, 3, 128)
    back = StateStore.load(path, cpu_model)
    assert back.capacity == 3 and back.names() == ["x", "y", "z"] and back.tokens == [3, 5, 6]
    for name in ("x", "y", "z"):
        for a, b in zip(_row_bits(st, st.row(name)), _row_bits(back, back.row(name))):
            assert torch.equal(a, b)                          # integer views: NaN payloads compare
    roomy = StateStore.load(path, cpu_model, capacity=5)
    assert roomy.capacity == 5 and roomy.reserve("new") == 3
    with pytest.raises(ValueError):
        StateStore.load(path, cpu_model, capacity=2)


def test_load_refuses_another_geometry(cpu_model, tmp_path):
    st = StateStore(cpu_model, 1)
    st.reserve("v")
    path = tmp_path / "v.pt"
    st.save(path)
    for other in (_cpu_model(L=3), _cpu_model(D=192), _cpu_model().to(torch.float32)):
        with pytest.raises(ValueError, match="needs"):
            StateStore.load(path, other)
    assert StateStore.load(path, _cpu_model(seed=5)).names() == ["v"]   # other weights, same geometry: the file cannot tell


# ---------------------------------------------------------------------------------------------------------------- entry
def test_row_seed_is_exported_and_rejects_bad_arguments_without_launching(hip_lib):
    assert "rwkv7_cache_rows_seed_bf16" in _lib.exported_symbols()
    assert SEED_ZERO == -1
    f = hip_lib.rwkv7_cache_rows_seed_bf16
    one = ctypes.c_void_p(16)   # never dereferenced: the checks fire first

    def call(layers=2, n=3, src=one, dst=one, sr=one, dr=one, D=128, H=2):
        return f(layers, n, src, dst, sr, dr, D, H, None)

    assert call(D=100, H=1) == -4                             # D % 8 != 0
    assert call(D=8200, H=128) == -4                          # wider than the row kernels
    assert call(D=128, H=3) == -3                             # D != 64 H
    assert call(D=72, H=1) == -3
    assert call(n=-1) == -1
    assert call(src=None) == -1 and call(dst=None) == -1
    assert call(sr=None) == -1 and call(dr=None) == -1        # index arrays are needed once n > 0
    assert call(layers=0) == -1 and call(layers=70000) == -1 and call(n=70000) == -1 and call(H=0, D=0) == -1
    assert call(n=0, sr=None, dr=None) == 0                   # nothing to do: no launch either


def test_seed_row_lists_are_checked_on_the_host():
    assert check_seed_rows([0, -1, 2], [3, 1, 0], 8, 4) == ([0, -1, 2], [3, 1, 0])   # -1: a zero entry, active
    assert check_seed_rows([9, -5], [-1, -1], 8, 4) == ([9, -5], [-1, -1])           # a skipped entry's source is not read
    assert check_seed_rows([-2, 1], [1, 1], 8, 4) == ([-2, 1], [1, 1])               # a source below -1 skips its entry too
    for src, dst in (([0, 1], [1]), ([0, 8], [0, 1]), ([0, -1], [4, 0]), ([0, -1], [2, 2]), ([3, 1], [1, 1])):
        with pytest.raises(ValueError):
            check_seed_rows(src, dst, 8, 4)


# ---------------------------------------------------------------------------------------------------------------- scheduler, submit
def test_the_schedulers_carry_state_row():
    assert Request(handle=0, embeds=None, max_new_tokens=1).state_row is None
    for cls in (SlotScheduler, OverlapScheduler, GroupScheduler):
        s = cls(4)
        s.submit(embeds=None, max_new_tokens=3, state="v", state_row=2)
        s.submit(embeds=None, max_new_tokens=3)
        took = s.reserve(4) if cls is OverlapScheduler else s.admit()
        assert [(slot, r.state, r.state_row) for slot, r in took] == [(0, "v", 2), (1, None, None)]
    g = GroupScheduler(4)
    hs = g.submit_group(3, [7, 8, 9], embeds=None, max_new_tokens=2, state="v", state_row=1)
    assert [(r.handle, r.leader, r.state_row, r.seed) for _, r in g.admit()] == [(hs[0], None, 1, 7), (hs[1], hs[0], 1, 8), (hs[2], hs[0], 1, 9)]


class _HostSubmit(ContinuousDecoder):
    """submit / submit_n with the prompt handling stubbed out: what remains is the state argument and the queue."""

    def __init__(self, store, admission="eager", slots=4):
        self.store, self.admission, self.slots = store, admission, slots
        self.sched = OverlapScheduler(slots) if admission == "overlap" else GroupScheduler(slots)

    def _request_fields(self, input_ids, inputs_embeds, max_new_tokens, *rest):
        return dict(embeds=input_ids, max_new_tokens=int(max_new_tokens))


def test_submit_state_argument_errors(cpu_model):
    eng = _HostSubmit(None)
    with pytest.raises(ValueError, match="state_store"):
        eng.submit(input_ids=[1], state="v")
    with pytest.raises(ValueError, match="state_store"):
        eng.submit_n(2, input_ids=[1], state="v")
    assert not eng.sched.pending
    assert eng.submit(input_ids=[1]) == 0                     # no state: as before
    st = StateStore(cpu_model, 2)
    st.reserve("v", 5)
    eng = _HostSubmit(st)
    with pytest.raises(KeyError):
        eng.submit(input_ids=[1], state="w")
    with pytest.raises(KeyError):
        eng.submit_n(2, input_ids=[1], state="w")
    assert not eng.sched.pending and st.pinned("v") == 0
    h = eng.submit(input_ids=[1], state="v")
    hs = eng.submit_n(3, input_ids=[1], state="v", seed=5)
    assert st.pinned("v") == 2                                # one pin per submit call: a group's first candidate unpins
    with pytest.raises(RuntimeError, match="pinned"):
        st.evict("v")
    took = eng.sched.admit()
    assert [(r.handle, r.state, r.state_row) for _, r in took] == [(h, "v", 0)] + [(x, "v", 0) for x in hs]
    eng._unpin(took)
    assert st.pinned("v") == 0
    st.evict("v")
    # n > 1 with admission="overlap" stays the error it is, and pins nothing
    st.reserve("v")
    ov = _HostSubmit(st, admission="overlap")
    with pytest.raises(ValueError, match="overlap"):
        ov.submit_n(2, input_ids=[1], state="v")
    assert st.pinned("v") == 0 and ov.submit_n(1, input_ids=[1], state="v") == [0] and st.pinned("v") == 1


def test_a_store_of_another_config_is_refused_at_construction(cpu_model):
    other = StateStore(_cpu_model(L=3), 1)
    with pytest.raises(ValueError, match="state_store"):
        ContinuousDecoder(cpu_model, slots=4, state_store=other)   # before anything touches the device
