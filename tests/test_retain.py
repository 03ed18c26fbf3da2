"""CPU: the device-free parts of retaining a finished request's state -- StateStore's pending names, the host check of the retain
rows, the export and the argument checks of rwkv7_cache_rows_retain_bf16, the retain arguments of ContinuousDecoder and of its
submit / submit_n (every error before anything touches a device), and the tokens a retained state has seen."""
import ctypes

import pytest
import torch

from rwkvtts_amd import _lib
from rwkvtts_amd.continuous import ContinuousDecoder, GroupScheduler, OverlapScheduler, Request, retained_tokens
from rwkvtts_amd.prefill import check_retain_rows
from rwkvtts_amd.state_store import StateStore


def _cpu_model(L=2, D=128, seed=0):
    from rwkvtts_amd.spark_llm import RWKV7ForSpeech, RWKV7SpeechConfig
    cfg = RWKV7SpeechConfig(vocab_size=300, text_vocab_size=300, audio_global_vocab_size=64, hidden_size=D, num_hidden_layers=L,
                            decay_low_rank_dim=32, a_low_rank_dim=32, v_low_rank_dim=32, gate_low_rank_dim=64)
    return RWKV7ForSpeech(cfg).init_weights(seed).to(torch.bfloat16).eval()


@pytest.fixture(scope="module")
def cpu_model():
    return _cpu_model()


# ---------------------------------------------------------------------------------------------------------------- store
def test_a_pending_name_is_invisible_until_published(cpu_model, tmp_path):
    st = StateStore(cpu_model, 4)
    assert st.reserve("a", 10) == 0 and st.pending() == []
    assert st.reserve_pending("p") == 1 and st.reserve_pending("q") == 2     # the lowest free rows
    assert st.pending() == ["p", "q"]
    assert "p" not in st and len(st) == 1 and st.names() == ["a"]
    with pytest.raises(KeyError):
        st.row("p")
    with pytest.raises(KeyError):
        st.pin("p")
    assert st.pinned("p") == 0
    with pytest.raises(KeyError):
        st.evict("p")
    st.save(tmp_path / "s.pt")
    blob = torch.load(tmp_path / "s.pt", weights_only=True)
    assert blob["names"] == ["a"] and blob["tokens"] == [10] and blob["att_kv"].shape[1] == 1
    # the rows are held: the next name takes row 3, not 1 or 2
    assert st.reserve("b") == 3
    # publish: an ordinary stored state
    assert st.publish("p", 77) == 1
    assert "p" in st and st.names() == ["a", "b", "p"] and st.row("p") == 1 and st.tokens[1] == 77 and len(st) == 3
    assert st.pending() == ["q"] and st.pin("p") == 1
    st.unpin("p")
    st.save(tmp_path / "s.pt")
    assert torch.load(tmp_path / "s.pt", weights_only=True)["names"] == ["a", "b", "p"]
    st.evict("p")
    assert st.reserve("c") == 1
    # abandon: the row is free again, and the lowest free row is the next one taken
    st.evict("a")
    st.abandon("q")
    assert st.pending() == [] and "q" not in st
    assert st.reserve_pending("r") == 0 and st.reserve_pending("s") == 2
    for gone in ("q", "nope", "c"):
        with pytest.raises(KeyError):
            st.publish(gone, 1)
        with pytest.raises(KeyError):
            st.abandon(gone)


def test_reserve_pending_refuses_stored_pending_and_full(cpu_model):
    st = StateStore(cpu_model, 2)
    st.reserve("v", 5)
    with pytest.raises(ValueError, match="stored"):
        st.reserve_pending("v")
    assert st.reserve_pending("p") == 1
    with pytest.raises(ValueError, match="pending"):
        st.reserve_pending("p")
    with pytest.raises(ValueError, match="pending"):
        st.reserve("p")                                       # nor may reserve / put / capture take the name meanwhile
    with pytest.raises(RuntimeError, match="full"):
        st.reserve_pending("q")
    with pytest.raises(RuntimeError, match="full"):
        st.reserve("w")                                       # a pending row is not free
    for bad in ("", None, 3):
        with pytest.raises(ValueError):
            st.reserve_pending(bad)
    assert st.pending() == ["p"] and st.names() == ["v"]
    st.abandon("p")
    assert st.reserve_pending("q") == 1


# ---------------------------------------------------------------------------------------------------------------- rows, entry
def test_retain_rows_are_checked_on_the_host():
    assert check_retain_rows([-1, 2, -1, 0], 3) == [-1, 2, -1, 0]
    assert check_retain_rows([-1, -1, -5], 1) == [-1, -1, -5]  # negative entries name no row and may repeat
    assert check_retain_rows([], 1) == []
    for rows, cap in (([0, 0], 4), ([-1, 2, 2], 4), ([3], 3), ([0, 1, 7], 4)):
        with pytest.raises(ValueError):
            check_retain_rows(rows, cap)


def test_row_retain_is_exported_and_rejects_bad_arguments_without_launching(hip_lib):
    assert "rwkv7_cache_rows_retain_bf16" in _lib.exported_symbols()
    f = hip_lib.rwkv7_cache_rows_retain_bf16
    one = ctypes.c_void_p(16)   # never dereferenced: the checks fire first

    def call(layers=2, slots=3, src=one, dst=one, live=one, armed=one, row=one, ticket=one, D=128, H=2):
        return f(layers, slots, src, dst, live, armed, row, ticket, D, H, None)

    assert call(D=100, H=1) == -4                             # D % 8 != 0
    assert call(D=8200, H=128) == -4                          # wider than the row kernels
    assert call(D=128, H=3) == -3 and call(D=72, H=1) == -3   # D != 64 H
    assert call(slots=-1) == -1
    assert call(src=None) == -1 and call(dst=None) == -1
    for name in ("live", "armed", "row", "ticket"):
        assert call(**{name: None}) == -1, name
        assert call(slots=0, **{name: None}) == -1, name      # whatever slots is
    assert call(layers=0) == -1 and call(layers=70000) == -1 and call(slots=70000) == -1 and call(H=0, D=0) == -1
    assert call(slots=0) == 0                                 # nothing to do: no launch either


# ---------------------------------------------------------------------------------------------------------------- engine arguments
def test_constructor_refuses_retain_without_a_store_or_with_overlap(cpu_model):
    with pytest.raises(ValueError, match="state_store"):
        ContinuousDecoder(cpu_model, slots=4, retain=True)    # before anything touches the device
    st = StateStore(cpu_model, 2)
    with pytest.raises(ValueError, match="overlap"):
        ContinuousDecoder(cpu_model, slots=4, state_store=st, retain=True, admission="overlap")
    assert ContinuousDecoder.retain is False


class _HostSubmit(ContinuousDecoder):
    """submit / submit_n with the prompt handling stubbed out: what remains is the state and retain arguments and the queue."""

    def __init__(self, store, retain=False, admission="eager", slots=4):
        self.store, self.retain, self.admission, self.slots = store, retain, admission, slots
        self.sched = OverlapScheduler(slots) if admission == "overlap" else GroupScheduler(slots)

    def _request_fields(self, input_ids, inputs_embeds, max_new_tokens, *rest):
        return dict(embeds=torch.zeros(len(input_ids), 1), max_new_tokens=int(max_new_tokens))


def test_submit_retain_argument_errors(cpu_model):
    st = StateStore(cpu_model, 3)
    st.reserve("v", 5)
    for eng in (_HostSubmit(None), _HostSubmit(st)):          # no store, and a store without the switch
        with pytest.raises(ValueError, match="retain=True"):
            eng.submit(input_ids=[1], retain="t")
        with pytest.raises(ValueError, match="retain=True"):
            eng.submit_n(1, input_ids=[1], retain="t")
        assert not eng.sched.pending
    assert st.pending() == []
    eng = _HostSubmit(st, retain=True)
    with pytest.raises(ValueError, match="one name holds one state"):
        eng.submit_n(2, input_ids=[1], retain="t")
    with pytest.raises(ValueError, match="stored"):
        eng.submit(input_ids=[1], retain="v")                 # also: state= and retain= cannot name the same state
    with pytest.raises(ValueError, match="stored"):
        eng.submit(input_ids=[1], state="v", retain="v")
    assert st.pending() == [] and st.pinned("v") == 0 and not eng.sched.pending
    # an unknown source state gives the pending row back
    with pytest.raises(KeyError):
        eng.submit(input_ids=[1], state="w", retain="t")
    assert st.pending() == [] and not eng.sched.pending
    h0 = eng.submit(input_ids=[1, 2, 3], retain="t")
    (h1,) = eng.submit_n(1, input_ids=[4], state="v", retain="u")
    assert st.pending() == ["t", "u"] and st.pinned("v") == 1 and "t" not in st
    with pytest.raises(ValueError, match="pending"):
        eng.submit(input_ids=[1], retain="t")
    with pytest.raises(RuntimeError, match="full"):
        eng.submit(input_ids=[1], retain="x")
    got = {r.handle: r for _, r in eng.sched.admit()}
    assert (got[h0].retain, got[h0].retain_row, got[h0].state_row, got[h0].base_tokens) == ("t", 1, None, 0)
    assert (got[h1].retain, got[h1].retain_row, got[h1].state, got[h1].state_row, got[h1].base_tokens) == ("u", 2, "v", 0, 5)
    # the caller's way out when the engine is dropped with requests in flight
    for name in st.pending():
        st.abandon(name)
    assert st.pending() == [] and st.reserve_pending("again") == 1


def test_request_defaults_carry_no_retain():
    r = Request(handle=0, embeds=None, max_new_tokens=1)
    assert r.retain is None and r.retain_row is None and r.base_tokens == 0


def test_retained_tokens():
    assert retained_tokens(0, 7, 1) == 7                      # ended with its first id: the state after the prompt
    assert retained_tokens(0, 7, 5) == 11                     # the last id was never fed back
    assert retained_tokens(50, 3, 10) == 62                   # continued from a stored state of 50 tokens
    for bad in ((0, 0, 1), (0, 5, 0), (-1, 5, 1)):
        with pytest.raises(ValueError):
            retained_tokens(*bad)
