"""CPU: the host side of state tuning (rwkvtts_amd/state_tune.py) -- the CSR a step hands to rwkv7_state_rows_adamw_f32, the errors of
step / add / load_state_dict, the state_dict round trip, the torch route of the step against a hand-written loop with one
torch.optim.AdamW per voice, and the two C entries' declaration, export and argument checks.

The model is a toy with the attributes StateStore and StateTuner read (config, device, dtype, parameters, train / eval) whose loss is
a smooth function of the cache rows: the backbone itself runs on the HIP device only (tests/test_state_tune_gpu.py)."""
import ctypes
import types

import pytest
import torch

from rwkvtts_amd import _lib
from rwkvtts_amd.backbone import Cache, LayerState
from rwkvtts_amd.state_store import StateStore
from rwkvtts_amd.state_tune import FIELDS, StateTuner, build_csr

L, D, H = 2, 128, 2
NAMES = ("v0", "v1", "v2")
VOICES = ["v2", "v0", "v2", None, "v0"]          # voice 1 absent, one untuned sequence
ALL = ("att_kv", "att_x_prev", "ffn_x_prev")


class Toy(torch.nn.Module):
    """loss = mean over sequences of a smooth function of the sequence's input and of its cache row (every field of every layer)."""

    def __init__(self, dtype=torch.bfloat16, layers=L, d=D):
        super().__init__()
        self.config = types.SimpleNamespace(num_hidden_layers=layers, hidden_size=d, num_heads=d // 64)
        g = torch.Generator().manual_seed(1)
        self.w_kv = torch.nn.Parameter(torch.randn(layers, d // 64, 64, 64, generator=g) * 0.1)
        self.w_x = torch.nn.Parameter(torch.randn(layers, 2, d, generator=g) * 0.1)
        self.frozen = torch.nn.Parameter(torch.ones(1), requires_grad=False)
        self._dtype = dtype
        self.calls = []

    device = property(lambda self: self.w_kv.device)
    dtype = property(lambda self: self._dtype)

    def forward(self, inputs_embeds=None, labels=None, past_key_values=None, cu_seqlens=None, explode=False, nan=False):
        x = inputs_embeds
        self.calls.append((self.training, [p.requires_grad for p in self.parameters()]))
        if explode:
            raise RuntimeError("boom")
        if cu_seqlens is not None:
            cu = cu_seqlens.tolist()
            x = torch.stack([x[0, a:b].mean() for a, b in zip(cu[:-1], cu[1:])]).unsqueeze(1)
        s = x.float().mean(1)
        for l, st in enumerate(past_key_values.states):
            s = s + (st.att_kv * self.w_kv[l]).sum((1, 2, 3)) * x.float().mean(1) + (st.att_x_prev.float() * self.w_x[l, 0]).sum(1) \
                + (st.ffn_x_prev.float() * self.w_x[l, 1]).sum(1).tanh()
        loss = ((s - labels.float()) ** 2).mean()
        return types.SimpleNamespace(loss=loss * float("nan") if nan else loss)


def _store(model, seed=0):
    """A 4-row store with the three voices in rows 1, 2, 3 (row 0 is somebody else's) and random states."""
    st = StateStore(model, 4)
    st.reserve("other")
    g = torch.Generator().manual_seed(seed)
    for n in NAMES:
        r = st.reserve(n, 10)
        for s in st.cache.states:
            s.att_x_prev[r] = (torch.randn(D, generator=g) * 0.5).bfloat16()
            s.att_kv[r] = torch.randn(H, 64, 64, generator=g) * 0.3
            s.ffn_x_prev[r] = (torch.randn(D, generator=g) * 0.5).bfloat16()
    return st


def _tuner(fields=ALL, seed=0, **kw):
    m = Toy()
    st = _store(m, seed)
    t = StateTuner(m, st, **{**dict(lr=1e-2, weight_decay=0.1, eps=1e-8, fields=fields), **kw})
    for n in NAMES:
        t.add(n)
    return m, st, t


def _batch(step=0, B=5):
    g = torch.Generator().manual_seed(100 + step)
    return dict(inputs_embeds=torch.randn(B, 7, generator=g), labels=torch.randn(B, generator=g))


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------- CSR
def test_csr_groups_rows_by_voice_ascending_with_per_voice_step_counts():
    assert build_csr([2, 0, 2, -1, 0], {0: 7, 2: 9}, {0: 4, 2: 0}) == ([0, 2, 4], [1, 4, 0, 2], [[0, 7, 5], [2, 9, 1]])
    assert build_csr([2, 0, 2, -1, 0, 2], {0: 1, 2: 3}, {0: 0, 2: 0}) == ([0, 2, 5], [1, 4, 0, 2, 5], [[0, 1, 1], [2, 3, 1]])
    assert build_csr([-1, -1], {}, {}) == ([0], [], [])
    m, st, t = _tuner()
    assert [t.row(n) for n in NAMES] == [0, 1, 2] and [st.row(n) for n in NAMES] == [1, 2, 3]
    voice, seg_start, seg_rows, seg_info = t.plan(VOICES)
    assert voice == [2, 0, 2, -1, 0] and seg_start == [0, 2, 4] and seg_rows == [1, 4, 0, 2]
    assert seg_info == [[0, 1, 1], [2, 3, 1]]                 # {master row, store row, the step this update is}
    t.step(voices=["v2", None, None, None, None], **_batch())
    t.step(voices=VOICES, **_batch())
    assert t.steps == [1, 0, 2, 0] and t.step_count("v2") == 2 and t.step_count("v1") == 0
    assert t.plan(VOICES)[3] == [[0, 1, 2], [2, 3, 3]]        # each voice counts its own updates


# ---------------------------------------------------------------------------------------------------------------- errors
def test_step_errors_leave_the_tuner_and_the_model_as_they_were():
    m, st, t = _tuner()
    m.train()
    before = [x.clone() for d in t.master for x in d.values()]
    with pytest.raises(KeyError, match="nobody"):
        t.step(voices=["v0", "nobody", None, None, None], **_batch())
    with pytest.raises(ValueError, match="4 voices for a batch of 5"):
        t.step(voices=VOICES[:4], **_batch())
    with pytest.raises(ValueError, match="past_key_values"):
        t.step(voices=VOICES, past_key_values=None, **_batch())
    st.pin("v0")
    with pytest.raises(RuntimeError, match="pinned"):
        t.step(voices=VOICES, **_batch())
    st.unpin("v0")
    st.evict("v2")
    with pytest.raises(KeyError, match="evicted"):
        t.step(voices=VOICES, **_batch())
    assert not m.calls, "every check fires before the model runs"
    t.publish(["v2"])                                         # back into the lowest free row, from the master
    assert st.row("v2") == 3
    # an exception inside the model: the flags and the mode come back
    with pytest.raises(RuntimeError, match="boom"):
        t.step(voices=VOICES, explode=True, **_batch())
    assert m.calls[-1] == (False, [False, False, False]), "frozen and in eval mode during the call"
    assert m.training and [p.requires_grad for p in m.parameters()] == [True, True, False]
    assert t.steps == [0, 0, 0, 0] and all(torch.equal(a, b) for a, b in zip(before, [x for d in t.master for x in d.values()]))
    # add
    with pytest.raises(ValueError, match="already"):
        t.add("v0")
    with pytest.raises(KeyError):
        StateTuner(m, st).add("unknown", init="store")
    st.pin("v1")
    with pytest.raises(RuntimeError, match="pinned"):
        StateTuner(m, st).add("v1")
    st.unpin("v1")
    with pytest.raises(ValueError, match="fields"):
        StateTuner(m, st, fields=("kv",))


def test_a_store_of_another_geometry_is_refused():
    m = Toy()
    for other in (Toy(layers=3), Toy(d=192), Toy(dtype=torch.float32)):
        with pytest.raises(ValueError, match="needs"):
            StateTuner(m, StateStore(other, 2))
    _, _, t = _tuner()
    sd = t.state_dict()
    m3 = Toy(layers=3)
    with pytest.raises(ValueError, match="fingerprint|store holds"):
        StateTuner(m3, StateStore(m3, 4), fields=ALL).load_state_dict(sd)
    m2 = Toy()
    with pytest.raises(ValueError, match="tunes"):
        StateTuner(m2, StateStore(m2, 4)).load_state_dict(sd)             # other fields
    with pytest.raises(ValueError, match="saved voices"):
        StateTuner(m2, StateStore(m2, 4), fields=ALL, capacity=2).load_state_dict(sd)


def test_init_zeros_reserves_and_zeroes_the_store_row():
    m = Toy()
    st = _store(m)
    t = StateTuner(m, st, fields=ALL, capacity=5)
    st.evict("other")
    assert t.add("fresh", init="zeros") == 0 and st.row("fresh") == 0
    assert t.add("v1", init="zeros") == 1 and st.row("v1") == 2           # a stored name keeps its row and loses its state
    for l in range(L):
        for f in FIELDS:
            assert not getattr(st.cache[l], f)[[0, 2]].any() and not t.master[l][f][:2].any()
            assert getattr(st.cache[l], f)[1].any()
    t.remove("fresh")
    assert t.names() == ["v1"] and "fresh" in st and t.add("v0") == 0


# ---------------------------------------------------------------------------------------------------------------- torch route
@pytest.mark.parametrize("fields", [("att_kv",), ALL])
def test_torch_route_equals_one_torch_adamw_per_voice(fields):
    """Four steps with a changing lr, weight decay > 0 and a batch whose voice sets differ, against leaf caches made by hand, the
    rows' gradients added by hand in batch order, and torch.optim.AdamW per voice (its own step count).  Bars of
    tests/test_trainer_clip_accum.py for the trainer's torch AdamW against torch.optim.AdamW: atol 2e-6, rtol 1e-5."""
    m, st, t = _tuner(fields)
    twin = Toy()
    row0 = [[{f: getattr(s, f)[st.row(n)].clone() for f in FIELDS} for s in st.cache.states] for n in NAMES]
    par = [[{f: torch.nn.Parameter(row0[v][l][f].float()) for f in fields} for l in range(L)] for v in range(3)]
    opts = [torch.optim.AdamW([p for d in par[v] for p in d.values()], lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1) for v in range(3)]
    other = [x.clone() for s in st.cache.states for x in (s.att_x_prev[0], s.att_kv[0], s.ffn_x_prev[0])]
    plans = [VOICES, ["v0", None, "v0", "v0", None], VOICES, ["v1", "v2", None, "v1", "v1"]]
    for step, voices in enumerate(plans):
        lr = 1e-2 * (1 + step)
        t.lr = lr
        batch = _batch(step)
        loss = t.step(voices=voices, **batch)
        idx = [None if n is None else NAMES.index(n) for n in voices]
        states = []
        for l in range(L):
            rows = {f: [] for f in FIELDS}
            for v in idx:
                for f in FIELDS:
                    if v is None:
                        rows[f].append(torch.zeros_like(row0[0][l][f]))
                    else:
                        rows[f].append(par[v][l][f].detach().to(row0[v][l][f].dtype) if f in fields else row0[v][l][f])
            states.append(LayerState(*[torch.stack(rows[f]).requires_grad_(f in fields) for f in FIELDS]))
        want = twin(past_key_values=Cache(states), **batch).loss
        assert torch.equal(loss, want.detach()) if step == 0 else torch.allclose(loss, want.detach(), rtol=1e-5, atol=1e-6)
        want.backward()
        for v in sorted({v for v in idx if v is not None}):
            for l in range(L):
                for f in fields:
                    g = None
                    for b, vb in enumerate(idx):
                        if vb == v:
                            gb = getattr(states[l], f).grad[b].float()
                            g = gb if g is None else g + gb
                    par[v][l][f].grad = g
            for group in opts[v].param_groups:
                group["lr"] = lr
            opts[v].step()
        for v, n in enumerate(NAMES):
            for l in range(L):
                for f in FIELDS:
                    ref = par[v][l][f].detach() if f in fields else row0[v][l][f].float()
                    assert torch.allclose(t.master[l][f][v], ref, atol=2e-6, rtol=1e-5), (step, n, l, f)
                    got = getattr(st.cache[l], f)[st.row(n)]
                    assert torch.equal(_bits(got), _bits(t.master[l][f][v].to(got.dtype))), "the store row is the master, rounded once"
    assert t.steps == [3, 1, 3, 0]
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(other, [x for s in st.cache.states for x in (s.att_x_prev[0], s.att_kv[0], s.ffn_x_prev[0])]))
    assert all(p.grad is None for p in m.parameters()) and m.training
    assert set(t.exp_avg[0]) == set(fields)


def test_packed_batches_count_their_sequences_and_a_nan_loss_steps_on_zero():
    m, st, t = _tuner()
    x = torch.randn(1, 40, generator=torch.Generator().manual_seed(3))
    cu = torch.tensor([0, 5, 12, 12, 30, 40], dtype=torch.int32)
    t.step(voices=VOICES, inputs_embeds=x, labels=torch.zeros(5), cu_seqlens=cu)
    assert t.steps == [1, 0, 1, 0]
    with pytest.raises(ValueError, match="6 voices for a batch of 5"):
        t.step(voices=VOICES + [None], inputs_embeds=x, labels=torch.zeros(5), cu_seqlens=cu)
    # NaN loss: the update of a zero gradient (decay and the moments' decay), nothing becomes NaN
    twin_m, twin_st, twin = _tuner()
    twin.load_state_dict(t.state_dict())
    loss = t.step(voices=VOICES, nan=True, **_batch())
    assert torch.isnan(loss)
    g0 = [{f: torch.zeros_like(getattr(s, f)[:1].expand(5, *getattr(s, f).shape[1:])).contiguous() for f in FIELDS} for s in st.cache.states]
    voice, seg_start, seg_rows, seg_info = twin.plan(VOICES)
    twin._apply(g0, 5, seg_start, seg_rows, seg_info, None, None)
    for l in range(L):
        for f in FIELDS:
            assert torch.isfinite(t.master[l][f]).all() and torch.equal(t.master[l][f], twin.master[l][f])
            assert torch.equal(t.exp_avg[l][f], twin.exp_avg[l][f]) and torch.equal(t.exp_avg_sq[l][f], twin.exp_avg_sq[l][f])


# ---------------------------------------------------------------------------------------------------------------- state_dict
def test_state_dict_round_trip_and_resume_are_bit_for_bit():
    m, st, t = _tuner()
    for step in range(2):
        t.step(voices=VOICES, **_batch(step))
    sd = t.state_dict()
    assert sd["names"] == list(NAMES) and sd["steps"] == [2, 0, 2] and sd["fields"] == list(FIELDS)
    assert sd["fingerprint"] == st.fingerprint and sd["master"]["att_kv"].shape == (L, 3, H, 64, 64)
    assert sd["exp_avg"]["att_x_prev"].shape == (L, 3, D) and all(x.device.type == "cpu" for x in sd["master"].values())
    m2 = Toy()
    st2 = StateStore(m2, 4)                                   # an empty store: load_state_dict publishes the masters into it
    t2 = StateTuner(m2, st2, fields=ALL)
    t2.load_state_dict(sd)
    assert t2.names() == list(NAMES) and t2.steps == [2, 0, 2, 0] and st2.names() == list(NAMES)
    assert (t2.lr, t2.betas, t2.eps, t2.weight_decay) == (t.lr, t.betas, t.eps, t.weight_decay)
    for step in range(2, 4):
        t.step(voices=VOICES, **_batch(step))
        t2.step(voices=VOICES, **_batch(step))
    assert t.steps == t2.steps == [4, 0, 4, 0]
    for l in range(L):
        for f in FIELDS:
            for a, b in ((t.master, t2.master), (t.exp_avg, t2.exp_avg), (t.exp_avg_sq, t2.exp_avg_sq)):
                assert torch.equal(a[l][f], b[l][f])
            for n in NAMES:
                assert torch.equal(_bits(getattr(st.cache[l], f)[st.row(n)]), _bits(getattr(st2.cache[l], f)[st2.row(n)]))


# ---------------------------------------------------------------------------------------------------------------- entries
def test_the_header_declares_both_entries_and_the_library_exports_them(hip_lib):
    names = _lib.exported_symbols()
    assert "rwkv7_state_rows_expand_f32" in names and "rwkv7_state_rows_adamw_f32" in names
    one = ctypes.c_void_p(16)   # never dereferenced: the checks fire first
    f = hip_lib.rwkv7_state_rows_expand_f32

    def expand(layers=2, n=3, master=one, dst=one, voice=one, D=128, H=2):
        return f(layers, n, master, dst, voice, D, H, None)

    assert expand(D=100, H=1) == -4 and expand(D=8200, H=128) == -4 and expand(D=128, H=3) == -3
    assert expand(n=-1) == -1 and expand(master=None) == -1 and expand(dst=None) == -1 and expand(voice=None) == -1
    assert expand(layers=0) == -1 and expand(n=70000) == -1 and expand(n=0, voice=None) == 0
    g = hip_lib.rwkv7_state_rows_adamw_f32

    def adamw(layers=2, n=5, A=2, tbl=(one,) * 5, seg=(one,) * 3, D=128, H=2):
        return g(layers, n, A, *tbl, *seg, None, 1e-3, 0.9, 0.95, 1e-8, 0.0, 1.0, D, H, None)

    assert adamw(D=100, H=1) == -4 and adamw(D=8200, H=128) == -4 and adamw(D=128, H=3) == -3
    for i in range(5):
        assert adamw(tbl=(one,) * i + (None,) + (one,) * (4 - i)) == -1
    for i in range(3):
        assert adamw(seg=(one,) * i + (None,) + (one,) * (2 - i)) == -1
    assert adamw(n=-1) == -1 and adamw(A=-1) == -1 and adamw(A=70000) == -1 and adamw(layers=0) == -1 and adamw(layers=30000) == -1
    assert adamw(n=0, seg=(None,) * 3) == 0 and adamw(A=0, seg=(None,) * 3) == 0
