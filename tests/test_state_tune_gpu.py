"""GPU (-m gpu): state tuning -- rwkv7_state_rows_expand_f32 bit for bit, rwkv7_state_rows_adamw_f32 against an fp64 restatement
(per-voice sum in the listed order, AdamW with per-voice bias correction), its isolation and determinism, and StateTuner end to end
on a tiny bf16 Spark model: frozen weights, the state gradients of the existing differentiable path, a falling loss, serving the
tuned state from a ContinuousDecoder, and a bit-exact resume.

Shapes: 2 layers, 3 stored voices, 5 sequences with voices [2, 0, 2, None, 0] (voice 1 absent, one untuned sequence) and ragged
lengths in 1 .. 70; the kernels also with a sixth row [.., 2] so that one voice owns 3 rows and one 2; D = 128 / H = 2 and
D = 192 / H = 3 (rows end off a tile boundary)."""
import math

import pytest
import torch

from rwkvtts_amd import _lib
from rwkvtts_amd.backbone import Cache, LayerState
from rwkvtts_amd.continuous import ContinuousDecoder
from rwkvtts_amd.decode import step_for
from rwkvtts_amd.prefill import cache_field_table
from rwkvtts_amd.state_store import StateStore
from rwkvtts_amd.state_tune import FIELDS, StateTuner, build_csr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L, V = 2, 3
GEOM = [(128, 2), (192, 3)]
VOICE6 = [2, 0, 2, -1, 0, 2]
ALL = ("att_kv", "att_x_prev", "ffn_x_prev")
I32 = dict(dtype=torch.int32, device=DEV)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _shape(f, n, D, H):
    return (n, H, 64, 64) if f == "att_kv" else (n, D)


def _f32_fields(n, D, H, seed, scale=0.5):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return [{f: torch.randn(_shape(f, n, D, H), generator=g, device=DEV) * scale for f in FIELDS} for _ in range(L)]


def _table(per_layer, fields=FIELDS):
    return torch.tensor([d[f].data_ptr() if f in fields else 0 for d in per_layer for f in FIELDS], dtype=torch.int64, device=DEV)


def _sentinel_cache(n, D, H):
    """A NaN-free pattern that no expanded row can equal by accident."""
    st = []
    for l in range(L):
        x = lambda k: torch.full((n, D), 3.0 + l + k, dtype=torch.bfloat16, device=DEV)
        st.append(LayerState(x(0.5), torch.full((n, H, 64, 64), -7.25 - l, device=DEV), x(0.25)))
    return Cache(st)


# ---------------------------------------------------------------------------------------------------------------- 1. expand
@pytest.mark.parametrize("D,H", GEOM)
def test_expand_copies_kv_bits_rounds_shift_rows_once_and_keeps_what_it_does_not_name(D, H):
    master = _f32_fields(V, D, H, 1)
    for d in master:   # values that round up, down and to even, denormals and a negative zero among them
        d["att_x_prev"][:, :6] = torch.tensor([1.00390625, 1.01171875, 1.0078125 + 2 ** -20, -0.0, 1e-40, 3.3895e38], device=DEV)
        d["att_kv"][:, 0, 0, :3] = torch.tensor([1e-42, -0.0, 3.4e38], device=DEV)
    voice = [2, -1, -2, 0, 2, -7, 1]                          # copies (one repeated), zero, two skipped entries
    n = len(voice)
    cache = _sentinel_cache(n + 1, D, H)                      # the last row is named by no entry
    before = [_bits(t).clone() for s in cache.states for t in (s.att_x_prev, s.att_kv, s.ffn_x_prev)]
    tbl = cache_field_table(cache)
    _lib.call("rwkv7_state_rows_expand_f32", tbl, L, n, _table(master), tbl, torch.tensor(voice, **I32), D, H)
    got = [_bits(t) for s in cache.states for t in (s.att_x_prev, s.att_kv, s.ffn_x_prev)]
    for l in range(L):
        for k, f in enumerate(FIELDS):
            g, b, m = got[3 * l + k], before[3 * l + k], master[l][f]
            want = m if f == "att_kv" else m.bfloat16()
            for i, v in enumerate(voice):
                if v >= 0:
                    assert torch.equal(g[i], _bits(want)[v]), (l, f, i)
                elif v == -1:
                    assert not g[i].any(), (l, f, i)
                else:
                    assert torch.equal(g[i], b[i]), (l, f, i)
            assert torch.equal(g[n], b[n])


# ---------------------------------------------------------------------------------------------------------------- 2., 3. step kernel
class _Case:
    """Masters, moments and a 4-row store cache (voice v -> store row v + 1; row 0 belongs to nobody) plus the kernel's tables."""

    def __init__(self, D, H, seed=10):
        self.D, self.H = D, H
        self.master, self.m, self.v = _f32_fields(V, D, H, seed), _f32_fields(V, D, H, seed + 1, 0.01), _f32_fields(V, D, H, seed + 2, 0.01)
        for d in self.v:
            for f in FIELDS:
                d[f].abs_()
        self.store = _sentinel_cache(V + 1, D, H)
        self.tbl = [_table(self.master), _table(self.m), _table(self.v), cache_field_table(self.store)]

    def step(self, grads, voice, hyper, steps, order=None, skip=None, fields=ALL, store_rows=None):
        store_rows = {v: v + 1 for v in range(V)} if store_rows is None else store_rows
        seg_start, seg_rows, seg_info = build_csr(voice, store_rows, steps)
        if order is not None:                                 # the same segments, listed in another order
            segs = [(seg_rows[seg_start[a]:seg_start[a + 1]], seg_info[a]) for a in order]
            seg_rows, seg_info = [r for s, _ in segs for r in s], [i for _, i in segs]
            seg_start = [0]
            for s, _ in segs:
                seg_start.append(seg_start[-1] + len(s))
        A = len(seg_info)
        dev = [torch.tensor(x, **I32).reshape(-1) for x in (seg_start, seg_rows, seg_info)]
        gt = _table(grads, fields)
        _lib.call("rwkv7_state_rows_adamw_f32", gt, L, len(voice), A, gt, *self.tbl, *dev, skip, hyper["lr"], hyper["b1"], hyper["b2"],
                  hyper["eps"], hyper["wd"], hyper["gs"], self.D, self.H)
        torch.cuda.synchronize()
        return seg_info

    def snapshot(self):
        return [d[f].clone() for per in (self.master, self.m, self.v) for d in per for f in FIELDS] + \
               [_bits(t).clone() for s in self.store.states for t in (s.att_x_prev, s.att_kv, s.ffn_x_prev)]


def _grads(n, D, H, seed, nan=False):
    out = _f32_fields(n, D, H, seed, 0.1)
    for d in out:
        for f in ("att_x_prev", "ffn_x_prev"):
            d[f] = d[f].bfloat16()
        if nan:
            for f in FIELDS:
                d[f].view(-1)[::3] = float("nan")
    return out


def _restate(p, m, v, g_rows, hyper, t, dt):
    """AdamW of one voice and field in `dt` arithmetic from the fp32 inputs: the rows added one after the other, then torch's rule."""
    g = torch.zeros_like(p, dtype=dt)
    for r in g_rows:
        g = g + r.to(dt)
    g = g * hyper["gs"]
    b1, b2 = (torch.tensor(hyper[k], dtype=torch.float32).to(dt) for k in ("b1", "b2"))
    lr, eps, wd = hyper["lr"], hyper["eps"], hyper["wd"]
    if dt == torch.float32:
        lr, eps, wd = (torch.tensor(x, dtype=torch.float32) for x in (lr, eps, wd))
    bc1, bc2 = 1.0 - float(b1.double()) ** t, 1.0 - float(b2.double()) ** t
    p = p.to(dt) * (1 - lr * wd)
    m = b1 * m.to(dt) + (1 - b1) * g
    v = b2 * v.to(dt) + (1 - b2) * g * g
    if dt == torch.float32:
        p = p - (lr * torch.tensor(1.0 / bc1, dtype=dt)) * m / (v.sqrt() * torch.tensor(1.0 / math.sqrt(bc2), dtype=dt) + eps)
    else:
        p = p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return p, m, v


@pytest.mark.parametrize("D,H", GEOM)
def test_step_kernel_vs_fp64_restatement(D, H):
    """Four steps, lr changing, weight decay > 0, random bf16 / fp32 gradients, voices [2, 0, 2, None, 0, 2] and [2, None, 2, None,
    None] alternating (so the voices' step counts differ; the sums run over 3 and 2 rows).  Bar: 2e-6 * max(1, |ref|max) on masters,
    the bar tests/test_fused_gpu.py::test_hip_adamw_matches_torch_adamw applies to the AdamW kernel, and the same relative bound on
    the moments (relative to |ref|max).  The sum of up to 3 rows in fp32 stays inside it, so the bar is not widened.  Measured on an
    MI355X, worst error over both widths: kernel 1.23e-7 / 1.05e-7 / 1.19e-7 (master, m, v), an fp32 restatement of the same order
    1.65e-7 / 1.25e-7 / 2.08e-7; both are printed.  The store row is the master bit for bit (att_kv) / master.bfloat16() (shift
    rows)."""
    c = _Case(D, H)
    ref = [[{f: per[l][f].double().cpu() for f in FIELDS} for l in range(L)] for per in (c.master, c.m, c.v)]
    f32 = [[{f: per[l][f].cpu() for f in FIELDS} for l in range(L)] for per in (c.master, c.m, c.v)]
    steps = {v: 0 for v in range(V)}
    worst = {"kernel": [0.0] * 3, "fp32": [0.0] * 3}
    for it in range(4):
        voice = VOICE6 if it % 2 == 0 else [2, -1, 2, -1, -1]
        hyper = dict(lr=1e-2 / (1 + it), b1=0.9, b2=0.95, eps=1e-8, wd=0.1, gs=0.5 if it == 1 else 1.0)
        grads = _grads(len(voice), D, H, 50 + it)
        info = c.step(grads, voice, hyper, steps)
        for v, _, t in info:
            steps[v] = t
            rows = [i for i, x in enumerate(voice) if x == v]
            for l in range(L):
                for f in FIELDS:
                    g_rows = [grads[l][f][i].cpu() for i in rows]
                    for dt, state in ((torch.float64, ref), (torch.float32, f32)):
                        out = _restate(state[0][l][f][v], state[1][l][f][v], state[2][l][f][v], g_rows, hyper, t, dt)
                        for k in range(3):
                            state[k][l][f][v] = out[k]
        for k, per in enumerate((c.master, c.m, c.v)):
            for l in range(L):
                for f in FIELDS:
                    r = ref[k][l][f]
                    scale = max(1.0, r.abs().max().item()) if k == 0 else r.abs().max().item()   # moments: relative to |ref|max
                    e = (per[l][f].double().cpu() - r).abs().max().item() / scale
                    e32 = (f32[k][l][f].double() - r).abs().max().item() / scale
                    worst["kernel"][k], worst["fp32"][k] = max(worst["kernel"][k], e), max(worst["fp32"][k], e32)
                    assert e <= 2e-6, (it, ("master", "m", "v")[k], l, f, e, e32)
    print(f"D={D}: worst |kernel - fp64| / max(1, |ref|max) master, m, v = {worst['kernel']}; fp32 restatement {worst['fp32']}")
    assert steps == {0: 2, 1: 0, 2: 4}
    for l, s in enumerate(c.store.states):
        for f in FIELDS:
            got, want = getattr(s, f), c.master[l][f] if f == "att_kv" else c.master[l][f].bfloat16()
            assert torch.equal(_bits(got[[1, 3]]), _bits(want[[0, 2]])), (l, f)   # voice v lives in store row v + 1


@pytest.mark.parametrize("D,H", GEOM)
def test_step_kernel_isolation_and_determinism(D, H):
    hyper = dict(lr=1e-2, b1=0.9, b2=0.95, eps=1e-8, wd=0.1, gs=1.0)
    grads = _grads(6, D, H, 70)
    steps = {0: 3, 1: 5, 2: 0}

    def run(voice, **kw):
        c = _Case(D, H)
        before = c.snapshot()
        c.step(grads, voice, hyper, steps, **kw)
        return before, c.snapshot()

    def rows_of(snap, v):   # voice v's rows of master, m, v (9 L tensors) and its store row (3 L)
        return [t[v] for t in snap[:9 * L]] + [t[v + 1] for t in snap[9 * L:]]

    before, base = run(VOICE6)
    # the absent voice and the store row of nobody keep every bit; the others moved
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(rows_of(before, 1), rows_of(base, 1)))
    assert all(torch.equal(a[0], b[0]) for a, b in zip(before[9 * L:], base[9 * L:]))
    assert not any(torch.equal(a, b) for a, b in zip(rows_of(before, 2), rows_of(base, 2)))
    # a voice alone in the launch, the segments listed in the other order, and the same call again: the same bits
    for v in (0, 2):
        _, alone = run([x if x == v else -1 for x in VOICE6])
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(rows_of(alone, v), rows_of(base, v))), v
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(rows_of(alone, 2 - v), rows_of(before, 2 - v)))
    for kw in (dict(order=[1, 0]), {}):
        _, again = run(VOICE6, **kw)
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(again, base)), kw
    # skip_flag with NaN gradients: the zero-gradient step, nothing becomes NaN
    zero = [{f: torch.zeros_like(t) for f, t in d.items()} for d in grads]
    cz, cn = _Case(D, H), _Case(D, H)
    cz.step(zero, VOICE6, hyper, steps)
    cn.step(_grads(6, D, H, 70, nan=True), VOICE6, hyper, steps, skip=torch.ones(1, device=DEV))
    want, got = cz.snapshot(), cn.snapshot()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, want))
    assert all(torch.isfinite(t).all() for t in got[:9 * L])
    # a flag of 0 is no skip; a NULL gradient pointer leaves the field alone, and -1 as store row writes no row
    _, flag0 = run(VOICE6, skip=torch.zeros(1, device=DEV))
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(flag0, base))
    _, kv_only = run(VOICE6, fields=("att_kv",), store_rows={0: 1, 1: 2, 2: -1})
    for k in range(3):                                        # master, m, v
        for l in range(L):
            for j, f in enumerate(FIELDS):
                i = k * 3 * L + 3 * l + j
                assert torch.equal(kv_only[i], base[i] if f == "att_kv" else before[i]), (k, l, f)
    for l in range(L):
        for j, f in enumerate(FIELDS):
            i = 9 * L + 3 * l + j
            assert torch.equal(kv_only[i][3], before[i][3]), "voice 2 has no store row in this call"
            assert torch.equal(kv_only[i][1], base[i][1] if f == "att_kv" else before[i][1])


# ---------------------------------------------------------------------------------------------------------------- 4..6 end to end
NAMES = ("v0", "v1", "v2")
VOICES = ["v2", "v0", "v2", None, "v0"]
LENS = [1, 70, 33, 17, 64]
VOCAB = 300


def _model(D=128, seed=0):
    from rwkvtts_amd.spark_llm import RWKV7ForSpeech, RWKV7SpeechConfig
    cfg = RWKV7SpeechConfig(vocab_size=VOCAB, text_vocab_size=300, audio_global_vocab_size=64, hidden_size=D, num_hidden_layers=L,
                            decay_low_rank_dim=32, a_low_rank_dim=32, v_low_rank_dim=32, gate_low_rank_dim=64)
    m = RWKV7ForSpeech(cfg).init_weights(seed)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        m.lm_head.weight.copy_(torch.randn(m.lm_head.weight.shape, generator=g) * 0.05)
        m.model.embeddings.weight.copy_(torch.randn(m.model.embeddings.weight.shape, generator=g) * 0.5)
    return m.to(DEV).to(torch.bfloat16).train()


def _ids(n, seed):
    return torch.randint(0, VOCAB, (n,), generator=torch.Generator().manual_seed(seed))


def _packed_batch():
    ids = torch.cat([_ids(n, 200 + i) for i, n in enumerate(LENS)]).unsqueeze(0).to(DEV)
    cu = torch.tensor([0] + torch.tensor(LENS).cumsum(0).tolist(), dtype=torch.int32)
    return dict(input_ids=ids, labels=ids.clone(), cu_seqlens=cu)


def _padded_batch():
    ids = torch.stack([_ids(64, 300 + i) for i in range(5)]).to(DEV)
    return dict(input_ids=ids, labels=ids.clone())


def _setup(m, fields=ALL, **kw):
    """A 4-row store whose rows 1..3 hold the voices' captured prompts, and a tuner over them."""
    store = StateStore(m, 4)
    store.reserve("other")
    for i, n in enumerate(NAMES):
        store.capture(n, input_ids=_ids(20 + 7 * i, 400 + i))
    t = StateTuner(m, store, **{**dict(lr=1e-3, fields=fields), **kw})
    for n in NAMES:
        t.add(n)
    return store, t


def _tuner_bits(t, store):
    out = [d[f] for per in (t.master, t.exp_avg, t.exp_avg_sq) for d in per for f in t.fields]
    return out + [_bits(getattr(s, f)[store.row(n)]) for s in store.cache.states for f in FIELDS for n in NAMES]


@pytest.mark.parametrize("D", [128, 192])
@pytest.mark.parametrize("form", ["packed", "padded"])
def test_steps_leave_the_model_alone_and_take_the_gradients_of_the_differentiable_path(D, form):
    m = _model(D)
    batch = _packed_batch() if form == "packed" else _padded_batch()
    store, t = _setup(m)
    params = [p.detach().clone() for p in m.parameters()]
    flags = [p.requires_grad for p in m.parameters()]
    list(m.parameters())[0].requires_grad_(False)             # a flag that was off stays off
    flags[0] = False
    # the first step's gradients, by hand: leaf caches expanded from the masters as they are now, the same forward, backward
    idx = [-1 if n is None else NAMES.index(n) for n in VOICES]
    states = []
    for l in range(L):
        rows = []
        for f in FIELDS:
            src = t.master[l][f] if f == "att_kv" else t.master[l][f].bfloat16()
            r = torch.stack([torch.zeros_like(src[0]) if v < 0 else src[v] for v in idx])
            rows.append(r.requires_grad_())
        states.append(LayerState(*rows))
    m.eval()
    for p in m.parameters():
        p.requires_grad_(False)
    hand = [{f: getattr(st, f) for f in FIELDS} for st in states]   # the forward rebinds the cache's fields to the new states
    loss_hand = m(past_key_values=Cache(states), **batch).loss
    loss_hand.backward()
    for p, f in zip(m.parameters(), flags):
        p.requires_grad_(f)
    m.train()
    losses = [t.step(voices=VOICES, **batch)]
    assert torch.equal(losses[0], loss_hand.detach())
    for l in range(L):
        for f in FIELDS:
            assert hand[l][f].grad.abs().sum() > 0 and torch.equal(_bits(t.last_leaves[l][f].grad), _bits(hand[l][f].grad)), (l, f)
    for _ in range(9):
        losses.append(t.step(voices=VOICES, **batch))
        if len(losses) == 3:
            assert m.training and [p.requires_grad for p in m.parameters()] == flags
            assert all(p.grad is None for p in m.parameters())
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(params, m.parameters()))
    vals = [x.item() for x in losses]
    print(f"D={D} {form}: loss {vals[0]:.4f} -> {vals[-1]:.4f}")
    assert all(math.isfinite(x) for x in vals) and vals[-1] < vals[0], vals
    assert t.steps == [10, 0, 10, 0]
    for l, s in enumerate(store.cache.states):               # the store serves the masters; the absent voice is what was captured
        for f in FIELDS:
            want = t.master[l][f] if f == "att_kv" else t.master[l][f].bfloat16()
            assert torch.equal(_bits(getattr(s, f)[1:]), _bits(want[:3])), (l, f)


def test_serving_a_tuned_state():
    m = _model()
    store, t = _setup(m, fields=("att_kv",))
    for _ in range(3):
        t.step(voices=VOICES, **_packed_batch())
    m.eval()
    suffix, fresh, new = _ids(23, 500), _ids(31, 501), 12
    kw = dict(slots=4, max_new_tokens_cap=32, prefill_buckets=(64, 128))
    eng = ContinuousDecoder(m, admission="eager", state_store=store, **kw)
    h = eng.submit(state="v2", input_ids=suffix, max_new_tokens=new)
    hf = eng.submit(input_ids=fresh, max_new_tokens=new)
    got = eng.run()
    plain = ContinuousDecoder(m, admission="eager", **kw)
    hp = [plain.submit(input_ids=_ids(23, 502), max_new_tokens=new), plain.submit(input_ids=fresh, max_new_tokens=new)]
    assert torch.equal(got[hf], plain.run()[hp[1]]), "the fresh neighbour is what it is without any store"
    # the model's own greedy generation from a cache row expanded from the master: generate()'s host loop (the suffix through the
    # model's forward into the row, then one DecodeStep per token on the argmax), started from that row instead of zeros
    cache = t.expand([t.row("v2"), -1, -1, -1])
    emb = m.get_input_embeddings()
    with torch.no_grad():
        hid = m.model(inputs_embeds=emb(suffix.to(DEV)).unsqueeze(0), cu_seqlens=torch.tensor([0, 23], dtype=torch.int32),
                      past_key_values=cache, cache_rows=torch.tensor([0])).last_hidden_state[0]
        ids = [m.lm_head(hid[-1:]).float().argmax(-1)]
        step = step_for(m.model, m.lm_head, cache)
        x = torch.zeros(4, m.config.hidden_size, dtype=torch.bfloat16, device=DEV)
        for _ in range(new - 1):
            x[0] = emb(ids[-1])[0]
            ids.append(step(x)[:1].float().argmax(-1))
    assert torch.equal(got[h], torch.cat(ids)), (got[h], torch.cat(ids))


def test_resume_is_bit_exact():
    m = _model()
    batches = [_packed_batch(), _padded_batch()]
    store_a, a = _setup(m, weight_decay=0.01)
    for i in range(4):
        a.step(voices=VOICES, **batches[i % 2])
    store_b, b = _setup(m, weight_decay=0.01)
    for i in range(2):
        b.step(voices=VOICES, **batches[i % 2])
    sd = b.state_dict()
    store_c = StateStore(m, 4)
    store_c.reserve("other")
    c = StateTuner(m, store_c, fields=ALL)                    # other hyper-parameters: load_state_dict brings the saved ones
    c.load_state_dict(sd)
    for i in range(2, 4):
        c.step(voices=VOICES, **batches[i % 2])
    assert a.steps == c.steps == [4, 0, 4, 0] and [store_c.row(n) for n in NAMES] == [1, 2, 3]
    assert all(torch.equal(x, y) for x, y in zip(_tuner_bits(a, store_a), _tuner_bits(c, store_c)))
