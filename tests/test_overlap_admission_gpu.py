"""GPU (-m gpu): overlapped admission -- rwkv7_cache_rows_commit_bf16 bit for bit against index_copy_, and
ContinuousDecoder(admission="overlap") against admission="graph" for the same pack compositions: every group of the overlap engine's
admission_log is submitted alone to a graph-mode engine of the same slot count and bucket set, and every request's ids must be equal.
The overlap engine prefills into a staging cache on a side stream while the captured step keeps replaying (and keeps overwriting the
reserved slots' rows with stale values), so equality is what shows that every hazard is ordered."""
import ctypes
import random

import pytest
import torch

from rwkvtts_amd import _lib, backbone
from rwkvtts_amd.backbone import Cache, LayerState
from rwkvtts_amd.continuous import ContinuousDecoder
from rwkvtts_amd.prefill import cache_field_table, cache_rows_commit, check_commit_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---------------------------------------------------------------------------------------------------------------- 1. kernel
def _pattern_cache(L, S, D, H, seed):
    """A cache whose fields hold random BITS (so NaN and Inf patterns of every kind occur), with quiet / signalling NaNs, infinities
    and negative zero planted at the head of every row."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    bf = torch.tensor([0x7FC0, 0x7F81, 0xFFFF, 0x7F80, 0xFF80, 0x8000, 0x0001, 0x7FFF], dtype=torch.int32).to(torch.int16).to(DEV)
    f32 = torch.tensor([0x7FC00000, 0x7F800001, -1, 0x7F800000, -0x800000, -0x80000000, 1, 0x7FFFFFFF], dtype=torch.int64).to(torch.int32).to(DEV)
    states = []
    for _ in range(L):
        xs = [torch.randint(-32768, 32768, (S, D), generator=g, device=DEV, dtype=torch.int32).to(torch.int16) for _ in range(2)]
        kv = torch.randint(-2 ** 31, 2 ** 31, (S, H, 64, 64), generator=g, device=DEV, dtype=torch.int64).to(torch.int32)
        for x in xs:
            x[:, :8] = bf
        kv[:, :, 0, :8] = f32
        states.append(LayerState(xs[0].view(torch.bfloat16), kv.view(torch.float32), xs[1].view(torch.bfloat16)))
    return Cache(states)


def _bits(c):
    return [t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) for s in c.states for t in (s.att_x_prev, s.att_kv, s.ffn_x_prev)]


def _commit(src, dst, src_row, dst_row, D, H):
    src_row, dst_row = check_commit_rows(src_row, dst_row, src[0].att_kv.shape[0], dst[0].att_kv.shape[0])
    i32 = dict(dtype=torch.int32, device=DEV)
    cache_rows_commit(cache_field_table(src), cache_field_table(dst), torch.tensor(src_row, **i32), torch.tensor(dst_row, **i32),
                      len(src_row), len(src), D, H)


@pytest.mark.parametrize("n", [1, 8])
@pytest.mark.parametrize("S", [3, 32, 128])
@pytest.mark.parametrize("D,H", [(64, 1), (192, 3), (1024, 16)])
@pytest.mark.parametrize("L", [1, 3])
def test_row_commit_equals_index_copy_bit_for_bit(L, D, H, S, n):
    src, dst = _pattern_cache(L, 8, D, H, 1), _pattern_cache(L, S, D, H, 2)
    before = [t.clone() for t in _bits(dst)]
    want = [t.clone() for t in before]
    if n == 1:
        # two launches of one active entry each: the last row, then row 0
        calls = [([5, 2, 7], [-1, S - 1, -1]), ([0, 6, 3], [-1, -1, 0])]
    else:
        rng = random.Random(S)
        rows = [S - 1, 0] + rng.sample(range(1, S - 1), min(n, S) - 2)   # not monotonic, with both ends
        rows[1], rows[-1] = rows[-1], rows[1]
        srcs = rng.sample(range(8), len(rows))
        calls = [(srcs[:1] + [4] + srcs[1:-1] + [1] + srcs[-1:], rows[:1] + [-1] + rows[1:-1] + [-1] + rows[-1:])]
    named = set()
    for src_row, dst_row in calls:
        assert sum(d < 0 for d in dst_row) == 2               # two skipped entries in every launch
        _commit(src, dst, src_row, dst_row, D, H)
        act = [(s, d) for s, d in zip(src_row, dst_row) if d >= 0]
        si, di = (torch.tensor(v, device=DEV) for v in zip(*act))
        for w, s in zip(want, _bits(src)):
            w.index_copy_(0, di, s[si])
        named |= {d for _, d in act}
    assert {0, S - 1} <= named and len(named) == min(n, S) + (n == 1)
    other = torch.tensor([r for r in range(S) if r not in named], dtype=torch.int64, device=DEV)
    for got, w, b in zip(_bits(dst), want, before):
        assert torch.equal(got, w)                            # named rows: what index_copy_ gives; integer views, so NaNs compare
        assert torch.equal(got[other], b[other])              # every other row: unchanged
    for s, s0 in zip(_bits(src), _bits(_pattern_cache(L, 8, D, H, 1))):
        assert torch.equal(s, s0)                             # the source is only read


def test_row_commit_argument_errors_do_not_launch():
    D, H, L = 128, 2, 2
    src, dst = _pattern_cache(L, 8, D, H, 3), _pattern_cache(L, 4, D, H, 4)
    before = [t.clone() for t in _bits(dst)]
    st, dt = cache_field_table(src), cache_field_table(dst)
    rows = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    f = _lib.lib().rwkv7_cache_rows_commit_bf16
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert f(L, 2, p(st), p(dt), p(rows), p(rows), 100, 1, stream) == -4      # D % 8 != 0
    assert f(L, 2, p(st), p(dt), p(rows), p(rows), D, 3, stream) == -3        # D != 64 H
    assert f(L, -1, p(st), p(dt), p(rows), p(rows), D, H, stream) == -1       # n < 0
    assert f(L, 2, None, p(dt), p(rows), p(rows), D, H, stream) == -1         # null tables
    assert f(L, 2, p(st), None, p(rows), p(rows), D, H, stream) == -1
    assert f(L, 0, p(st), p(dt), None, None, D, H, stream) == 0               # nothing to do
    with pytest.raises(ValueError):
        cache_rows_commit(st, dt, rows, rows, 2, L, D, 3)
    with pytest.raises(ValueError):
        _commit(src, dst, [0, 1], [4, 0], D, H)                               # a destination row outside the cache: host check
    torch.cuda.synchronize()
    for got, b in zip(_bits(dst), before):
        assert torch.equal(got, b)


# ---------------------------------------------------------------------------------------------------------------- 2..7 engine
def _model(L=2, V=300, seed=0, **dims):
    from rwkvtts_amd.spark_llm import RWKV7ForSpeech, RWKV7SpeechConfig
    d = dict(hidden_size=128, num_hidden_layers=L, decay_low_rank_dim=32, a_low_rank_dim=32, v_low_rank_dim=32, gate_low_rank_dim=64)
    d.update(dims)
    cfg = RWKV7SpeechConfig(vocab_size=V, text_vocab_size=300, audio_global_vocab_size=64, **d)
    m = RWKV7ForSpeech(cfg).init_weights(seed)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        m.lm_head.weight.copy_(torch.randn(m.lm_head.weight.shape, generator=g) * 0.05)
        m.model.embeddings.weight.copy_(torch.randn(m.model.embeddings.weight.shape, generator=g) * 0.5)
    return m.to(DEV).to(torch.bfloat16).eval()


@pytest.fixture(scope="module")
def small():
    return _model()


def _requests(n, D, seed, lo=3, hi=80, budgets=(5, 40)):
    """n requests: prompts of lo..hi tokens, budgets in `budgets`, every other one sampled (with its own key and warper settings)."""
    g = torch.Generator().manual_seed(seed)
    rng = random.Random(seed)
    reqs = []
    for i in range(n):
        t = rng.randint(lo, hi)
        kw = dict(inputs_embeds=(torch.randn(t, D, generator=g) * 0.5).to(DEV, torch.bfloat16), max_new_tokens=rng.randint(*budgets))
        if i % 2:
            top_k, top_p = rng.choice([0, 5, 50]), rng.choice([1.0, 0.9])
            kw.update(do_sample=True, seed=1000 + i, top_k=top_k, top_p=top_p if top_k else 1.0,   # top_p needs top_k
                      temperature=rng.choice([0.8, 1.0, 1.3]))
        reqs.append(kw)
    return reqs


class _GraphRef:
    """One graph-mode engine per (slots, buckets, ...) and the ids it gives each pack composition, computed once."""

    def __init__(self, m, reqs, **kw):
        self.eng, self.reqs, self.ids = ContinuousDecoder(m, admission="graph", **kw), reqs, {}

    def group(self, handles):
        key = tuple(handles)
        if key not in self.ids:
            assert self.eng.sched.idle
            hs = [self.eng.submit(**self.reqs[h]) for h in handles]
            out = self.eng.run()
            assert sorted(self.eng.sched.free) == list(range(self.eng.slots))
            self.ids[key] = [out[h] for h in hs]
        return self.ids[key]


def _check_groups(eng, got, ref, only=None):
    n = 0
    for _, _, group in eng.admission_log:
        if only is not None and not set(group) & set(only):
            continue
        for h, want in zip(group, ref.group(group)):
            assert got[h].dtype == torch.int64 and torch.equal(got[h], want), (h, group, got[h], want)
            n += 1
    return n


def _overlapped(eng):
    """Groups launched while a slot was busy and committed at least one replay later (replays are only issued while a slot is busy)."""
    return [(a, b, g) for a, b, g in eng.admission_log if b > a]


SMALL = dict(slots=4, max_new_tokens_cap=64, prefill_buckets=(64, 128, 256))
_refs = {}


def _small_ref(m):
    if "small" not in _refs:
        _refs["small"] = _GraphRef(m, _requests(12, m.config.hidden_size, 5), **SMALL)
    return _refs["small"]


@pytest.mark.parametrize("lag", [8, 0, 64])
def test_overlap_equals_graph_mode_per_composition(small, lag):
    ref = _small_ref(small)
    eng = ContinuousDecoder(small, admission="overlap", overlap_replays=lag, **SMALL)
    hs = [eng.submit(**kw) for kw in ref.reqs]
    assert hs == list(range(12))
    got = eng.run()
    assert sorted(got) == hs and [got[h].numel() for h in hs] == [kw["max_new_tokens"] for kw in ref.reqs]
    assert [h for _, _, g in eng.admission_log for h in g] == hs
    if lag == 0:
        assert not _overlapped(eng)                           # committed in the step that launched them
    else:
        assert _overlapped(eng), eng.admission_log            # otherwise nothing here ran next to a prefill
    if lag == 8:
        assert any(b - a == 8 for a, b, _ in eng.admission_log)
    if lag == 64:
        assert all(b - a < 64 for a, b, _ in eng.admission_log)   # budgets <= 40: every commit came because nothing was busy
    assert _check_groups(eng, got, ref) == 12
    assert not eng.dstep.barrier_timed_out()


def test_long_prompt_continues_from_its_staging_row(small):
    """A prompt longer than the largest bucket is several replays on the side stream, each continuing from the staging row."""
    D = small.config.hidden_size
    reqs = _requests(3, D, 7, budgets=(50, 60))
    reqs[2]["inputs_embeds"] = (torch.randn(300, D, generator=torch.Generator().manual_seed(8)) * 0.5).to(DEV, torch.bfloat16)
    kw = dict(slots=4, max_new_tokens_cap=64, prefill_buckets=(64, 128))
    eng = ContinuousDecoder(small, admission="overlap", overlap_replays=8, **kw)
    assert len(eng.prefill.plan([300], [0])) > 1
    h0, h1 = eng.submit(**reqs[0]), eng.submit(**reqs[1])
    assert eng.step() == [] and sorted(eng.sched.busy) == [0, 1]
    h2 = eng.submit(**reqs[2])
    got = eng.run()
    assert eng.admission_log[0][2] == [h0, h1] and eng.admission_log[1][2] == [h2]
    a, b, _ = eng.admission_log[1]
    assert a > 0 and b - a == 8                               # launched next to running slots, committed eight replays later
    assert _check_groups(eng, got, _GraphRef(small, reqs, **kw)) == 3


def test_eos_retirement_with_slot_reuse(small):
    """Ids restricted to six values, one of them the EOS id, sampled hot: every request meets its EOS well inside its budget, and five
    requests go through two slots, so slots are reused after a read-back retirement."""
    D, E = small.config.hidden_size, 103
    sup = [t for t in range(300) if not 100 <= t < 106]
    reqs = _requests(5, D, 11)
    for i, kw in enumerate(reqs):
        kw.update(max_new_tokens=120, min_new_tokens=(0, 3, 9, 0, 5)[i], do_sample=True, seed=50 + i, top_k=0, top_p=1.0, temperature=2.0)
    kw = dict(slots=2, max_new_tokens_cap=128, prefill_buckets=(64, 128, 256), eos_token_id=E, suppress_tokens=sup, check_every=4)
    eng = ContinuousDecoder(small, admission="overlap", overlap_replays=8, **kw)
    hs = [eng.submit(**r) for r in reqs]
    got = eng.run()
    assert sorted(got) == hs and len(eng.admission_log) >= 3
    for h, r in zip(hs, reqs):
        ids = got[h].tolist()
        assert ids[-1] == E and ids.count(E) == 1 and len(ids) < 120 and len(ids) > r["min_new_tokens"], (h, ids)
        assert all(100 <= t < 106 for t in ids)
    assert _overlapped(eng)
    assert _check_groups(eng, got, _GraphRef(small, reqs, **kw)) == 5


def test_64_slots_wide_step(small):
    reqs = _requests(70, small.config.hidden_size, 13, lo=3, hi=40)
    kw = dict(slots=64, max_new_tokens_cap=64, prefill_buckets=(64, 128, 256))
    eng = ContinuousDecoder(small, admission="overlap", overlap_replays=8, **kw)
    hs = [eng.submit(**r) for r in reqs]
    got = eng.run()
    assert sorted(got) == hs and all(got[h].numel() == r["max_new_tokens"] for h, r in zip(hs, reqs))
    assert max(len(g) for _, _, g in eng.admission_log) == 8 and _overlapped(eng)
    picked = random.Random(0).sample(hs, 10)
    assert _check_groups(eng, got, _GraphRef(small, reqs, **kw), only=picked) >= 10


def test_04b_widths_depth_4():
    c = backbone.config_0p4b()
    m = _model(L=4, V=8193, hidden_size=c.hidden_size, decay_low_rank_dim=c.decay_low_rank_dim, a_low_rank_dim=c.a_low_rank_dim,
               v_low_rank_dim=c.v_low_rank_dim, gate_low_rank_dim=c.gate_low_rank_dim, intermediate_size=c.intermediate_size)
    reqs = _requests(40, m.config.hidden_size, 17, lo=4, hi=200, budgets=(1, 48))
    kw = dict(slots=32, max_new_tokens_cap=64, prefill_buckets=(256, 512))
    eng = ContinuousDecoder(m, admission="overlap", **kw)
    assert eng.overlap_replays == 8
    hs = [eng.submit(**r) for r in reqs]
    got = eng.run()                                           # raises on a barrier timeout
    assert sorted(got) == hs and all(got[h].numel() == r["max_new_tokens"] for h, r in zip(hs, reqs))
    assert not eng.dstep.barrier_timed_out() and _overlapped(eng)
    assert _check_groups(eng, got, _GraphRef(m, reqs, **kw)) == 40
