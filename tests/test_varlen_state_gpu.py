"""Packed rows (cu_seqlens) that carry one recurrent state per sequence, on the MI355X: the two state+seq C entries against fp64
autograd of the oracle scan, bit identity with the stateless packed entries and with the per-sequence op, and the model's stateful
packed path against per-sequence stateful forwards, DecodeStep continuation and fp32 CPU autograd of the oracle."""
import ctypes

import pytest
import torch

from oracle import rwkv7_ref as R
from rwkvtts_amd import _lib, ops
from rwkvtts_amd.backbone import Cache, LayerState
from rwkvtts_amd.synthetic import make_wkv_inputs
from test_model_gpu import _spark_pair
from test_wkv7_gpu import _assert_bf16_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES6 = ("dr", "dw", "dk", "dv", "da", "db")
LENS = [1, 17, 32, 33, 100, 0, 256]


def _c(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp(min=1e-30)).item()


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def _identity_rows(xs, rows):
    """q w k v a b [1,T,H,64] with identity steps (w = W_PAD, the rest 0) at `rows`."""
    for x, f in zip(xs, (0.0, ops.W_PAD, 0.0, 0.0, 0.0, 0.0)):
        x[:, rows] = f


def _run_entries(ins, dy, seq_chunks, h0, dhT):
    """fwd_state_seq + bseq_state_seq on one packed row (B = 1); h0 / dhT may be None. Returns y, hT, dh0, sa, hs, e_vk, z."""
    q, w, k, v, a, b = ins
    _, T, H, _ = q.shape
    lib, st = _lib.lib(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nseq = len(seq_chunks) - 1
    so = torch.tensor(seq_chunks, dtype=torch.int32, device=DEV)
    tinv = ops.wkv7_chunk_prep(w, a, b)
    y, sa = torch.empty_like(v), torch.empty(1, T, H, 64, device=DEV)
    hs = torch.empty(1, H, T // 32, ops.Q15_REC, dtype=torch.int16, device=DEV)
    e_vk, z = torch.empty_like(hs), torch.empty(1, T, H, 64, device=DEV)
    hT = torch.full((nseq, H, 64, 64), float("nan"), device=DEV) if h0 is not None else None
    dh0 = torch.full((nseq, H, 64, 64), float("nan"), device=DEV) if dhT is not None else None
    assert lib.rwkv7_wkv_chunk_fwd_state_seq_bf16(1, T, H, _c(w), _c(q), _c(k), _c(v), _c(a), _c(b), _c(tinv), _c(y), _c(sa), _c(hs),
                                                  _c(so), nseq, _c(h0), _c(hT), st) == 0
    assert lib.rwkv7_wkv_chunk_bseq_state_seq_bf16(1, T, H, _c(w), _c(q), _c(a), _c(b), _c(dy), _c(tinv), _c(e_vk), _c(z), _c(so),
                                                   nseq, _c(dhT), _c(dh0), st) == 0
    torch.cuda.synchronize()
    return y, hT, dh0, sa, hs, e_vk, z


def test_state_seq_entries_on_an_unframed_packed_row_vs_fp64():
    """The entries directly, on a packed row with NO identity chunks: hT and dh0 of every sequence against fp64 autograd of the oracle
    scan of that sequence alone -- three real sequences (64, 32 and 96 steps), an empty one between them, and a masked tail
    pseudo-sequence of identity steps (its hT must be its h0 bit for bit after passing 64 identity steps)."""
    H, T = 4, 256
    seq_chunks = [0, 2, 2, 3, 6, 8]   # A: 0-1, B: empty, C: 2, D: 3-5, tail: 6-7
    w, q, k, v, a, b = [t.clone() for t in make_wkv_inputs(1, T, H, 61, torch.bfloat16)]
    _identity_rows((q, w, k, v, a, b), slice(192, 256))
    g = torch.Generator().manual_seed(62)
    h0, dhT = torch.randn(5, H, 64, 64, generator=g), torch.randn(5, H, 64, 64, generator=g)
    dy = torch.randn(1, T, H, 64, generator=g).bfloat16()
    y, hT, dh0, *_ = _run_entries([t.to(DEV) for t in (q, w, k, v, a, b)], dy.to(DEV), seq_chunks, h0.to(DEV), dhT.to(DEV))
    for s in range(5):
        lo, hi = seq_chunks[s] * 32, seq_chunks[s + 1] * 32
        if lo == hi:
            assert torch.equal(hT[s].cpu(), h0[s]) and torch.equal(dh0[s].cpu(), dhT[s]), "empty sequence: hT = h0, dh0 = dhT"
            continue
        xs = [t[:, lo:hi].double().requires_grad_() for t in (q, w, k, v, a, b)]
        s0 = h0[s:s + 1].double().requires_grad_()
        y_o, hT_o = R.wkv7_scan(*xs, state=s0)
        ((y_o * dy[:, lo:hi].double()).sum() + (hT_o * dhT[s:s + 1].double()).sum()).backward()
        _assert_bf16_close(y[:, lo:hi], y_o.detach(), f"y[{s}]")
        e_hT, e_dh0 = _rel(hT[s:s + 1], hT_o), _rel(dh0[s:s + 1], s0.grad)
        print(f"sequence {s} ({hi - lo} steps): hT rel. L2 {e_hT:.2e}, dh0 rel. L2 {e_dh0:.2e}")
        assert e_hT <= 2e-3 and e_dh0 <= 2e-3, (s, e_hT, e_dh0)
    # the tail pseudo-sequence: identity steps only, the state passes through exactly, y = 0
    assert torch.equal(hT[4].cpu(), h0[4]) and torch.equal(dh0[4].cpu(), dhT[4])
    assert torch.equal(y[:, 192:].float().cpu(), torch.zeros(1, 64, H, 64))


def test_null_state_seq_pointers_are_bit_identical_to_the_stateless_seq_entries():
    """NULL states dispatch to the stateless packed kernels; ZERO states run the stateful instantiations on packed rows -- both must
    equal rwkv7_wkv_chunk_fwd_seq_bf16 / rwkv7_wkv_chunk_bseq_bf16 with the same seq_chunk_off bit for bit (y, sa, hs, e_vk, z and
    the six gradients of the per-chunk kernel on top)."""
    H, T = 4, 320
    seq_chunks = [0, 3, 3, 4, 7, 10]
    w, q, k, v, a, b = [t.to(DEV) for t in make_wkv_inputs(1, T, H, 71, torch.bfloat16)]
    ins = [q, w, k, v, a, b]
    dy = torch.randn(1, T, H, 64, generator=torch.Generator().manual_seed(72)).bfloat16().to(DEV)
    lib, st = _lib.lib(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def grads(sa, hs, e_vk, z):
        gs = [torch.empty_like(w) for _ in range(6)]
        assert lib.rwkv7_wkv_chunk_bwd_out_z_bf16(1, T, H, _c(w), _c(q), _c(k), _c(v), _c(a), _c(b), _c(dy), _c(hs), _c(sa), _c(z),
                                                  _c(e_vk), *[_c(g_) for g_ in gs], st) == 0
        torch.cuda.synchronize()
        return gs

    so = torch.tensor(seq_chunks, dtype=torch.int32, device=DEV)
    tinv = ops.wkv7_chunk_prep(w, a, b)
    y, sa = torch.empty_like(v), torch.empty(1, T, H, 64, device=DEV)
    hs = torch.empty(1, H, T // 32, ops.Q15_REC, dtype=torch.int16, device=DEV)
    e_vk, z = torch.empty_like(hs), torch.empty(1, T, H, 64, device=DEV)
    assert lib.rwkv7_wkv_chunk_fwd_seq_bf16(1, T, H, _c(w), _c(q), _c(k), _c(v), _c(a), _c(b), _c(tinv), _c(y), _c(sa), _c(hs),
                                            _c(so), 5, st) == 0
    assert lib.rwkv7_wkv_chunk_bseq_bf16(1, T, H, _c(w), _c(q), _c(a), _c(b), _c(dy), _c(tinv), _c(e_vk), _c(z), _c(so), 5, st) == 0
    torch.cuda.synchronize()
    old = [y, sa, hs, e_vk, z] + grads(sa, hs, e_vk, z)
    names = ("y", "sa", "hs", "e_vk", "z") + NAMES6
    for mode in ("null", "zero"):
        zs = torch.zeros(5, H, 64, 64, device=DEV) if mode == "zero" else None
        y2, hT, dh0, sa2, hs2, e2, z2 = _run_entries(ins, dy, seq_chunks, zs, zs)
        new = [y2, sa2, hs2, e2, z2] + grads(sa2, hs2, e2, z2)
        for n, x, x0 in zip(names, new, old):
            assert torch.equal(_bits(x), _bits(x0)), f"{mode}: {n} differs"
        if mode == "zero":
            assert torch.equal(hT[1], zs[1]) and torch.equal(dh0[1], zs[1])   # the empty sequence


def _varlen_case(H, seed):
    T = sum(LENS)
    w, q, k, v, a, b = make_wkv_inputs(1, T, H, seed, torch.bfloat16)
    g = torch.Generator().manual_seed(seed + 50)
    h0 = torch.randn(len(LENS), H, 64, 64, generator=g)
    dy = torch.randn(1, T, H * 64, generator=g).bfloat16()
    dhT = torch.randn(len(LENS), H, 64, 64, generator=g)
    cu = torch.tensor([0] + list(torch.tensor(LENS).cumsum(0).tolist()), dtype=torch.int32)
    flat = lambda t: t.reshape(1, T, H * 64)
    return [flat(t) for t in (q, w, k, v, a, b)], h0, dy, dhT, cu


def _loss_backward(y, hT, dy, dhT):
    loss = (y.float() * dy.float()).sum()
    if dhT is not None:
        loss = loss + (hT * dhT).sum()
    loss.backward()


@pytest.mark.parametrize("with_dhT", [True, False])
def test_varlen_op_is_bit_identical_to_per_sequence_op(with_dhT):
    """wkv7_state_chunked_varlen against N calls of wkv7_state_chunked: y, hT, dh0 and the six input gradients bit for bit (an
    identity chunk passes the state through exactly and each (sequence, head) runs the same per-chunk arithmetic); forward-only
    calls too."""
    H = 4
    ins, h0, dy, dhT, cu = _varlen_case(H, seed=81)
    dhT = dhT if with_dhT else None
    xs = [t.to(DEV).requires_grad_() for t in ins]
    s0 = h0.to(DEV).requires_grad_()
    y, hT = ops.wkv7_state_chunked_varlen(s0, *xs, cu)
    _loss_backward(y, hT, dy.to(DEV), None if dhT is None else dhT.to(DEV))
    with torch.no_grad():
        y_nt, hT_nt = ops.wkv7_state_chunked_varlen(h0.to(DEV), *[t.to(DEV) for t in ins], cu.to(DEV))   # device cu_seqlens too
    torch.cuda.synchronize()
    assert torch.equal(_bits(y_nt), _bits(y.detach())) and torch.equal(hT_nt, hT.detach()), "forward-only differs from training"
    cl = cu.tolist()
    for i, n in enumerate(LENS):
        lo, hi = cl[i], cl[i + 1]
        if n == 0:
            assert torch.equal(hT[i], s0[i].detach())
            assert torch.equal(s0.grad[i], dhT[i].to(DEV) if dhT is not None else torch.zeros_like(s0.grad[i]))
            continue
        xi = [t[:, lo:hi].detach().clone().requires_grad_() for t in xs]
        si = s0[i:i + 1].detach().clone().requires_grad_()
        yi, hTi = ops.wkv7_state_chunked(si, *xi)
        _loss_backward(yi, hTi, dy[:, lo:hi].to(DEV), None if dhT is None else dhT[i:i + 1].to(DEV))
        torch.cuda.synchronize()
        assert torch.equal(_bits(y[:, lo:hi].detach()), _bits(yi.detach())), f"y of sequence {i} (n={n})"
        assert torch.equal(hT[i:i + 1].detach(), hTi.detach()), f"hT of sequence {i} (n={n})"
        assert torch.equal(s0.grad[i:i + 1], si.grad), f"dh0 of sequence {i} (n={n})"
        for nm, gv, gi in zip(NAMES6, xs, xi):
            assert torch.equal(_bits(gv.grad[:, lo:hi]), _bits(gi.grad)), f"{nm} of sequence {i} (n={n})"


@pytest.mark.parametrize("with_dhT", [True, False])
def test_varlen_op_vs_fp64_autograd(with_dhT):
    """The op against fp64 autograd of the oracle scan, sequence by sequence: y within 1 bf16 ulp, the six gradients within 2 (the
    bars of test_state_op_vs_fp64_autograd), hT and dh0 at relative L2 <= 2e-3."""
    H = 4
    ins, h0, dy, dhT, cu = _varlen_case(H, seed=91)
    dhT = dhT if with_dhT else None
    xs = [t.to(DEV).requires_grad_() for t in ins]
    s0 = h0.to(DEV).requires_grad_()
    y, hT = ops.wkv7_state_chunked_varlen(s0, *xs, cu)
    _loss_backward(y, hT, dy.to(DEV), None if dhT is None else dhT.to(DEV))
    torch.cuda.synchronize()
    cl = cu.tolist()
    un = lambda t: t.detach().cpu().view(1, -1, H, 64)
    for i, n in enumerate(LENS):
        if n == 0:
            continue
        lo, hi = cl[i], cl[i + 1]
        xo = [un(t[:, lo:hi]).double().requires_grad_() for t in ins]
        so = h0[i:i + 1].double().requires_grad_()
        y_o, hT_o = R.wkv7_scan(*xo, state=so)
        loss = (y_o * un(dy[:, lo:hi]).double()).sum() + ((hT_o * dhT[i:i + 1].double()).sum() if dhT is not None else 0.0)
        loss.backward()
        _assert_bf16_close(un(y[:, lo:hi]), y_o.detach(), f"y[{i}]")
        for nm, gv, go in zip(NAMES6, xs, xo):
            _assert_bf16_close(un(gv.grad[:, lo:hi]), go.grad, f"{nm}[{i}]", ulps=2.0)
        e_hT, e_dh0 = _rel(hT[i:i + 1], hT_o), _rel(s0.grad[i:i + 1], so.grad)
        print(f"n={n} dhT={with_dhT}: hT rel. L2 {e_hT:.2e}, dh0 rel. L2 {e_dh0:.2e}")
        assert e_hT <= 2e-3 and e_dh0 <= 2e-3, (n, e_hT, e_dh0)


# ---------------------------------------------------------------------------------------------------------------- model
DIMS = dict(hidden_size=128, num_hidden_layers=2, decay_low_rank_dim=32, a_low_rank_dim=32, v_low_rank_dim=32, gate_low_rank_dim=64)


def _decode_pair(seed=11):
    """A 2-layer bf16 Spark model the one-kernel decode step supports (ranks >= 32), and the oracle's parameters."""
    from rwkvtts_amd.spark_llm import RWKV7ForSpeech, RWKV7SpeechConfig
    V = 257
    cfg = RWKV7SpeechConfig(vocab_size=V, text_vocab_size=300, audio_global_vocab_size=64, **DIMS)
    rcfg = R.RefConfig(vocab_size=V, **DIMS)
    p = R.init_params(rcfg, seed=seed)
    p["lm_head.weight"] = torch.randn(V, 128, generator=torch.Generator().manual_seed(seed + 1)) * 0.05
    p = {k: v.to(torch.bfloat16).float() for k, v in p.items()}
    model = RWKV7ForSpeech(cfg)
    sd = dict(p)
    for n in ("text_embedder", "global_embedder", "tts_tag_embedder"):
        sd[n + ".weight"] = getattr(model, n).weight.detach().clone()
    model.load_state_dict(sd, strict=True)
    return model.to(DEV).to(torch.bfloat16).eval(), p, rcfg


def _random_cache(cfg, N, seed, differentiable=False, leaves=False):
    g = torch.Generator().manual_seed(seed)
    H, D = cfg.num_heads, cfg.hidden_size
    states = []
    for _ in range(cfg.num_hidden_layers):
        t = [(torch.randn(N, D, generator=g) * 0.5).to(DEV, torch.bfloat16), (torch.randn(N, H, 64, 64, generator=g) * 0.3).to(DEV),
             (torch.randn(N, D, generator=g) * 0.5).to(DEV, torch.bfloat16)]
        if leaves:
            t = [x.requires_grad_() for x in t]
        states.append(LayerState(*t))
    return Cache(states, differentiable=differentiable)


def _row(cache, i):
    return Cache([LayerState(s.att_x_prev[i:i + 1].detach().clone(), s.att_kv[i:i + 1].detach().clone(),
                             s.ffn_x_prev[i:i + 1].detach().clone()) for s in cache.states])


def test_model_packed_prefill_with_cache_matches_per_sequence_and_decode_continues():
    """No grad: a packed row with a random cache against each sequence alone as [1, n_i] with its cache row -- hidden states and every
    cache field at relative L2 < 1.5e-2 (the per-sequence path runs the scalar state kernel), in place: the tensors keep their
    addresses -- then DecodeStep from the packed cache against DecodeStep from the
    per-sequence caches: next-token logits within the bars of test_decode_step_gpu.py."""
    from rwkvtts_amd.decode import DecodeStep
    model, p, rcfg = _decode_pair()
    bb = model.model
    lens = [5, 0, 40, 32, 77, 1]
    N, total = len(lens), sum(lens) + 3   # three trailing positions outside cu_seqlens come back as zeros
    x = (torch.randn(1, total, 128, generator=torch.Generator().manual_seed(5)) * 0.5).to(DEV, torch.bfloat16)
    cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32)
    cache = _random_cache(bb.config, N, seed=7)
    ptrs = [(s.att_x_prev.data_ptr(), s.att_kv.data_ptr(), s.ffn_x_prev.data_ptr()) for s in cache.states]
    rows = [_row(cache, i) for i in range(N)]
    with torch.no_grad():
        out = bb(inputs_embeds=x, cu_seqlens=cu.to(DEV), past_key_values=cache)
    assert out.past_key_values is cache and cache.seen_tokens == sum(lens)
    assert [(s.att_x_prev.data_ptr(), s.att_kv.data_ptr(), s.ffn_x_prev.data_ptr()) for s in cache.states] == ptrs
    h = out.last_hidden_state
    assert torch.equal(h[0, sum(lens):].float(), torch.zeros(3, 128, device=DEV))
    cl = cu.tolist()
    for i, n in enumerate(lens):
        if n:
            with torch.no_grad():
                hi = bb(inputs_embeds=x[:, cl[i]:cl[i + 1]], past_key_values=rows[i], use_cache=True).last_hidden_state
            e_h = _rel(h[:, cl[i]:cl[i + 1]], hi)
            assert e_h < 1.5e-2, (i, e_h)
        for l_, (sp, sr) in enumerate(zip(cache.states, rows[i].states)):
            if n == 0:   # untouched, bit for bit
                assert torch.equal(sp.att_kv[i:i + 1], sr.att_kv) and torch.equal(sp.att_x_prev[i:i + 1], sr.att_x_prev)
                assert torch.equal(sp.ffn_x_prev[i:i + 1], sr.ffn_x_prev)
                continue
            for nm in ("att_kv", "att_x_prev", "ffn_x_prev"):   # the bar of the differentiable-cache vs no-grad test
                e = _rel(getattr(sp, nm)[i:i + 1], getattr(sr, nm))
                assert e < 1.5e-2, (i, l_, nm, e)
    # continue both with the one-kernel decode step (one step per sequence)
    ids = torch.randint(0, 257, (N,), generator=torch.Generator().manual_seed(9)).to(DEV)
    xe = torch.nn.functional.embedding(ids, bb.embeddings.weight)
    step = DecodeStep(bb, model.lm_head, cache)
    with torch.no_grad():
        lp = step(xe).float().clone()
    for i in range(N):
        si = DecodeStep(bb, model.lm_head, rows[i])
        with torch.no_grad():
            li = si(xe[i:i + 1]).float()
        scale = li.abs().max().item()
        assert (lp[i] - li[0]).abs().max().item() < 2e-2 * scale, (i, (lp[i] - li[0]).abs().max().item(), scale)


def test_model_two_packed_segments_through_the_state_vs_oracle_autograd():
    """Training: two packed segments carried WITHOUT detach from random initial states (leaf tensors, differentiable cache) -- loss,
    every parameter gradient and the initial-state gradients against fp32 CPU autograd of the oracle run sequence by sequence.
    Bars of test_spark_model_two_segments_through_the_state_vs_oracle_autograd: relative L2, median < 2.5e-2, worst < 0.10."""
    model, p, rcfg = _spark_pair(seed=13)
    model = model.to(torch.bfloat16).train()
    bb = model.model
    seg = [[20, 0, 64, 7], [33, 5, 0, 40]]   # segment 1 / segment 2 lengths of the four sequences
    N = 4
    g = torch.Generator().manual_seed(17)
    xs = [(torch.randn(1, sum(s), 128, generator=g) * 0.5).bfloat16().float() for s in seg]
    proj = torch.randn(128, generator=g)
    cache = _random_cache(bb.config, N, seed=19, differentiable=True, leaves=True)
    leaves = [t for s in cache.states for t in (s.att_x_prev, s.att_kv, s.ffn_x_prev)]
    st0 = [t.detach().float().cpu() for t in leaves]
    loss = 0.0
    for x, lens in zip(xs, seg):
        cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32)
        h = bb(inputs_embeds=x.to(DEV, torch.bfloat16), cu_seqlens=cu, past_key_values=cache).last_hidden_state
        loss = loss + (h.float() * proj.to(DEV)).pow(2).mean()
    assert cache.seen_tokens == sum(map(sum, seg)) and cache[0].att_kv.grad_fn is not None
    loss.backward()
    # oracle: every sequence alone, two segments, from its own row of the initial states
    pr = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    sr = [t.clone().requires_grad_(True) for t in st0]
    loss_o = 0.0
    rows_st = [[t[i:i + 1] for t in sr] for i in range(N)]
    offs = [[0] + torch.tensor(s).cumsum(0).tolist() for s in seg]
    for si, (x, lens) in enumerate(zip(xs, seg)):
        hs = []
        for i in range(N):
            if lens[i] == 0:
                continue
            hi, rows_st[i] = R.backbone(pr, rcfg, x[:, offs[si][i]:offs[si][i + 1]], None, rows_st[i])
            hs.append(hi)
        loss_o = loss_o + (torch.cat(hs, 1) * proj).pow(2).mean()
    loss_o.backward()
    assert abs(loss.item() - loss_o.item()) < 2e-2 * abs(loss_o.item()), (loss.item(), loss_o.item())
    named = dict(model.named_parameters())
    rels = {k: _rel(named[k].grad.float(), v.grad) for k, v in pr.items()
            if v.grad is not None and k not in ("model.embeddings.weight", "lm_head.weight")}
    for i, (a, b) in enumerate(zip(leaves, sr)):
        rels[f"state[{i}]"] = _rel(a.grad.float(), b.grad)
    vals = sorted(rels.values())
    top = sorted(rels.items(), key=lambda kv: -kv[1])[:5]
    print(f"loss {loss.item():.5f} (oracle {loss_o.item():.5f}); rel. L2 median {vals[len(vals) // 2]:.2e}, worst {top}")
    assert len(rels) >= 40
    assert vals[len(vals) // 2] < 2.5e-2, f"median {vals[len(vals) // 2]:.3e}; worst five {top}"
    assert top[0][1] < 0.10, f"worst five {top}"


def test_packed_cache_errors():
    model, p, rcfg = _spark_pair(seed=3)   # fp32
    x = torch.randn(1, 32, 128, device=DEV)
    cu = torch.tensor([0, 20, 32], dtype=torch.int32)
    with pytest.raises(ValueError, match="bf16"):
        model.model(inputs_embeds=x, cu_seqlens=cu, past_key_values=Cache.zeros(model.config, 2, DEV, torch.float32))
    mb = model.to(torch.bfloat16)
    for B in (1, 3):
        with pytest.raises(ValueError, match="cu_seqlens"):
            with torch.no_grad():
                mb.model(inputs_embeds=x.bfloat16(), cu_seqlens=cu, past_key_values=Cache.zeros(model.config, B, DEV, torch.bfloat16))
    # use_cache without a cache: still the stateless packed path, no cache returned
    with torch.no_grad():
        out = mb.model(inputs_embeds=x.bfloat16(), cu_seqlens=cu, use_cache=True)
    assert out.past_key_values is None
