"""GPU (-m gpu): the wide decode step (B = 33 .. 128; csrc/decode_step_wide.hip through decode.WideDecodeStep).

1. Bit-identity to the 32-row kernel: a row's values depend only on its own MFMA column, and the K split, the head phase's pairing
   and every summation order are the 32-row kernel's, so the wide step on B rows must equal, bit for bit, one DecodeStep per
   32-aligned group of rows -- logits and all three state fields of every layer, after every step, with the pointers as kernel
   arguments and read from the device table.
2. The fp64 restatement of tests/ref_decode_step.py in one of its hard regimes at B = 64, with the bars its bars() computes: a wide
   kernel that merely agrees with a wrong narrow one does not pass.
3. Rows behind B (logits and state) are never written.
4. GraphDecoder at B = 64 gives the greedy ids of two 32-row GraphDecoders on the halves of the batch.
5. The three continuous-batching engines at 64 slots: a request's ids do not depend on its slot (below or above row 32) or on when it
   is admitted, and every handle returns once with slots reused."""
import dataclasses
import random

import pytest
import torch

import ref_decode_step as RD
from rwkvtts_amd import backbone
from rwkvtts_amd.backbone import Cache, LayerState, RWKV7Config, RWKV7ForCausalLM
from rwkvtts_amd.decode import DecodeStep, GraphDecoder, WideDecodeStep, step_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _model(D, L, V, ranks, seed=0, head_bias=False):
    cfg = RWKV7Config(hidden_size=D, num_hidden_layers=L, vocab_size=V, decay_low_rank_dim=ranks[0], a_low_rank_dim=ranks[1],
                      v_low_rank_dim=ranks[2], gate_low_rank_dim=ranks[3])
    torch.manual_seed(seed)
    m = RWKV7ForCausalLM(cfg, head_bias=head_bias)
    backbone.init_weights(m, cfg, seed=seed)
    with torch.no_grad():
        m.lm_head.weight.normal_(0, 0.05)
        if head_bias:
            m.lm_head.bias.normal_(0, 0.1)
        for blk in m.model.layers:   # non-trivial norms and biases
            for ln in (blk.attn_norm, blk.ffn_norm):
                ln.weight.add_(torch.randn_like(ln.weight) * 0.1)
                ln.bias.add_(torch.randn_like(ln.bias) * 0.1)
    return cfg, m.to(DEV).to(torch.bfloat16).eval()


def _fields(c):
    return [t for s in c.states for t in (s.att_x_prev, s.att_kv, s.ffn_x_prev)]


def _slice(c, a, b):
    """rows a..b of a cache as a cache of its own (copies)"""
    return Cache([LayerState(s.att_x_prev[a:b].clone(), s.att_kv[a:b].clone(), s.ffn_x_prev[a:b].clone()) for s in c.states], c.seen_tokens)


# ------------------------------------------------------------------------------------------------------------ 1. bit-identity
@pytest.mark.parametrize("D,L,V,ranks,B,bias", [
    (128, 2, 77, (32, 32, 32, 32), 33, True),         # one row in the second tile, and an odd pair
    (128, 2, 77, (32, 32, 32, 32), 40, False),        # partial second tile
    (128, 3, 64, (64, 32, 32, 96), 64, False),        # RT = 2, three layers
    (128, 2, 77, (32, 32, 32, 32), 96, False),        # RT = 3
    (256, 2, 200, (160, 32, 32, 64), 97, False),      # a rank above 128: the generic fragment-slot instantiation, one-row fourth tile
    (1024, 2, 8193, (64, 64, 32, 128), 128, False),   # 0.4B widths
    (2048, 2, 1025, (96, 96, 64, 256), 128, True),    # 1.5B widths
])
def test_wide_step_is_bit_identical_to_the_32_row_step_per_group(D, L, V, ranks, B, bias):
    cfg, m = _model(D, L, V, ranks, seed=D + B, head_bias=bias)
    g = torch.Generator().manual_seed(B)
    prompt = torch.randint(0, V, (B, 6), generator=g).to(DEV)
    wide_c = Cache.zeros(cfg, B, DEV, torch.bfloat16)
    with torch.no_grad():
        m(input_ids=prompt, past_key_values=wide_c, use_cache=True)
    tbl_c = _slice(wide_c, 0, B)                               # the device-table-only call runs on a copy
    cuts = [(a, min(a + 32, B)) for a in range(0, B, 32)]      # 32-aligned groups; the last holds B mod 32 rows
    groups = [_slice(wide_c, a, b) for a, b in cuts]
    assert WideDecodeStep.supported(m.model, m.lm_head, wide_c) is None
    wide = WideDecodeStep(m.model, m.lm_head, wide_c)
    wide_t = WideDecodeStep(m.model, m.lm_head, tbl_c, host_table=False)
    narrow = [DecodeStep(m.model, m.lm_head, c) for c in groups]
    assert isinstance(step_for(m.model, m.lm_head, wide_c), WideDecodeStep) and isinstance(step_for(m.model, m.lm_head, groups[0]), DecodeStep)
    emb = m.model.embeddings.weight
    ids = torch.randint(0, V, (B,), generator=g).to(DEV)
    for it in range(5):
        x = torch.nn.functional.embedding(ids, emb).contiguous()
        lw = wide(x)
        assert torch.isfinite(lw).all()
        assert torch.equal(wide_t(x), lw), it                  # pointers as kernel arguments or fetched from the device table
        for (a, b), step in zip(cuts, narrow):
            ln = step(x[a:b].contiguous())
            assert torch.equal(lw[a:b], ln), (it, a, (lw[a:b] - ln).abs().max().item())
        for (a, b), c in zip(cuts, groups):
            for l, (sw, sn) in enumerate(zip(wide_c.states, c.states)):
                assert torch.equal(sw.att_x_prev[a:b], sn.att_x_prev), (it, a, l)
                assert torch.equal(sw.att_kv[a:b], sn.att_kv), (it, a, l)
                assert torch.equal(sw.ffn_x_prev[a:b], sn.ffn_x_prev), (it, a, l)
        for tw, tt in zip(_fields(wide_c), _fields(tbl_c)):
            assert torch.equal(tw, tt), it
        ids = lw.argmax(-1)


# ------------------------------------------------------------------------------------------------------------ 2. fp64 restatement
WIDE_CASE = dataclasses.replace(next(c for c in RD.CASES if c.regime == "mixed_decay" and c.B == 32), B=64)


def test_wide_step_against_fp64_reference():
    """tests/test_decode_step_parity_gpu.py's comparison for ref_decode_step's `mixed_decay` case with B = 64 instead of 32: two
    consecutive steps, each against the reference started from the state the kernel had before it; bar = 2 e_round + floor on every
    element of every observable, as ref_decode_step.bars computes it for this case."""
    case = WIDE_CASE
    p, states, ids = RD.make_case(case)
    cfg = RWKV7Config(hidden_size=case.D, num_hidden_layers=case.L, vocab_size=case.V, decay_low_rank_dim=case.ranks[0],
                      a_low_rank_dim=case.ranks[1], v_low_rank_dim=case.ranks[2], gate_low_rank_dim=case.ranks[3], intermediate_size=case.F)
    model = RWKV7ForCausalLM(cfg, head_bias=case.bias)
    model.load_state_dict(p, strict=True)
    model = model.to(DEV).to(torch.bfloat16).eval()
    emb = p["model.embeddings.weight"]
    p64 = {k: v.double() for k, v in p.items()}
    cache = Cache.zeros(cfg, case.B, DEV, torch.bfloat16)
    for i, s in enumerate(cache.states):
        s.att_x_prev.copy_(states[3 * i].to(torch.bfloat16))
        s.att_kv.copy_(states[3 * i + 1])
        s.ffn_x_prev.copy_(states[3 * i + 2].to(torch.bfloat16))
    step = WideDecodeStep(model.model, model.lm_head, cache)
    read = lambda: [t.float().cpu() if t.dtype == torch.bfloat16 else t.cpu().clone() for t in _fields(cache)]
    x_in = emb[ids]
    failures, worst = [], {}
    for it in range(2):
        before = read()
        logits = step(x_in.to(DEV).to(torch.bfloat16).contiguous()).double().cpu()
        after = read()
        exact = RD.ref_step(p64, before, x_in, case, rounded=False)
        rnd = RD.ref_step(p64, before, x_in, case, rounded=True)
        bars = RD.bars(exact, rnd, before, case)
        hip = {("logits", None): logits}
        for l in range(case.L):
            hip[("att_x_prev", l)], hip[("att_kv", l)], hip[("ffn_x_prev", l)] = (t.double() for t in after[3 * l:3 * l + 3])
        for name, l, xe in RD.observables(exact, case):
            xh, b = hip[(name, l)], bars[(name, l)]
            assert xh.shape == xe.shape and torch.isfinite(xh).all(), (it, name, l)
            err, idx = RD.worst(xh, xe)
            worst[name] = max(worst.get(name, 0.0), err / b["bar"])
            if err > b["bar"]:
                failures.append(f"step {it} layer {l} {name} at {idx}: error {err:.4g} > bar {b['bar']:.4g}")
        x_in = emb[exact["logits"].argmax(-1)]
    for name, r in worst.items():
        print(f"RATIO {case.id} {name} {r:.3f}")
    assert not failures, "\n".join(failures[:12])


# ------------------------------------------------------------------------------------------------------------ 3. rows outside B
def test_rows_behind_the_batch_are_never_written():
    D, L, V, B, PAD = 128, 2, 77, 40, 8
    cfg, m = _model(D, L, V, (32, 32, 32, 32), seed=3)
    g = torch.Generator().manual_seed(1)
    H = cfg.num_heads
    full = [((torch.randn(B + PAD, D, generator=g) * 0.5).to(DEV, torch.bfloat16), (torch.randn(B + PAD, H, 64, 64, generator=g) * 0.3).to(DEV),
             (torch.randn(B + PAD, D, generator=g) * 0.5).to(DEV, torch.bfloat16)) for _ in range(L)]
    canary = [[t[B:].clone() for t in layer] for layer in full]
    cache = Cache([LayerState(*(t[:B] for t in layer)) for layer in full])      # the first B rows of larger tensors, in place
    assert all(t.is_contiguous() for t in _fields(cache))
    step = WideDecodeStep(m.model, m.lm_head, cache)
    big_logits = torch.full((B + PAD, V), -123.0, device=DEV)
    step.logits = big_logits[:B]
    before = [t.clone() for t in _fields(cache)]
    x = (torch.randn(B, D, generator=g) * 0.5).to(DEV, torch.bfloat16)
    for _ in range(2):
        out = step(x)
    torch.cuda.synchronize()
    assert out.data_ptr() == big_logits.data_ptr() and torch.isfinite(out).all()
    assert (big_logits[B:] == -123.0).all()
    for layer, can in zip(full, canary):
        for t, c in zip(layer, can):
            assert torch.equal(t[B:], c)
    assert all(not torch.equal(a, b) for a, b in zip(_fields(cache), before))   # ... and the rows of the batch were


# ------------------------------------------------------------------------------------------------------------ 4. GraphDecoder
def test_graph_decoder_64_rows_equals_two_32_row_decoders():
    """The prefill is the only part the two shapes do not share (its GEMMs see 64 or 32 rows), so it is made identical by running it
    ONCE, at B = 64: each 32-row decoder is prepared on its half of the prompts (prefill, first id, captured step), and then its live
    cache rows, first ids and next input rows are overwritten with the 64-row decoder's rows before any step is replayed.  From there
    on both run the same captured loop: step kernel, greedy pick, embedding of the id."""
    D, L, V, B, P, NEW = 128, 2, 200, 64, 7, 12
    cfg, m16 = _model(D, L, V, (32, 32, 32, 64), seed=21)
    prompt = torch.randint(0, V, (B, P), generator=torch.Generator().manual_seed(4)).to(DEV)
    big = GraphDecoder(m16, B, step_kernel=True).prepare(input_ids=prompt, max_new_tokens=NEW)
    assert isinstance(big.step, WideDecodeStep)
    halves = []
    for a in (0, 32):
        d = GraphDecoder(m16, 32, step_kernel=True).prepare(input_ids=prompt[a:a + 32], max_new_tokens=NEW)
        assert type(d.step) is DecodeStep and (d.tail is None) == (big.tail is None)
        for sd, sb in zip(d.cache.states, big.cache.states):
            sd.att_x_prev.copy_(sb.att_x_prev[a:a + 32])
            sd.att_kv.copy_(sb.att_kv[a:a + 32])
            sd.ffn_x_prev.copy_(sb.ffn_x_prev[a:a + 32])
        d.ids.copy_(big.ids[a:a + 32])
        d.out[:, 0] = big.out[a:a + 32, 0]
        if d.tail is not None:
            d.x_next.copy_(big.x_next[a:a + 32])
        halves.append(d)
    for d in [big] + halves:
        for _ in range(d.steps_left):
            d.graph.replay()
    got = big.finish()
    want = torch.cat([d.finish() for d in halves], 0)
    assert got.shape == (B, NEW)
    for r in range(B):
        assert torch.equal(got[r], want[r]), (r, got[r], want[r])
    assert len({tuple(r) for r in got.tolist()}) > B // 2      # the rows are not all alike


# ------------------------------------------------------------------------------------------------------------ 5. engines, 64 slots
def _twins_at_64_slots(eng, submit_filler, submit_twin):
    """43 requests through 64 slots.  41 are admitted at once: fillers into slots 0..40 except 3 and 40, which take the same request
    (the twins); the filler in slot 35 has a budget of 4.  After the first step() slot 35 has retired, and the same request once more
    is admitted by the next step() into it, the lowest free slot, while every other request is still running.  -> the twins' results [slot 3, slot 40, slot 35 admitted late], after
    checking that every handle returned once."""
    handles, twins = [], []
    for i in range(41):
        if i in (3, 40):
            twins.append(submit_twin())
            handles.append(twins[-1])
        else:
            handles.append(submit_filler(i, 4 if i == 35 else 40))
    out = {}

    def step():
        for h, r in eng.step():
            assert h not in out
            out[h] = r

    step()
    slot_of = lambda h: [s for s, r in eng.sched.busy.items() if r.handle == h]
    assert slot_of(twins[0]) == [3] and slot_of(twins[1]) == [40]
    assert sorted(out) == [handles[35]] and eng.sched.free[0] == 35
    twins.append(submit_twin())
    handles.append(twins[-1])
    handles.append(submit_filler(99, 40))
    step()
    assert slot_of(twins[2]) == [35] and slot_of(handles[-1]) == [41]      # a retired slot >= 32, admitted later
    while not eng.sched.idle:
        step()
    assert sorted(out) == sorted(handles) and eng.sched.free == list(range(64))
    return [out[h] for h in twins]


def test_continuous_decoder_64_slots():
    from rwkvtts_amd.continuous import ContinuousDecoder
    from rwkvtts_amd.spark_llm import RWKV7ForSpeech, RWKV7SpeechConfig
    cfg = RWKV7SpeechConfig(vocab_size=300, text_vocab_size=300, audio_global_vocab_size=64, hidden_size=128, num_hidden_layers=2,
                            decay_low_rank_dim=32, a_low_rank_dim=32, v_low_rank_dim=32, gate_low_rank_dim=64)
    m = RWKV7ForSpeech(cfg).init_weights(0)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        m.lm_head.weight.copy_(torch.randn(m.lm_head.weight.shape, generator=g) * 0.05)
        m.model.embeddings.weight.copy_(torch.randn(m.model.embeddings.weight.shape, generator=g) * 0.5)
    m = m.to(DEV).to(torch.bfloat16).eval()
    prompt = lambda: (torch.randn(int(torch.randint(3, 20, (1,), generator=g)), 128, generator=g) * 0.5).to(DEV, torch.bfloat16)
    eng = ContinuousDecoder(m, slots=64, max_new_tokens_cap=64)
    assert isinstance(eng.dstep, WideDecodeStep)
    twin = prompt()
    a, b, c = _twins_at_64_slots(
        eng, lambda i, n: eng.submit(inputs_embeds=prompt(), max_new_tokens=n, do_sample=True, seed=100 + i),
        lambda: eng.submit(inputs_embeds=twin, max_new_tokens=24, do_sample=True, top_k=50, temperature=0.9, seed=7))
    assert a.shape == (24,) and torch.equal(a, b) and torch.equal(a, c), (a, b, c)


def test_continuous_xy_decoder_64_slots():
    from rwkvtts_amd.continuous_xy import ContinuousXYDecoder
    from rwkvtts_amd.xy_llm import RWKV7XYConfig, RWKV7XYLM
    cfg = RWKV7XYConfig(vocab_size=300, speech_vocab_size=64, num_channels=4, text_shift_size=200, hidden_size=128, num_hidden_layers=2,
                        decay_low_rank_dim=32, a_low_rank_dim=32, v_low_rank_dim=32, gate_low_rank_dim=32)
    m = RWKV7XYLM(cfg).init_weights(seed=5)
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for h in m.heads:
            h.weight.copy_(torch.randn(h.weight.shape, generator=g) * 0.05)
            h.bias.copy_(torch.randn(h.bias.shape, generator=g) * 0.1)
        for e in m.embs:
            e.weight.copy_(torch.randn(e.weight.shape, generator=g) * 0.5)
    m.zero_embs()
    m = m.to(DEV).to(torch.bfloat16).eval()

    def prompt():
        t = int(torch.randint(3, 20, (1,), generator=g))
        return torch.cat([torch.randint(0, 264, (t, 1), generator=g), torch.randint(0, 63, (t, 3), generator=g)], 1).to(DEV)

    eng = ContinuousXYDecoder(m, slots=64, max_new_frames_cap=64)
    assert isinstance(eng.dstep, WideDecodeStep)
    twin = prompt()
    a, b, c = _twins_at_64_slots(
        eng, lambda i, n: eng.submit(prompt(), max_new_frames=n, do_sample=True, seed=100 + i),
        lambda: eng.submit(twin, max_new_frames=24, do_sample=True, top_k=50, temperature=0.9, seed=7))
    assert a.shape == (24, 4) and torch.equal(a, b) and torch.equal(a, c), (a, b, c)


def test_continuous_cosy_decoder_64_slots():
    from rwkvtts_amd.continuous_cosy import ContinuousCosyDecoder, cosy_request
    from rwkvtts_amd.cosy_llm import RWKV7CosyConfig, RWKV7CosyLM
    m = RWKV7CosyLM(RWKV7CosyConfig(vocab_size=300, speech_token_size=96, hidden_size=128, num_hidden_layers=2, decay_low_rank_dim=32,
                                    a_low_rank_dim=32, v_low_rank_dim=32, gate_low_rank_dim=32)).init_weights(seed=5)
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        m.lm_head.weight.copy_(torch.randn(m.lm_head.weight.shape, generator=g) * 0.05)
        m.lm_head.bias.copy_(torch.randn(m.lm_head.bias.shape, generator=g) * 0.1)
        for e in (m.llm_embedding, m.text_embedding, m.speech_embedding):
            e.weight.copy_(torch.randn(e.weight.shape, generator=g) * 0.5)
    m = m.to(DEV).to(torch.bfloat16).eval()
    rng = random.Random(2)

    def prompt():
        text = torch.randint(0, 300, (rng.randint(3, 16),), generator=g)
        speech = torch.randint(0, 96, (rng.randint(0, 8),), generator=g)
        return cosy_request(m, text, None, speech).embeds

    eng = ContinuousCosyDecoder(m, slots=64, max_len_cap=64)
    assert isinstance(eng.dstep, WideDecodeStep)
    twin = prompt()
    # EOS is barred up to min_len: a filler runs exactly to its limit, and a twin holds its slot for at least 20 steps
    a, b, c = _twins_at_64_slots(
        eng, lambda i, n: eng.submit(inputs_embeds=prompt(), min_len=n, max_len=n, original_text_len=0, seed=100 + i),
        lambda: eng.submit(inputs_embeds=twin, min_len=20, max_len=30, original_text_len=0, sampling=25, seed=7))
    assert 20 <= a.numel() <= 30 and torch.equal(a, b) and torch.equal(a, c), (a, b, c)
