"""GPU (-m gpu): preference (DPO) training on the HIP route -- rwkv7_ce_seq_bwd_bf16 alone,
losses.fused_linear_seq_logprob, the heads' sequence_logprobs on the real backbone, DataParallelTrainer.preference_step.

Kernel: NO tolerance.  With scales c_s the gradient of every row of sequence s, and loss_rows of every row, equal bit for bit what
rwkv7_ce_fwd_bwd_ld_bf16 writes for the same logits (at the same address modulo 16 bytes) with the uniform scale c_s and smoothing 0.
Forward: bit for bit -fused_linear_score's loss_sum, for every chunk size.
Gradients: MEASURED against a yardstick, not a fixed number.  The reference is test_preference.seq_logprob_fp64 (plain autograd in
fp64) fed the same bf16 hidden / weight / bias; the yardstick is the relative L2 error of the existing fused_linear_cross_entropy HIP
path against its own fp64 restatement on the same inputs, computed in the same test; the bar is 2 x that yardstick: the bf16 logits
and the bf16 rounding of the gradient are the same, the scale now precedes that rounding instead of following it (which can only
help), and the factor 2 covers the other order of dW's fp32 accumulation across chunks.  Every comparison prints
`PARITY <case> <observable> <error> <yardstick>`; the record of one run is profiles/preference_head_parity.txt.
Heads: bit for bit their own score, with autograd on as well (the backbone runs as score runs it and is recomputed with autograd in
backward), and on the hidden states of the very pass that formed the value."""
import pytest
import torch
import torch.nn.functional as F

from rwkvtts_amd import _lib, layouts as L, losses, trainer
from rwkvtts_amd.cosy_llm import RWKV7CosyConfig, RWKV7CosyLM
from rwkvtts_amd.spark_llm import RWKV7ForSpeech, RWKV7SpeechConfig
from test_preference import seq_logprob_fp64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IGN = -100
SENTINEL = 0x7b7b   # bf16 bits of the columns V .. ld - 1


# ---- the kernel alone --------------------------------------------------------------------------------------------------------------
ROWS = 67                          # 17 workgroups of four rows, the last one with three
OFFSETS = [5, 6, 6, 22, 41, 60]    # relative to row0: rows 0-4 in front; one row; an empty range; 22 falls inside the workgroup of rows
SCALES = [3.0, 7.0, 0.0, -0.5, 1e-4]   # 20-23; rows 60-66 behind.  7.0 belongs to the empty sequence: no row may take it


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("row0", [0, 1000])
@pytest.mark.parametrize("V,ld", [(8193, 8193), (8193, 8448), (6562, 6568), (1025, 1032), (5, 8)])
def test_kernel_equals_the_uniform_scale_kernel_row_by_row(hip_lib, V, ld, row0):
    g = torch.Generator().manual_seed(V + ld + row0)
    x = torch.full((ROWS, ld), 0.0, dtype=torch.bfloat16)
    x[:, :V] = (torch.randn(ROWS, V, generator=g) * 3).bfloat16()
    _bits(x)[:, V:] = SENTINEL
    lab = torch.randint(0, V, (ROWS,), generator=g)
    lab[[2, 7, 23, 40, 59, 63]] = IGN
    x, lab = x.to(DEV), lab.to(DEV)
    st = (torch.tensor(OFFSETS) + row0).to(DEV)
    scales = torch.tensor(SCALES, dtype=torch.float32, device=DEV)
    got, loss = x.clone(), torch.full((ROWS + 2,), -77.0, device=DEV)
    _lib.call("rwkv7_ce_seq_bwd_bf16", got, ROWS, V, ld, got, lab, IGN, row0, len(SCALES), st, scales, loss[1:])
    torch.cuda.synchronize()
    assert loss[0] == -77 and loss[-1] == -77, "loss_rows written outside [0, rows)"
    assert torch.equal(_bits(got)[:, V:], _bits(x)[:, V:]), "columns V .. ld - 1 must stay untouched"
    seq_of = torch.full((ROWS,), -1)
    for s in range(len(SCALES)):
        seq_of[OFFSETS[s]:OFFSETS[s + 1]] = s
    assert (seq_of == 1).sum() == 0 and (seq_of == 0).sum() == 1 and seq_of[21] != seq_of[22]
    for s, c in enumerate(SCALES):
        want, want_loss = x.clone(), torch.empty(ROWS, device=DEV)   # a clone: the same address modulo 16 bytes, row by row
        assert want.data_ptr() % 16 == got.data_ptr() % 16
        _lib.call("rwkv7_ce_fwd_bwd_ld_bf16", want, ROWS, V, ld, want, lab, IGN, c, want_loss, 0.0)
        assert torch.equal(loss[1:-1].view(torch.int32), want_loss.view(torch.int32)), "loss_rows"
        rows = (seq_of == s).nonzero().squeeze(1).to(DEV)
        assert torch.equal(_bits(got)[rows, :V], _bits(want)[rows, :V]), f"sequence {s}, scale {c}"
    outside = ((seq_of == -1) | (lab.cpu() == IGN) | (seq_of == 2)).nonzero().squeeze(1).to(DEV)   # sequence 2: the zero scale
    assert outside.numel() >= 5 + 7 + 6 and bool((got[outside, :V] == 0).all()), "out-of-range and ignored rows are zeros"
    live = ((seq_of == 3) & (lab.cpu() != IGN)).nonzero().squeeze(1).to(DEV)
    assert bool((got[live, :V] != 0).any(dim=1).all())
    again = x.clone()   # loss_rows may be NULL
    _lib.call("rwkv7_ce_seq_bwd_bf16", again, ROWS, V, ld, again, lab, IGN, row0, len(SCALES), st, scales, None)
    assert torch.equal(_bits(again), _bits(got))


# ---- fused_linear_seq_logprob on the HIP route ---------------------------------------------------------------------------------------
N, D = 200, 256
SEQ_START = [0, 50, 50, 70, 140, 200]   # sequences across the chunk boundaries 64 and 128 (and 72, where the last chunk of 128 starts)


def _head(V, bias, seed=0):
    g = torch.Generator().manual_seed(V + seed)
    h = torch.randn(N, D, generator=g).bfloat16().to(DEV)
    w = (torch.randn(V, D, generator=g) * 0.1).bfloat16().to(DEV)
    b = (torch.randn(V, generator=g) * 0.1).bfloat16().to(DEV) if bias else None
    lab = torch.randint(0, V, (N,), generator=g)
    lab[torch.rand(N, generator=g) < 0.1] = IGN
    up = torch.rand(len(SEQ_START) - 1, generator=g, dtype=torch.float64) * 2 - 1   # the upstream gradient, in [-1, 1]
    return h, w, b, lab.to(DEV), torch.tensor(SEQ_START, device=DEV), up.to(DEV)


def _grads(h, w, b, lab, st, up, chunk):
    leaves = [t.detach().clone().requires_grad_() for t in (h, w, b) if t is not None]
    logp = losses.fused_linear_seq_logprob(leaves[0], lab, leaves[1], leaves[2] if b is not None else None, IGN, seq_start=st, chunk=chunk)
    (logp * up).sum().backward()
    return logp.detach(), [t.grad for t in leaves]


@pytest.mark.parametrize("V", [1025, 8193])
def test_forward_is_the_negated_score_for_every_chunk_size(hip_lib, V):
    h, w, b, lab, st, up = _head(V, bias=V == 1025)
    for chunk, launches in ((64, 4), (128, 2), (N, 1)):   # 64: 0, 64, 128 and the last 64 rows; 128: 0 and the last 128 rows
        want = losses.fused_linear_score(h, lab, w, b, IGN, losses.EVAL_CE, seq_start=st, chunk=chunk)[0]
        hits = losses.SEQLP_HITS[0]
        logp, grads = _grads(h, w, b, lab, st, up, chunk)
        assert losses.SEQLP_HITS[0] == hits + launches, "the HIP route: one rwkv7_ce_seq_bwd_bf16 launch per chunk"
        assert logp.dtype == torch.float64 and torch.equal(logp.view(torch.int64), (-want).view(torch.int64)), chunk
        assert logp[1] == 0 and all(bool(torch.isfinite(g_).all()) for g_ in grads)
        assert grads[0].dtype == grads[1].dtype == torch.bfloat16 and grads[0].shape == h.shape and grads[1].shape == w.shape


def _rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def _fp64_grads(fn, h, w, b):
    leaves = [t.detach().double().requires_grad_() for t in (h, w, b) if t is not None]
    fn(leaves[0], leaves[1], leaves[2] if b is not None else None).backward()
    return [t.grad for t in leaves]


def _yardstick(h, w, b, lab):
    """Relative L2 errors (dh, dW, db) of the existing fused_linear_cross_entropy HIP path against its fp64 restatement."""
    leaves = [t.detach().clone().requires_grad_() for t in (h, w, b)]
    losses.fused_linear_cross_entropy(leaves[0], lab, leaves[1], leaves[2], IGN, chunk=N).backward()
    want = _fp64_grads(lambda h_, w_, b_: F.cross_entropy(F.linear(h_, w_, b_), lab, ignore_index=IGN), h, w, b)
    return [_rel_l2(t.grad, r) for t, r in zip(leaves, want)]


@pytest.fixture(scope="module")
def parity(hip_lib):
    """One head with bias (so that db exists), its yardstick, the fp64 reference and the new path's gradients at three chunk sizes."""
    h, w, b, lab, st, up = _head(1025, bias=True, seed=1)
    want = _fp64_grads(lambda h_, w_, b_: (seq_logprob_fp64(h_, w_, b_, lab, st, IGN) * up).sum(), h, w, b)
    return dict(case=(h, w, b, lab, st, up), yard=_yardstick(h, w, b, lab), want=want,
                got={c: _grads(h, w, b, lab, st, up, c)[1] for c in (64, 128, N)})


def test_gradients_within_twice_the_cross_entropy_paths_own_error(parity):
    for chunk, got in parity["got"].items():
        for name, g_, r, yard in zip(("dh", "dW", "db"), got, parity["want"], parity["yard"]):
            err = _rel_l2(g_, r)
            print(f"PARITY chunk={chunk} {name} {err:.3e} {yard:.3e}")
            assert 0 < err <= 2 * yard, (chunk, name, err, yard)


def test_an_overlapping_last_chunk_is_not_counted_twice(parity):
    """N = 200, chunk = 128: the last chunk is rows 72 .. 199 and overlaps 56 rows of the first."""
    h, w, b, lab, st, up = parity["case"]
    one, two = parity["got"][N], parity["got"][128]
    # the overlapped rows' contribution, restated in torch from the bf16 logits
    rows = slice(72, 128)
    x = F.linear(h[rows], w, b).float()
    p = torch.softmax(x, dim=1)
    p.scatter_add_(1, lab[rows].clamp(min=0).unsqueeze(1), torch.full_like(p[:, :1], -1.0))
    scale = losses._row_scales(st, (-up).float(), 72, 56) * (lab[rows] != IGN)
    pd = (p * scale.unsqueeze(1)).bfloat16()
    extra = dict(dW=(pd.t() @ h[rows]).float(), db=pd.float().sum(0))
    for name, i in (("dW", 1), ("db", 2)):
        bar = 2 * parity["yard"][i]
        same, doubled = _rel_l2(two[i], one[i]), _rel_l2(two[i], one[i].float() + extra[name])
        print(f"PARITY overlap {name} {same:.3e} {parity['yard'][i]:.3e} double-counted {doubled:.3e}")
        assert same <= bar, (name, same, bar)
        assert doubled > 10 * bar, (name, doubled, bar)
    assert _rel_l2(two[0], one[0]) <= 2 * parity["yard"][0]   # dh: every row written once, by the chunk that owns it


# ---- the heads on the real backbone ------------------------------------------------------------------------------------------------
MID = dict(hidden_size=256, num_hidden_layers=2, decay_low_rank_dim=32, a_low_rank_dim=32, v_low_rank_dim=16, gate_low_rank_dim=32)


def _spark(vocab=257, seed=3):
    cfg = RWKV7SpeechConfig(vocab_size=vocab, text_vocab_size=300, audio_global_vocab_size=64, **MID)
    return RWKV7ForSpeech(cfg).init_weights(seed=seed).to(DEV).to(torch.bfloat16)


def _grad_names(m, loss):
    """Backward of `loss`; the names of the parameters that received a gradient, every one of them finite."""
    m.zero_grad(set_to_none=True)
    loss.backward()
    got = {k for k, p in m.named_parameters() if p.grad is not None}
    assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters() if p.grad is not None)
    return got


def _spark_padded():
    m = _spark().eval()

    def batch():   # a fresh graph into the embedders at every call
        bt = L.synthetic_spark_batch(m, 4, 64, seed=5, n_text=9, n_global=4)
        for b_, keep in enumerate((48, 30, 17, 5)):   # utterances of different lengths
            bt["labels"][b_, 64 - 48 + keep:] = -100
        return bt
    return m, batch, [48, 30, 17, 5]


def _spark_packed():
    m = _spark().eval()
    g = torch.Generator().manual_seed(6)
    cu = torch.tensor([0, 20, 33, 33, 61, 64])   # five utterances, one empty: four of different lengths and the empty one
    labels = torch.randint(0, 256, (1, 64), generator=g)
    labels[0, cu[1:] - 1] = -100
    emb = (torch.randn(1, 64, 256, generator=g) * 0.5).bfloat16().to(DEV)
    shifted = torch.cat((labels[0, 1:], torch.tensor([-100])))
    tokens = [int((shifted[a:b] != -100).sum()) for a, b in zip(cu[:-1].tolist(), cu[1:].tolist())]
    return m, lambda: dict(inputs_embeds=emb, labels=labels.to(DEV), cu_seqlens=cu.to(DEV)), tokens


def _cosy():
    cfg = RWKV7CosyConfig(vocab_size=200, speech_token_size=50, lsm_weight=0.0, length_normalized_loss=True, **MID)
    llm = RWKV7CosyLM(cfg).init_weights(seed=4).to(torch.bfloat16).to(DEV).eval()
    text = [[3, 4, 5, 6], [7, 8], [9, 10, 11], [12]]
    speech = [list(range(10, 40)), [20, 21, 22], list(range(5, 20)), list(range(1, 9))]
    bt = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in L.cosy_collate(text, speech, pad_to_max_length=False).items()}
    return llm, lambda: dict(batch=bt), [31, 4, 16, 9]


HEADS = dict(spark_padded=_spark_padded, spark_packed=_spark_packed, cosy=_cosy)


def _grad_names(m, loss):
    """Backward of `loss`; the names of the parameters that received a gradient, every one of them finite."""
    m.zero_grad(set_to_none=True)
    loss.backward()
    got = {k for k, p in m.named_parameters() if p.grad is not None}
    assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters() if p.grad is not None)
    return got


class _Replay(torch.nn.Module):
    """Stands in for the backbone: returns the hidden states a pass has produced."""

    def __init__(self, hidden):
        super().__init__()
        self.hidden = hidden

    def forward(self, *args, **kwargs):
        return (self.hidden,)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


@pytest.mark.parametrize("head", list(HEADS))
def test_sequence_logprobs_on_the_real_backbone(hip_lib, head):
    """tokens are score's and logp is bit for bit -loss_sum, under no_grad and with autograd on; the value is -fused_linear_score of
    the hidden states the forward pass produced.  Backward launches the kernel once (one chunk) and fills, with finite values, the
    gradient of every parameter the head's own training loss on the same batch reaches (on the real backbone a few parameters take
    part in no forward pass, and the embedders in none when the batch brings inputs_embeds as data)."""
    m, batch, tokens = HEADS[head]()
    n = len(tokens)
    score = m.score(**batch())
    with torch.no_grad():
        quiet = m.sequence_logprobs(**batch())
    assert quiet["tokens"].tolist() == tokens and torch.equal(quiet["tokens"], score["tokens"])
    assert quiet["logp"].dtype == torch.float64 and quiet["logp"].shape == (n,) and _same_bits(quiet["logp"], -score["loss_sum"])
    trained = _grad_names(m, m(**batch()).loss)
    seen = []
    hook = m.model.register_forward_hook(lambda mod, args, out: seen.append(out[0].detach()))
    seq = m.sequence_logprobs(**batch())
    hook.remove()
    assert torch.equal(seq["tokens"], score["tokens"]) and seq["logp"].requires_grad and len(seen) == 1
    again = batch()
    backbone, m.model = m.model, _Replay(seen[0])   # score of exactly those hidden states
    own = m.score(**again)
    m.model = backbone
    assert _same_bits(seq["logp"].detach(), -own["loss_sum"])
    hits = losses.SEQLP_HITS[0]
    got = _grad_names(m, (seq["logp"] * torch.linspace(-1, 1, n, dtype=torch.float64, device=DEV)).sum())
    assert losses.SEQLP_HITS[0] == hits + 1, "one chunk: one rwkv7_ce_seq_bwd_bf16 launch"
    assert got == trained and len(got) > 20 and any("lm_head" in k for k in got), sorted(trained ^ got)


@pytest.mark.parametrize("head", list(HEADS))
def test_logp_with_autograd_on_equals_score_bit_for_bit(hip_lib, head):
    """Eval mode, autograd ON: logp == -score's loss_sum bit for bit.  The backbone chooses other kernels (its fused training nodes)
    when autograd is on than under no_grad, which score uses, and their bf16 hidden states differ in the last bits (measured on
    MI355X when sequence_logprobs still ran the backbone on the tape: up to 3.2e-05 relative for the padded Spark case, 5.9e-05 for
    Cosy, 0 for packed rows).  sequence_logprobs therefore runs the backbone as score does and recomputes it with autograd in
    backward (losses.scored_forward); the gradients must still arrive."""
    m, batch, _ = HEADS[head]()
    score, seq = m.score(**batch()), m.sequence_logprobs(**batch())
    rel = ((seq["logp"].detach() + score["loss_sum"]).abs() / score["loss_sum"].abs().clamp(min=1e-30)).max().item()
    print(f"PARITY {head} logp (autograd on) against -score loss_sum: max relative difference {rel:.3e}")
    assert torch.equal(seq["tokens"], score["tokens"])
    assert _same_bits(seq["logp"].detach(), -score["loss_sum"]), rel
    assert "lm_head.weight" in _grad_names(m, seq["logp"].sum()) and m.model.layers[0].attn.o_proj.weight.grad is not None


# ---- DataParallelTrainer.preference_step on the HIP AdamW path -----------------------------------------------------------------------
KW = dict(lr=1e-4, warmup_steps=0, total_steps=100)
BETA = 0.1


def _pairs(m, P, T, seed):
    batch = L.synthetic_spark_batch(m, 2 * P, T, seed=seed, n_text=31, n_global=8)
    batch["inputs_embeds"] = batch["inputs_embeds"].detach()   # the batch is used for several steps: no graph into the embedders
    return batch


@pytest.mark.timeout(120)
def test_preference_step_on_the_hip_path(hip_lib):
    torch.manual_seed(11)
    m = _spark(vocab=8193).train()
    tr = trainer.DataParallelTrainer(m, max_grad_norm=1.0, **KW)
    assert tr.hip_adamw
    batch = _pairs(m, 4, 512, seed=21)   # 4 pairs, N = 8 x 512 = 4096 rows, V = 8193
    ref = -torch.from_numpy(tr.score([batch])["loss_sum"])   # the frozen reference: the policy before tuning
    hits = losses.SEQLP_HITS[0]
    outs, norms = [], []
    for _ in range(5):
        outs.append(tr.preference_step(beta=BETA, ref_logps=ref, **batch))
        norms.append(tr.last_grad_norm.item())
    assert losses.SEQLP_HITS[0] == hits + 5 and tr.step_idx == 5
    margins = [o["margin"].item() for o in outs]
    assert all(o["loss"].is_cuda and o["logp_chosen"].shape == (4,) for o in outs)
    assert margins[-1] > margins[0], margins
    assert all(bool(torch.isfinite(o["loss"])) and 0 <= o["accuracy"].item() <= 1 for o in outs)
    # the first step's norm: once the pairs are separated softplus saturates and the bf16 gradient may underflow to an exact zero
    assert all(n == n and n != float("inf") for n in norms) and norms[0] > 0, norms
    # a NaN among the reference values: step()'s zero-gradient step -- the state a step() on a NaN loss leaves behind
    twin = trainer.DataParallelTrainer(_spark(vocab=8193).train(), max_grad_norm=1.0, **KW)
    for name in ("master", "exp_avg", "exp_avg_sq"):
        getattr(twin, name).copy_(getattr(tr, name))
    twin.flat.flat_param.copy_(tr.flat.flat_param)
    twin.step_idx = tr.step_idx
    bad = ref.clone()
    bad[3] = float("nan")
    tr.preference_step(beta=BETA, ref_logps=bad, **batch)
    poisoned = dict(batch, inputs_embeds=batch["inputs_embeds"].clone())
    poisoned["inputs_embeds"][0, 5, 7] = float("nan")
    twin.step(**poisoned)
    torch.cuda.synchronize()
    assert tr.nan_flag.item() == 1 and tr.step_idx == 6
    for name in ("master", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(tr, name), getattr(twin, name)), name
    assert torch.equal(tr.flat.flat_param, twin.flat.flat_param) and bool(torch.isfinite(tr.master).all())


def test_fresh_trainer_nan_reference_moves_nothing(hip_lib):
    m = _spark().train()
    tr = trainer.DataParallelTrainer(m, **KW)
    batch = _pairs(m, 2, 64, seed=22)
    before = [t.clone() for t in (tr.master, tr.exp_avg, tr.exp_avg_sq, tr.flat.flat_param)]
    tr.preference_step(beta=BETA, ref_logps=torch.tensor([0.0, float("nan"), 0.0, 0.0]), **batch)
    torch.cuda.synchronize()
    assert tr.nan_flag.item() == 1 and tr.step_idx == 1
    assert all(torch.equal(a, b) for a, b in zip(before, (tr.master, tr.exp_avg, tr.exp_avg_sq, tr.flat.flat_param)))


def test_peak_memory_stays_below_the_materialised_logits_route(hip_lib):
    """N = 4096 rows, V = 8193: the peak of sequence_logprobs + backward against the eval-mode forward(labels=...) route (logits,
    fp32 log_softmax, gather) on the same batch.  Both measured here; the condition is the point of the feature."""
    m = _spark(vocab=8193).eval()
    batch = _pairs(m, 4, 512, seed=23)
    up = torch.linspace(-1, 1, 8, dtype=torch.float64, device=DEV)

    def fused():
        (m.sequence_logprobs(**batch)["logp"] * up).sum().backward()

    def materialised():
        out = m(**batch)
        lab = torch.cat((batch["labels"][:, 1:], torch.full_like(batch["labels"][:, :1], -100)), 1)
        lp = F.log_softmax(out.logits.float(), dim=-1).gather(2, lab.clamp(min=0).unsqueeze(2)).squeeze(2)
        ((lp * (lab != -100)).sum(1).double() * up).sum().backward()

    peaks = []
    for fn in (fused, materialised):
        fn()   # warm-up: workspaces and caches exist before the measured call
        m.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - base)
        m.zero_grad(set_to_none=True)
    print(f"PARITY memory fused {peaks[0] / 2 ** 20:.1f} MiB materialised {peaks[1] / 2 ** 20:.1f} MiB")
    assert peaks[0] < peaks[1], peaks
