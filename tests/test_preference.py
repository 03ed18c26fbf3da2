"""CPU: preference (DPO) training -- the C ABI of rwkv7_ce_seq_bwd_bf16, losses.fused_linear_seq_logprob on its torch route, the heads'
sequence_logprobs and DataParallelTrainer.preference_step.

What the values are compared against:
  * fused_linear_seq_logprob: plain autograd in fp64 (log_softmax -> gather -> masked segment sums) on the same numbers.  logp within
    1e-6 relative (fp32 logits and row losses, summed in fp64); dh / dW / db within 1e-5 relative L2 (fp32 rounding of softmax and
    of the three products).
  * the heads: their own score -- tokens equal, logp bit for bit -loss_sum in eval mode (the Cosy head where lsm_weight = 0: its
    score is the label-smoothing KL, which without smoothing is -log p).
  * preference_step: a hand-written DPO step (plain logits, log_softmax, the AdamW rule of the trainer's torch path) from the same
    initial state, parameters within 1e-5.  eps = 1e-3 instead of the trainer's default 1e-18: with the default the first AdamW
    update is lr * sign(g), which amplifies a rounding-sized difference of a near-zero gradient element to 2 lr; with eps = 1e-3 the
    update is lr g / (|g| + eps), Lipschitz in g with constant lr / eps = 10.
The heads run on test_head_eval's CPU stand-in for the backbone; the real one is in test_preference_gpu.py."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from rwkvtts_amd import _lib, losses, trainer
from rwkvtts_amd.cosy_llm import RWKV7CosyConfig, RWKV7CosyLM, RWKV7LM
from rwkvtts_amd.xy_llm import RWKV7XYLM
from test_head_eval import SMALL, _assert_same_state, _cosy_batch, _spark, _spark_batch, _state, _stubbed
from test_trainer_dist import _free_port

NAME = "rwkv7_ce_seq_bwd_bf16"
OPT = dict(lr=1e-2, warmup_steps=0, total_steps=100, eps=1e-3)
BETA = 0.5


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_and_the_library_exports_it(hip_lib):
    assert NAME in _lib.exported_symbols()
    restype, argtypes = _lib.prototypes()[NAME]
    P, L, I = ctypes.c_void_p, ctypes.c_long, ctypes.c_int
    # rows, V, ld, logits, labels, ignore_index, row0, n_seq, seq_start, seq_scale, loss_rows, the stream
    assert restype is I and argtypes == [L, I, L, P, P, L, L, L, P, P, P, P]
    fn = getattr(hip_lib, NAME)
    assert fn.restype is I and list(fn.argtypes) == argtypes


def test_entry_point_rejects_bad_arguments_before_any_launch(hip_lib):
    one = 16   # never dereferenced: the checks fire first
    names = ["logits", "labels", "seq_start", "seq_scale"]

    def call(rows=5, V=11, ld=16, row0=0, n_seq=2, **null):
        p = {n: (None if n in null else one) for n in names}
        return getattr(hip_lib, NAME)(rows, V, ld, p["logits"], p["labels"], -100, row0, n_seq, p["seq_start"], p["seq_scale"], None, None)

    for n in names:
        assert call(**{n: True}) == -1, n
    assert call(rows=0) == -1 and call(V=0) == -1 and call(ld=10) == -1 and call(row0=-1) == -1 and call(n_seq=0) == -1


# ---- fused_linear_seq_logprob, torch route -----------------------------------------------------------------------------------------
N, D = 37, 16
# rows 0-2 in front of seq_start[0]; an empty sequence; a one-row one; six rows; five ignored rows; fifteen rows; rows 30-36 behind
SEQ_START = [3, 3, 4, 10, 15, 30]
IGNORED_ONLY = 3


def _case(V, bias=True):
    g = torch.Generator().manual_seed(V)
    h = torch.randn(N, D, generator=g)
    w = torch.randn(V, D, generator=g) * 0.5
    b = torch.randn(V, generator=g) * 0.1 if bias else None
    lab = torch.randint(0, V, (N,), generator=g)
    lab[[1, 6, 20, 33]] = -100
    lab[SEQ_START[IGNORED_ONLY]:SEQ_START[IGNORED_ONLY + 1]] = -100
    up = torch.randn(len(SEQ_START) - 1, generator=g, dtype=torch.float64)
    up[1], up[2], up[4] = 0.7, 0.0, -1.3   # mixed signs and a zero on sequences that own rows
    return h, w, b, lab, torch.tensor(SEQ_START), up


def seq_logprob_fp64(h, w, b, lab, st, ignore=-100):
    """The definition in plain autograd, fp64: log_softmax of the logits, gathered at the label, masked, summed per sequence."""
    lp = F.log_softmax(F.linear(h.double(), w.double(), None if b is None else b.double()), dim=1)
    rows = lp.gather(1, lab.clamp(min=0).unsqueeze(1)).squeeze(1) * (lab != ignore)
    st = st.tolist()
    return torch.stack([rows[st[s]:st[s + 1]].sum() for s in range(len(st) - 1)])


def _rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


@pytest.mark.parametrize("V", [11, 257])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("chunk", [None, 8])
def test_torch_route_against_fp64_autograd(V, bias, chunk):
    h, w, b, lab, st, up = _case(V, bias)
    leaves = [t.clone().requires_grad_() for t in (h, w, b) if t is not None]
    hits = losses.SEQLP_HITS[0], losses.SCORE_HITS[0]
    got = losses.fused_linear_seq_logprob(leaves[0], lab, leaves[1], leaves[2] if bias else None, -100, seq_start=st, chunk=chunk)
    assert got.dtype == torch.float64 and got.shape == (5,) and got.requires_grad
    (got * up).sum().backward()
    assert (losses.SEQLP_HITS[0], losses.SCORE_HITS[0]) == hits, "CPU tensors must take the torch route"
    ref_leaves = [t.double().requires_grad_() for t in (h, w, b) if t is not None]
    want = seq_logprob_fp64(ref_leaves[0], ref_leaves[1], ref_leaves[2] if bias else None, lab, st)
    (want * up).sum().backward()
    assert want[0] == 0 and want[IGNORED_ONLY] == 0 and got[0] == 0 and got[IGNORED_ONLY] == 0
    assert bool(((got - want).abs() <= 1e-6 * want.abs()).all()), (got, want)
    for name, a, r in zip(("dh", "dW", "db"), leaves, ref_leaves):
        assert a.grad.dtype == a.dtype and a.grad.shape == a.shape
        assert _rel_l2(a.grad, r.grad) <= 1e-5, (name, _rel_l2(a.grad, r.grad))
    dh = leaves[0].grad
    outside = [0, 1, 2] + list(range(30, 37)) + [6, 20] + list(range(10, 15)) + [4, 5, 7, 8, 9]   # rows 4-9: the zero upstream
    assert bool((dh[outside] == 0).all()) and bool((dh[3] != 0).any()) and bool((dh[29] != 0).any())


def test_forward_is_the_negated_score_and_fp32_upstream_is_taken():
    h, w, b, lab, st, up = _case(257)
    got = losses.fused_linear_seq_logprob(h.requires_grad_(), lab, w, b, -100, seq_start=st, chunk=8)
    want = losses.fused_linear_score(h, lab, w, b, -100, losses.EVAL_CE, seq_start=st, chunk=8)
    assert torch.equal(got.detach(), -want[0])
    assert torch.equal(losses.seq_token_counts(lab, -100, st), want[1])
    got.backward(up.float())
    assert h.grad is not None and bool(torch.isfinite(h.grad).all())
    for bad in (None, torch.zeros(1, dtype=torch.int64), torch.zeros(2, 2, dtype=torch.int64)):
        with pytest.raises(ValueError):
            losses.fused_linear_seq_logprob(h, lab, w, b, -100, seq_start=bad)


# ---- the heads ---------------------------------------------------------------------------------------------------------------------
def _check_head(m, score, seq, n):
    assert set(seq) == {"logp", "tokens"} and seq["logp"].shape == seq["tokens"].shape == (n,)
    assert seq["logp"].dtype == torch.float64 and seq["tokens"].dtype == torch.int64 and seq["logp"].requires_grad
    assert torch.equal(seq["tokens"], score["tokens"])
    assert torch.equal(seq["logp"].detach(), -score["loss_sum"]), "eval mode: bit for bit the score's loss_sum"
    seq["logp"].sum().backward()
    got = [p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool((p.grad != 0).any()) for p in m.lm_head.parameters()]
    assert all(got), "the head's parameters must receive a gradient"


def test_spark_sequence_logprobs_padded():
    m = _spark().eval()
    batch = _spark_batch(3)
    _check_head(m, m.score(**batch), m.sequence_logprobs(**batch), 2)
    assert m.model.mix.weight.grad is not None, "the gradient must reach the backbone"
    m.train()
    torch.manual_seed(0)
    a = m.sequence_logprobs(**batch)["logp"]
    assert m.training and not torch.equal(a.detach(), -m.score(**batch)["loss_sum"]), "training mode: forward's dropout is live"


def test_spark_sequence_logprobs_packed_cu_seqlens():
    m = _spark().eval()
    g = torch.Generator().manual_seed(8)
    cu = torch.tensor([0, 5, 5, 18, 26])   # four utterances, one empty; two rows behind cu_seqlens[-1]
    labels = torch.randint(0, 257, (1, 28), generator=g)
    labels[0, [4, 17, 25]] = -100
    batch = dict(inputs_embeds=torch.randn(1, 28, 128, generator=g) * 0.5, labels=labels, cu_seqlens=cu)
    seq = m.sequence_logprobs(**batch)
    assert seq["tokens"].tolist()[1] == 0 and seq["logp"][1] == 0
    _check_head(m, m.score(**batch), seq, 4)
    m.config.strict_reference_loss = True
    _check_head(m, m.score(**batch), m.sequence_logprobs(**batch), 5)


def test_cosy_sequence_logprobs_one_sequence_per_utterance():
    cfg = RWKV7CosyConfig(vocab_size=200, speech_token_size=50, lsm_weight=0.0, drop_ratio=0.1, **SMALL)
    llm = _stubbed(RWKV7CosyLM(cfg), 200, 3).eval()
    batch = _cosy_batch()
    seq = llm.sequence_logprobs(batch=batch)
    assert seq["tokens"].tolist() == [11, 4]
    _check_head(llm, llm.score(batch=batch), seq, 2)
    with torch.no_grad():   # the plain log-softmax at the target
        lp = F.log_softmax(llm(batch=batch).logits.double(), dim=-1)
        tgt = llm.build_inputs(batch)[2]
        want = (lp.gather(2, tgt.clamp(min=0).unsqueeze(2)).squeeze(2) * (tgt != -1)).sum(1)
    assert bool(((seq["logp"].detach() - want).abs() <= 1e-5 * want.abs()).all())
    torch.manual_seed(9)
    w = RWKV7LM(128, 128, 50, llm, lsm_weight=0.0, drop_ratio=0.1).eval()
    llm.zero_grad()
    _check_head(llm, w.score(batch), w.sequence_logprobs(batch), 2)
    # with label smoothing the score is the KL, the log-probability stays the plain one
    llm.config.lsm_weight = 0.1
    assert torch.equal(llm.sequence_logprobs(batch=batch)["logp"].detach(), seq["logp"].detach())
    assert not hasattr(RWKV7XYLM, "sequence_logprobs"), "the XY model is out of scope"


# ---- DataParallelTrainer.preference_step -------------------------------------------------------------------------------------------
def _pairs(seed, P=2, T=12):
    """2P utterances (chosen, rejected, chosen, ...) as one padded Spark batch."""
    return _spark_batch(seed, B=2 * P, T=T)


def _policy_logps(model, batch):
    """Plain logits -> log_softmax -> the shifted labels' log-probabilities summed per utterance (fp64), and the token counts."""
    logits = model(inputs_embeds=batch["inputs_embeds"], attention_mask=batch["attention_mask"]).logits
    lab = torch.cat((batch["labels"][:, 1:], torch.full_like(batch["labels"][:, :1], -100)), 1)
    lp = F.log_softmax(logits.double(), dim=-1).gather(2, lab.clamp(min=0).unsqueeze(2)).squeeze(2)
    return (lp * (lab != -100)).sum(1), (lab != -100).sum(1)


def _dpo_loss(model, batch, ref, beta, sft_weight=0.0):
    logp, tokens = _policy_logps(model, batch)
    margin = beta * ((logp[0::2] - logp[1::2]) - (ref[0::2] - ref[1::2]))
    return F.softplus(-margin).mean() - sft_weight * logp[0::2].sum() / tokens[0::2].sum()


def _hand_written_step(model, shards, refs, lr, beta, sft_weight=0.0, betas=(0.9, 0.95), eps=1e-3):
    """The first AdamW step (zero moments, no weight decay) on the mean over the shards of the DPO loss; the parameters afterwards."""
    params = [p for p in model.parameters() if p.requires_grad]
    loss = sum(_dpo_loss(model, b, r, beta, sft_weight) for b, r in zip(shards, refs)) / len(shards)
    grads = torch.autograd.grad(loss, params, allow_unused=True)
    out = []
    for p, g in zip(params, grads):
        g = torch.zeros_like(p) if g is None else g
        m, v = (1 - betas[0]) * g, (1 - betas[1]) * g * g
        out.append(p.detach() - lr / (1 - betas[0]) * m / (v.sqrt() / (1 - betas[1]) ** 0.5 + eps))
    return out


def _ref_logps(seed, n):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 3


def _assert_params_match(got, want, before):
    err = max((a - b).abs().max().item() for a, b in zip(got, want))
    moved = max((a - b).abs().max().item() for a, b in zip(want, before))
    assert moved > 1e-3, "the step must move the parameters for the comparison to mean something"
    assert err <= 1e-5, f"parameters differ from the hand-written DPO step by {err}"


@pytest.mark.parametrize("sft_weight", [0.0, 0.3])
def test_one_rank_equals_the_hand_written_dpo_step(sft_weight):
    m = _spark().eval()   # eval mode: no dropout draw on either side
    twin = copy.deepcopy(m)
    batch, ref = _pairs(40), _ref_logps(41, 4)
    tr = trainer.DataParallelTrainer(m, **OPT)
    out = tr.preference_step(beta=BETA, ref_logps=ref.numpy(), sft_weight=sft_weight, **batch)
    assert set(out) == {"loss", "margin", "accuracy", "logp_chosen", "logp_rejected"} and tr.step_idx == 1
    assert all(torch.is_tensor(v) and not v.requires_grad for v in out.values())
    assert out["logp_chosen"].shape == out["logp_rejected"].shape == (2,)
    with torch.no_grad():
        logp, _ = _policy_logps(twin, batch)
        assert abs(out["loss"].item() - _dpo_loss(twin, batch, ref, BETA, sft_weight).item()) <= 1e-6
    margin = BETA * ((logp[0::2] - logp[1::2]) - (ref[0::2] - ref[1::2]))
    assert abs(out["margin"].item() - margin.mean().item()) <= 1e-5 and out["accuracy"].item() == (margin > 0).double().mean().item()
    before = [p.detach().clone() for p in twin.parameters()]
    want = _hand_written_step(twin, [batch], [ref], tr.last_lr, BETA, sft_weight)
    _assert_params_match([p.detach() for p in m.parameters()], want, before)


def test_ref_logps_none_means_zeros():
    a, b = (trainer.DataParallelTrainer(_spark().eval(), **OPT) for _ in range(2))
    batch = _pairs(42)
    oa = a.preference_step(beta=BETA, **batch)
    ob = b.preference_step(beta=BETA, ref_logps=torch.zeros(4), **batch)
    assert torch.equal(oa["loss"], ob["loss"]) and torch.equal(a.flat.flat_param, b.flat.flat_param)


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    trainer.init_distributed("gloo")
    torch.set_num_threads(1)
    tr = trainer.DataParallelTrainer(_spark().eval(), bucket_bytes=4096, **OPT)
    out = tr.preference_step(beta=BETA, ref_logps=_ref_logps(60 + rank, 4), **_pairs(50 + rank))
    q.put((rank, [p.detach().numpy().copy() for p in tr.model.parameters()], out["loss"].item(), tr.last_lr))   # by value
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_gloo_ranks_equal_the_hand_written_dpo_step_on_both_shards():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert all(np.array_equal(a, b) for a, b in zip(res[0][1], res[1][1])), "the replicas must stay identical"
    twin = _spark().eval()
    before = [p.detach().clone() for p in twin.parameters()]
    want = _hand_written_step(twin, [_pairs(50), _pairs(51)], [_ref_logps(60, 4), _ref_logps(61, 4)], res[0][3], BETA)
    _assert_params_match([torch.from_numpy(a) for a in res[0][1]], want, before)


def test_the_mean_margin_rises_over_five_steps_on_four_fixed_pairs():
    tr = trainer.DataParallelTrainer(_spark().eval(), **OPT)
    batch, ref = _pairs(43, P=4), _ref_logps(44, 8)
    margins = [tr.preference_step(beta=BETA, ref_logps=ref, **batch)["margin"].item() for _ in range(5)]
    assert margins[-1] > margins[0] and tr.step_idx == 5, margins


def _moving(tr):
    return {k: v for k, v in _state(tr).items() if k in ("param", "master", "exp_avg", "exp_avg_sq")}


def test_nan_in_ref_logps_is_a_zero_gradient_step():
    batch, ref = _pairs(45), _ref_logps(46, 4)
    bad = ref.clone()
    bad[2] = float("nan")
    # from a fresh state (zero moments) a zero-gradient step leaves parameters and moments as they were
    tr = trainer.DataParallelTrainer(_spark().eval(), **OPT)
    before = _moving(tr)
    out = tr.preference_step(beta=BETA, ref_logps=bad, **batch)
    assert tr.nan_flag.item() == 1 and tr.step_idx == 1 and not torch.isfinite(out["loss"])
    _assert_same_state(before, _moving(tr))
    # an infinite entry leaves the loss finite (softplus saturates) and must raise the flag all the same
    bad[2], bad[3] = ref[2], float("inf")
    out = tr.preference_step(beta=BETA, ref_logps=bad, **batch)
    assert tr.nan_flag.item() == 1 and torch.isfinite(out["loss"])
    _assert_same_state(before, _moving(tr))
    # from a warm state it is step()'s NaN rule: what a step() on a NaN loss leaves behind, bit for bit
    a, b = (trainer.DataParallelTrainer(_spark().eval(), **OPT) for _ in range(2))
    for t in (a, b):
        t.preference_step(beta=BETA, ref_logps=ref, **batch)
        t.step(**_spark_batch(47))
    warm = _moving(a)
    bad[3] = float("nan")
    a.preference_step(beta=BETA, ref_logps=bad, **batch)
    poisoned = _spark_batch(48)
    poisoned["inputs_embeds"][0, 5, 7] = float("nan")
    assert not torch.isfinite(b.step(**poisoned))
    _assert_same_state(_moving(a), _moving(b))
    assert not torch.equal(warm["exp_avg"], a.exp_avg) and bool(torch.isfinite(a.flat.flat_param).all())
    a.preference_step(beta=BETA, ref_logps=ref, **batch)   # the next clean step trains
    assert a.nan_flag.item() == 0


def test_odd_utterance_count_and_wrong_ref_length_raise_and_leave_the_trainer_usable():
    tr = trainer.DataParallelTrainer(_spark().eval(), **OPT)
    with pytest.raises(ValueError):
        tr.preference_step(beta=BETA, **_spark_batch(49, B=3))
    with pytest.raises(ValueError):
        tr.preference_step(beta=BETA, ref_logps=np.zeros(3), **_pairs(49))
    assert tr.step_idx == 0 and all(p.grad is not None for p in tr.model.parameters())
    tr.preference_step(beta=BETA, **_pairs(49))
    assert tr.step_idx == 1


def test_inside_an_accumulation_window_raises():
    tr = trainer.DataParallelTrainer(_spark().eval(), **OPT)
    tr.accumulate(**_spark_batch(1))
    with pytest.raises(RuntimeError, match="accumulation window"):
        tr.preference_step(beta=BETA, **_pairs(2))
    tr.step(**_spark_batch(2))
    tr.preference_step(beta=BETA, **_pairs(2))


def test_a_step_after_a_preference_step_equals_a_step_after_loading_that_state(tmp_path):
    torch.manual_seed(5)
    a = trainer.DataParallelTrainer(_spark().train(), **OPT)   # training mode: dropout draws, the checkpoint carries the RNG
    a.step(**_spark_batch(70))
    a.preference_step(beta=BETA, ref_logps=_ref_logps(71, 4), **_pairs(72))
    a.save_checkpoint(str(tmp_path))
    a.step(**_spark_batch(73))
    torch.manual_seed(6)
    b = trainer.DataParallelTrainer(_spark(seed=2).train(), **OPT)
    b.load_checkpoint(str(tmp_path))
    b.step(**_spark_batch(73))
    _assert_same_state(_state(a), _state(b))
