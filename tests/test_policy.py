"""CPU: policy-gradient (GRPO / PPO-clip) training -- the C ABI of rwkv7_ce_policy_fwd_bwd_bf16, losses.group_advantages,
losses.fused_linear_policy on its torch route, the heads' policy_loss / token_logprobs and DataParallelTrainer.policy_step (DESIGN.md
section 6.7).

What the values are compared against:
  * fused_linear_policy: plain autograd in fp64 (log_softmax -> gather -> exp -> minimum / clamp -> k3 KL) on the same numbers.  The
    bar for dh / dW / db is 2 x the relative L2 error of fused_linear_cross_entropy against ITS fp64 restatement on the same shape.
  * the reduction: with old_logps = token_logprobs, advantages = 1, no KL and normalize = "token" every ratio is 1, the loss is -1 and
    its gradient is that of the token-mean negative log-likelihood: policy_step must move the parameters as step does (1e-5, the bar
    of preference_step's comparisons; eps = 1e-3 for the reason given in test_preference).
  * policy_step: a hand-written GRPO step from materialised logits (fp64 log_softmax, torch.minimum / clamp, the AdamW rule of the
    trainer's torch path), parameters within 1e-5, on one and on two gloo ranks.
The heads run on test_head_eval's CPU stand-in for the backbone; the real one is in test_policy_gpu.py."""
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
from test_preference import _assert_params_match, _moving, _rel_l2
from test_trainer_dist import _free_port

NAME = "rwkv7_ce_policy_fwd_bwd_bf16"
OPT = dict(lr=1e-2, warmup_steps=0, total_steps=100, eps=1e-3)
CLIP, BETA = (0.2, 0.3), 0.4


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_and_the_library_exports_it(hip_lib):
    assert NAME in _lib.exported_symbols()
    restype, argtypes = _lib.prototypes()[NAME]
    P, L, I, Fl = ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_float
    # rows, V, ld, logits, labels, ignore_index, row0, n_seq, seq_start, adv, seq_w, old_lp, ref_lp, eps_lo, eps_hi, beta, the four
    # per-row outputs, the stream
    assert restype is I and argtypes == [L, I, L, P, P, L, L, L, P, P, P, P, P, Fl, Fl, Fl, P, P, P, P, P]
    fn = getattr(hip_lib, NAME)
    assert fn.restype is I and list(fn.argtypes) == argtypes


def test_entry_point_rejects_bad_arguments_before_any_launch(hip_lib):
    one = 16   # never dereferenced: the checks fire first
    names = ["logits", "labels", "seq_start", "adv", "seq_w", "old_lp"]

    def call(rows=5, V=11, ld=16, row0=0, n_seq=2, eps_lo=0.2, eps_hi=0.2, **null):
        p = {n: (None if n in null else one) for n in names}
        return getattr(hip_lib, NAME)(rows, V, ld, p["logits"], p["labels"], -100, row0, n_seq, p["seq_start"], p["adv"], p["seq_w"],
                                      p["old_lp"], None, eps_lo, eps_hi, 0.1, None, None, None, None, None)

    for n in names:
        assert call(**{n: True}) == -1, n
    assert call(rows=0) == -1 and call(V=0) == -1 and call(ld=10) == -1 and call(row0=-1) == -1 and call(n_seq=0) == -1
    assert call(eps_lo=-0.1) == -1 and call(eps_lo=1.0) == -1 and call(eps_hi=-0.1) == -1 and call(eps_lo=float("nan")) == -1


# ---- group_advantages --------------------------------------------------------------------------------------------------------------
def test_group_advantages_have_zero_mean_per_group_and_vanish_for_constant_groups():
    r = torch.tensor([1.0, 2.0, 4.0, 9.0, 3.0, 3.0, 3.0, 3.0, -1.0, 0.0, 0.5, 7.0])
    a = losses.group_advantages(r, 4)
    assert a.shape == r.shape and a.dtype == r.dtype
    assert bool((a.reshape(3, 4).sum(1).abs() <= 1e-6).all())
    assert bool((a[4:8] == 0).all()), "a group of equal rewards"
    g = r[:4]
    want = (g - g.mean()) / (g.std(unbiased=False) + 1e-6)
    assert torch.allclose(a[:4], want, rtol=1e-6, atol=0) and a[3] > a[2] > a[1] > a[0]
    assert losses.group_advantages([1, 2, 3, 4], 2).tolist() == pytest.approx([-1, 1, -1, 1], abs=1e-5)
    with pytest.raises(ValueError):
        losses.group_advantages(r, 5)


# ---- fused_linear_policy, torch route ----------------------------------------------------------------------------------------------
N, D, V = 200, 256, 1025
# rows 0-2 in front of seq_start[0]; an empty sequence; sequences of 1, 56, 40 (all ignored), 90 rows; rows 190-199 behind
SEQ_START = [3, 3, 4, 60, 100, 190]
IGNORED_ONLY = 3


def policy_case(seed=0, dtype=torch.float32, device="cpu"):
    """Inputs of the fused_linear_policy tests (also test_policy_gpu's, in bf16): h, w, b, labels, seq_start, adv, seq_w, old, ref.
    old is the fp64 log-probability of the (rounded) inputs plus noise wide enough that both branches of the clip are well
    populated; advantages of both signs."""
    g = torch.Generator().manual_seed(seed)
    h = (torch.randn(N, D, generator=g) * 0.5).to(dtype)
    w = (torch.randn(V, D, generator=g) * 0.1).to(dtype)
    b = (torch.randn(V, generator=g) * 0.1).to(dtype)
    lab = torch.randint(0, V, (N,), generator=g)
    lab[[1, 7, 150, 195]] = -100
    lab[120] = V - 1
    lab[SEQ_START[IGNORED_ONLY]:SEQ_START[IGNORED_ONLY + 1]] = -100
    lp = F.log_softmax(F.linear(h.double(), w.double(), b.double()), dim=1).gather(1, lab.clamp(min=0).unsqueeze(1)).squeeze(1)
    old = (lp + (torch.rand(N, generator=g, dtype=torch.float64) - 0.5) * 2.0).float()
    ref = (lp + (torch.rand(N, generator=g, dtype=torch.float64) - 0.5) * 0.6).float()
    adv = torch.tensor([0.7, -0.4, -0.9, 1.3, 0.8])
    seq_w = torch.tensor([0.3, 0.5, 1.0 / 56, 0.25, 1.0 / 90])
    return tuple(t.to(device) for t in (h, w, b, lab, torch.tensor(SEQ_START), adv, seq_w, old, ref))


def policy_fp64(h, w, b, lab, st, adv, seq_w, old, ref, clip, beta, ignore=-100, count=None):
    """The definition in plain autograd, fp64: (loss, lp, kl, clipped, rho) with lp / kl / clipped / rho [N] masked to the rows that
    count.  count: how often each row enters the loss (None: once)."""
    lp = F.log_softmax(F.linear(h.double(), w.double(), None if b is None else b.double()), dim=1)
    lp = lp.gather(1, lab.clamp(min=0).unsqueeze(1)).squeeze(1)
    s, inside = losses._row_sequences(st, 0, lab.numel())
    on = inside & (lab != ignore)
    A, rho = adv.double()[s], torch.exp(lp - old.double())
    s1, s2 = rho * A, rho.clamp(1 - clip[0], 1 + clip[1]) * A
    per = -torch.minimum(s1, s2)
    kl = torch.zeros_like(lp)
    if ref is not None:
        d = ref.double() - lp
        kl = torch.exp(d) - d - 1
        per = per + beta * kl
    weight = seq_w.double()[s] * on if count is None else seq_w.double()[s] * on * count
    return (per * weight).sum(), lp.detach() * on, kl.detach() * on, ((s1 > s2) & on).detach(), rho.detach()


def ce_yardstick(h, w, b, lab, chunk):
    """Relative L2 errors (dh, dW, db) of fused_linear_cross_entropy against its fp64 restatement on the same inputs."""
    leaves = [t.clone().requires_grad_() for t in (h, w, b)]
    losses.fused_linear_cross_entropy(leaves[0], lab, leaves[1], leaves[2], -100, chunk=chunk).backward()
    refs = [t.double().requires_grad_() for t in (h, w, b)]
    F.cross_entropy(F.linear(*refs), lab, ignore_index=-100).backward()
    return [_rel_l2(a.grad, r.grad) for a, r in zip(leaves, refs)]


@pytest.mark.parametrize("with_ref", [True, False])
@pytest.mark.parametrize("chunk", [64, 128, N])
def test_torch_route_against_fp64_autograd(with_ref, chunk):
    h, w, b, lab, st, adv, seq_w, old, ref = policy_case()
    ref = ref if with_ref else None
    leaves = [t.clone().requires_grad_() for t in (h, w, b)]
    hits = losses.POLICY_HITS[0]
    loss, rows = losses.fused_linear_policy(leaves[0], lab, leaves[1], leaves[2], -100, seq_start=st, adv=adv, seq_w=seq_w, old_logp=old,
                                            ref_logp=ref, clip=CLIP, kl_beta=BETA, chunk=chunk)
    assert loss.dtype == torch.float64 and loss.shape == () and loss.requires_grad
    assert set(rows) == {"logp", "kl", "clipped"} and all(v.shape == (N,) and not v.requires_grad for v in rows.values())
    (loss * 1.7).backward()
    assert losses.POLICY_HITS[0] == hits, "CPU tensors must take the torch route"
    refs = [t.double().requires_grad_() for t in (h, w, b)]
    want, lp, kl, clipped, rho = policy_fp64(*refs, lab, st, adv, seq_w, old, ref, CLIP, BETA)
    (want * 1.7).backward()
    on = lp != 0
    assert int(on.sum()) == 1 + 55 + 89 and 0.25 * on.sum() <= clipped.sum() <= 0.75 * on.sum(), (on.sum(), clipped.sum())
    assert abs(loss.item() - want.item()) <= 1e-5 * abs(want.item())
    assert bool(((rows["logp"] - lp).abs() <= 1e-5).all()) and bool(((rows["kl"] - kl).abs() <= 1e-5).all())
    assert (rows["kl"] != 0).any().item() == with_ref
    near = ((rho / (1 - CLIP[0]) - 1).abs() <= 1e-4) | ((rho / (1 + CLIP[1]) - 1).abs() <= 1e-4)
    assert torch.equal(rows["clipped"][~near] != 0, clipped[~near])
    yard = ce_yardstick(h, w, b, lab, chunk)
    for name, a, r, y in zip(("dh", "dW", "db"), leaves, refs, yard):
        assert a.grad.dtype == a.dtype and a.grad.shape == a.shape
        assert _rel_l2(a.grad, r.grad) <= 2 * y, (name, _rel_l2(a.grad, r.grad), y)
    dh = leaves[0].grad
    outside = [0, 1, 2, 7, 150] + list(range(60, 100)) + list(range(190, 200))
    assert bool((dh[outside] == 0).all()) and bool((dh[3] != 0).any()) and bool((dh[189] != 0).any())


def test_arguments_are_checked():
    h, w, b, lab, st, adv, seq_w, old, ref = policy_case()
    kw = dict(seq_start=st, adv=adv, seq_w=seq_w, old_logp=old)
    for bad in (dict(seq_start=None), dict(seq_start=torch.zeros(1, dtype=torch.int64)), dict(adv=adv[:3]), dict(old_logp=old[:7]),
                dict(ref_logp=ref[:7]), dict(clip=(1.0, 0.2)), dict(clip=(0.2, -0.1))):
        with pytest.raises(ValueError):
            losses.fused_linear_policy(h, lab, w, b, -100, **{**kw, **bad})


# ---- the heads ---------------------------------------------------------------------------------------------------------------------
def _shifted(labels):
    return torch.cat((labels[:, 1:], torch.full_like(labels[:, :1], -100)), 1)


def test_spark_token_logprobs_are_the_scores_rows():
    m = _spark().train()
    batch = _spark_batch(3)
    lp = m.token_logprobs(**batch)
    assert m.training and lp.shape == (24,) and lp.dtype == torch.float32 and not lp.requires_grad
    lab = _shifted(batch["labels"]).reshape(-1)
    assert bool((lp[lab == -100] == 0).all()) and bool((lp[lab != -100] < 0).all())
    score = m.score(**batch)
    assert torch.allclose(lp.double().reshape(2, 12).sum(1), -score["loss_sum"], rtol=1e-6, atol=0)
    m.eval()
    with torch.no_grad():
        want = F.log_softmax(m(**{k: v for k, v in batch.items() if k != "labels"}).logits.double(), dim=-1)
        want = want.gather(2, lab.clamp(min=0).reshape(2, 12, 1)).reshape(-1) * (lab != -100)
    assert bool(((lp - want).abs() <= 1e-5).all())


def _reduction(m, batch, n_seq, **kw):
    """old_logps = token_logprobs, advantages = 1, no KL, normalize = "token": loss -1, every ratio 1, nothing clipped."""
    old = m.token_logprobs(**batch)
    out = m.policy_loss(advantages=torch.ones(n_seq), old_logps=old, normalize="token", **kw, **batch)
    assert set(out) == {"loss", "logp", "kl", "clipped", "valid"} and out["loss"].requires_grad
    assert abs(out["loss"].item() + 1.0) <= 1e-5 and not bool(out["clipped"].any()) and not bool(out["kl"].any())
    assert bool(((out["logp"] - old).abs() <= 1e-5).all()) and torch.equal(out["valid"], old != 0)
    return out


def test_spark_policy_loss_padded_reduces_to_the_token_mean_log_likelihood():
    m = _spark().eval()
    batch = _spark_batch(3)
    out = _reduction(m, batch, 2)
    out["loss"].backward()
    got = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    assert "model.mix.weight" in got and "lm_head.weight" in got, "the gradient must reach the backbone and the head"
    m.zero_grad()
    m(**batch).loss.backward()   # the mean cross-entropy over the same positions
    for n, p in m.named_parameters():
        if p.grad is not None:
            assert _rel_l2(got[n], p.grad) <= 1e-5, n


def test_spark_policy_loss_packed_cu_seqlens_against_materialised_logits():
    """The packed layout against the definition from materialised logits.  Packed against padded batches of the same utterances needs
    a backbone that honours cu_seqlens, which the CPU stand-in does not:
    test_policy_gpu.py::test_packed_cu_seqlens_and_padded_batches_of_the_same_utterances_agree."""
    m = _spark().eval()
    g = torch.Generator().manual_seed(8)
    cu = torch.tensor([0, 5, 5, 18, 26])   # four utterances, one empty; two rows behind cu_seqlens[-1]
    labels = torch.randint(0, 257, (1, 28), generator=g)
    labels[0, [4, 17, 25]] = -100
    emb = torch.randn(1, 28, 128, generator=g) * 0.5
    adv = torch.tensor([0.5, 2.0, -1.0, 1.5])
    packed = dict(inputs_embeds=emb, labels=labels, cu_seqlens=cu)
    _reduction(m, packed, 4)
    old = m.token_logprobs(**packed) + (torch.rand(28, generator=g) - 0.5) * 0.8
    ref = m.token_logprobs(**packed) + (torch.rand(28, generator=g) - 0.5) * 0.4
    lab = _shifted(labels).reshape(-1)
    lab[26:] = -100
    for normalize in ("sequence", "token"):
        a = m.policy_loss(advantages=adv, old_logps=old, ref_logps=ref, clip=CLIP, kl_beta=BETA, normalize=normalize, **packed)
        assert 0 < a["clipped"].sum() < a["valid"].sum() == 23 and torch.equal(a["valid"], lab != -100)
        lp = F.log_softmax(m(inputs_embeds=emb, cu_seqlens=cu).logits.double()[0], dim=-1).gather(1, lab.clamp(min=0).unsqueeze(1))[:, 0]
        rho, d = torch.exp(lp - old), ref - lp
        A = adv.double()[torch.searchsorted(cu, torch.arange(28), right=True).clamp(max=4) - 1]
        per = (-torch.minimum(rho * A, rho.clamp(1 - CLIP[0], 1 + CLIP[1]) * A) + BETA * (torch.exp(d) - d - 1)) * (lab != -100)
        utt = [per[s:e].sum() / max(int((lab[s:e] != -100).sum()), 1) for s, e in zip(cu[:-1].tolist(), cu[1:].tolist())]
        want = sum(utt) / 4 if normalize == "sequence" else per.sum() / 23
        assert abs(a["loss"].item() - want.item()) <= 1e-5 * abs(want.item()), normalize
        ga = torch.autograd.grad(a["loss"], list(m.lm_head.parameters()) + [m.model.mix.weight])
        gb = torch.autograd.grad(want, list(m.lm_head.parameters()) + [m.model.mix.weight])
        assert all(_rel_l2(x, y) <= 1e-5 for x, y in zip(ga, gb))
    with pytest.raises(ValueError):
        m.policy_loss(advantages=adv[:3], old_logps=old, **packed)
    with pytest.raises(ValueError):
        m.policy_loss(advantages=adv, old_logps=old, normalize="batch", **packed)


def test_cosy_policy_loss_and_token_logprobs():
    cfg = RWKV7CosyConfig(vocab_size=200, speech_token_size=50, lsm_weight=0.1, drop_ratio=0.1, **SMALL)
    llm = _stubbed(RWKV7CosyLM(cfg), 200, 3).eval()
    batch = _cosy_batch()
    lp = llm.token_logprobs(batch=batch)
    tgt = llm.build_inputs(batch)[2]
    with torch.no_grad():   # the plain log-softmax at the target, whatever lsm_weight says
        want = F.log_softmax(llm(batch=batch).logits.double(), dim=-1).gather(2, tgt.clamp(min=0).unsqueeze(2)).squeeze(2) * (tgt != -1)
    assert lp.shape == (tgt.numel(),) and bool(((lp - want.reshape(-1)).abs() <= 1e-5).all()) and int((lp != 0).sum()) == 15
    out = _reduction(llm, dict(batch=batch), 2)
    out["loss"].backward()
    assert llm.model.mix.weight.grad is not None and bool((llm.lm_head.weight.grad != 0).any())
    torch.manual_seed(9)
    w = RWKV7LM(128, 128, 50, llm, lsm_weight=0.0, drop_ratio=0.1).eval()
    _reduction(w, dict(batch=batch), 2)
    assert not hasattr(RWKV7XYLM, "policy_loss") and not hasattr(RWKV7XYLM, "token_logprobs"), "the XY model is out of scope"


# ---- DataParallelTrainer.policy_step -----------------------------------------------------------------------------------------------
def _grpo_inputs(model, batch, seed):
    """(advantages, old_logps, ref_logps) of a Spark batch: group advantages of random rewards, and the model's own token
    log-probabilities moved by noise wide enough to clip some rows."""
    g = torch.Generator().manual_seed(seed)
    B = batch["labels"].shape[0]
    lp = model.token_logprobs(**batch)
    adv = losses.group_advantages(torch.randn(B, generator=g), B)
    return adv, lp + (torch.rand(lp.shape, generator=g) - 0.5) * 0.8, lp + (torch.rand(lp.shape, generator=g) - 0.5) * 0.4


def _grpo_loss(model, batch, adv, old, ref, clip, beta):
    """GRPO from materialised logits in fp64: mean over the utterances of the token mean of -min(rho A, clamp(rho) A) + beta k3."""
    logits = model(inputs_embeds=batch["inputs_embeds"], attention_mask=batch["attention_mask"]).logits
    lab = _shifted(batch["labels"])
    lp = F.log_softmax(logits.double(), dim=-1).gather(2, lab.clamp(min=0).unsqueeze(2)).squeeze(2)
    on = lab != -100
    rho, A = torch.exp(lp - old.double().reshape(lp.shape)), adv.double().unsqueeze(1)
    per = -torch.minimum(rho * A, rho.clamp(1 - clip[0], 1 + clip[1]) * A)
    if ref is not None:
        d = ref.double().reshape(lp.shape) - lp
        per = per + beta * (torch.exp(d) - d - 1)
    return ((per * on).sum(1) / on.sum(1)).mean()


def _hand_written_step(model, shards, inputs, lr, clip, beta, betas=(0.9, 0.95), eps=1e-3):
    """The first AdamW step (zero moments, no weight decay) on the mean over the shards of the GRPO loss; the parameters afterwards."""
    params = [p for p in model.parameters() if p.requires_grad]
    loss = sum(_grpo_loss(model, b, *i, clip, beta) for b, i in zip(shards, inputs)) / len(shards)
    grads = torch.autograd.grad(loss, params, allow_unused=True)
    out = []
    for p, g in zip(params, grads):
        g = torch.zeros_like(p) if g is None else g
        m, v = (1 - betas[0]) * g, (1 - betas[1]) * g * g
        out.append(p.detach() - lr / (1 - betas[0]) * m / (v.sqrt() / (1 - betas[1]) ** 0.5 + eps))
    return out


@pytest.mark.parametrize("with_ref", [True, False])
def test_one_rank_equals_the_hand_written_grpo_step(with_ref):
    m = _spark().eval()   # eval mode: no dropout draw on either side
    twin = copy.deepcopy(m)
    batch = _spark_batch(40, B=4)
    adv, old, ref = _grpo_inputs(m, batch, 41)
    ref = ref if with_ref else None
    tr = trainer.DataParallelTrainer(m, **OPT)
    out = tr.policy_step(advantages=adv, old_logps=old, ref_logps=ref, clip=CLIP, kl_beta=BETA, **batch)
    assert list(out) == ["loss", "clip_frac", "kl", "ratio_mean"] and tr.step_idx == 1
    assert all(torch.is_tensor(v) and v.shape == () and not v.requires_grad for v in out.values())
    with torch.no_grad():
        assert abs(out["loss"].item() - _grpo_loss(twin, batch, adv, old, ref, CLIP, BETA).item()) <= 1e-6
    assert 0 < out["clip_frac"].item() < 1 and (out["kl"].item() > 0) == with_ref and 0.7 < out["ratio_mean"].item() < 1.4
    before = [p.detach().clone() for p in twin.parameters()]
    want = _hand_written_step(twin, [batch], [(adv, old, ref)], tr.last_lr, CLIP, BETA)
    _assert_params_match([p.detach() for p in m.parameters()], want, before)


def test_reduction_policy_step_moves_the_parameters_as_step_does():
    a, b = (trainer.DataParallelTrainer(_spark().eval(), **OPT) for _ in range(2))
    batch = _spark_batch(42, B=3)
    old = a.token_logprobs([batch])[0]
    out = a.policy_step(advantages=np.ones(3), old_logps=old, normalize="token", **batch)
    assert abs(out["loss"].item() + 1) <= 1e-5 and out["clip_frac"].item() == 0 and abs(out["ratio_mean"].item() - 1) <= 1e-5
    before = [p.detach().clone() for p in b.model.parameters()]
    b.step(**batch)
    _assert_params_match([p.detach() for p in a.model.parameters()], [p.detach() for p in b.model.parameters()], before)


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    trainer.init_distributed("gloo")
    torch.set_num_threads(1)
    tr = trainer.DataParallelTrainer(_spark().eval(), bucket_bytes=4096, **OPT)
    batch = _spark_batch(50 + rank, B=4)
    adv, old, ref = _grpo_inputs(tr.model, batch, 60 + rank)
    out = tr.policy_step(advantages=adv, old_logps=old, ref_logps=ref, clip=CLIP, kl_beta=BETA, **batch)
    q.put((rank, [p.detach().numpy().copy() for p in tr.model.parameters()], out["loss"].item(), tr.last_lr))   # by value
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_gloo_ranks_equal_the_hand_written_grpo_step_on_both_shards():
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
    shards = [_spark_batch(50, B=4), _spark_batch(51, B=4)]
    inputs = [_grpo_inputs(twin, b, 60 + r) for r, b in enumerate(shards)]
    want = _hand_written_step(twin, shards, inputs, res[0][3], CLIP, BETA)
    _assert_params_match([torch.from_numpy(a) for a in res[0][1]], want, before)


def test_non_finite_inputs_make_steps_zero_gradient_step():
    batch = _spark_batch(45, B=4)
    a, b = (trainer.DataParallelTrainer(_spark().eval(), **OPT) for _ in range(2))
    adv, old, ref = _grpo_inputs(a.model, batch, 46)
    for t in (a, b):
        t.policy_step(advantages=adv, old_logps=old, ref_logps=ref, kl_beta=BETA, **batch)
        t.step(**_spark_batch(47))
    warm = _moving(a)
    valid_row = 2
    assert _shifted(batch["labels"]).reshape(-1)[valid_row] != -100
    bad = old.clone()
    bad[valid_row] = float("nan")
    out = a.policy_step(advantages=adv, old_logps=bad, ref_logps=ref, kl_beta=BETA, **batch)
    assert a.nan_flag.item() == 1 and not torch.isfinite(out["loss"])
    poisoned = _spark_batch(48)
    poisoned["inputs_embeds"][0, 5, 7] = float("nan")
    assert not torch.isfinite(b.step(**poisoned))
    _assert_same_state(_moving(a), _moving(b))   # step()'s NaN rule, bit for bit
    assert not torch.equal(warm["exp_avg"], a.exp_avg) and bool(torch.isfinite(a.flat.flat_param).all())
    # a non-finite entry on a row that does not count is never read
    ignored = int((_shifted(batch["labels"]).reshape(-1) == -100).nonzero()[0])
    ok = old.clone()
    ok[ignored] = float("inf")
    out = a.policy_step(advantages=adv, old_logps=ok, ref_logps=ref, kl_beta=BETA, **batch)
    assert a.nan_flag.item() == 0 and torch.isfinite(out["loss"])
    # an infinite reference entry or advantage raises the flag as well (the loss may stay finite): from a fresh state (zero moments)
    # a zero-gradient step leaves parameters and moments as they were
    c = trainer.DataParallelTrainer(_spark().eval(), **OPT)
    before = _moving(c)
    for kw in (dict(ref_logps=torch.where(torch.arange(ref.numel()) == valid_row, float("-inf"), ref)),
               dict(ref_logps=ref, advantages=torch.tensor([1.0, float("inf"), 0.0, -1.0]))):
        c.policy_step(**{**dict(advantages=adv, old_logps=old, kl_beta=BETA), **kw}, **batch)
        assert c.nan_flag.item() == 1
        _assert_same_state(before, _moving(c))


def test_wrong_lengths_raise_and_leave_the_trainer_usable():
    tr = trainer.DataParallelTrainer(_spark().eval(), **OPT)
    batch = _spark_batch(49, B=4)
    adv, old, _ = _grpo_inputs(tr.model, batch, 1)
    with pytest.raises(ValueError):
        tr.policy_step(advantages=adv[:3], old_logps=old, **batch)
    with pytest.raises(ValueError):
        tr.policy_step(advantages=adv, old_logps=old[:5], **batch)
    assert tr.step_idx == 0 and all(p.grad is not None for p in tr.model.parameters())
    tr.policy_step(advantages=adv, old_logps=old, **batch)
    assert tr.step_idx == 1


def test_inside_an_accumulation_window_raises():
    tr = trainer.DataParallelTrainer(_spark().eval(), **OPT)
    batch = _spark_batch(2, B=4)
    adv, old, _ = _grpo_inputs(tr.model, batch, 3)
    tr.accumulate(**_spark_batch(1))
    with pytest.raises(RuntimeError, match="accumulation window"):
        tr.policy_step(advantages=adv, old_logps=old, **batch)
    with pytest.raises(RuntimeError, match="accumulation window"):
        tr.token_logprobs([batch])
    tr.step(**_spark_batch(2))
    tr.policy_step(advantages=adv, old_logps=old, **batch)


def test_a_step_after_a_policy_step_equals_a_step_after_loading_that_state(tmp_path):
    torch.manual_seed(5)
    a = trainer.DataParallelTrainer(_spark().train(), **OPT)   # training mode: dropout draws, the checkpoint carries the RNG
    a.step(**_spark_batch(70))
    batch = _spark_batch(72, B=4)
    adv, old, ref = _grpo_inputs(a.model, batch, 71)
    assert a.model.training, "token_logprobs restores the mode"
    a.policy_step(advantages=adv, old_logps=old, ref_logps=ref, kl_beta=BETA, **batch)
    a.save_checkpoint(str(tmp_path))
    a.step(**_spark_batch(73))
    torch.manual_seed(6)
    b = trainer.DataParallelTrainer(_spark(seed=2).train(), **OPT)
    b.load_checkpoint(str(tmp_path))
    b.step(**_spark_batch(73))
    _assert_same_state(_state(a), _state(b))
