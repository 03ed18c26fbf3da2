"""CPU: held-out evaluation (rwkv7_head_eval_bf16, losses.fused_linear_eval, the heads' eval_metrics, DataParallelTrainer.evaluate).

The HIP backbone cannot run on the CPU (by design), so the head models here are the real classes at L = 2, D = 128 with `.model`
replaced by a small CPU stand-in (`StubBackbone`): what is under test is everything eval_metrics adds around the backbone -- label
handling, the torch route of fused_linear_eval, normalisation, the mode switch -- against the SAME model's existing eval-mode
forward(..., labels=...) in fp32.  The real backbone on the HIP path is in test_head_eval_gpu.py.

fp32 against fp32 / fp64: the row formulas carry a few fp32 roundings per term; REL = 1e-5 relative is ~100 ulp (test_cosy_head.py)."""
import ctypes
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

from cosy_head_ref import exact_rows
from rwkvtts_amd import _lib, layouts as L, losses, trainer
from rwkvtts_amd.backbone import ModelOutput
from rwkvtts_amd.cosy_llm import RWKV7CosyConfig, RWKV7CosyLM, RWKV7LM
from rwkvtts_amd.spark_llm import RWKV7ForSpeech, RWKV7SpeechConfig
from rwkvtts_amd.xy_llm import RWKV7XYConfig, RWKV7XYLM
from test_trainer_dist import _free_port

REL = 1e-5
SMALL = dict(hidden_size=128, num_hidden_layers=2, decay_low_rank_dim=32, a_low_rank_dim=32, v_low_rank_dim=16, gate_low_rank_dim=32)


# ---- the entry point -------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_and_the_library_exports_it(hip_lib):
    assert "rwkv7_head_eval_bf16" in _lib.exported_symbols()
    restype, argtypes = _lib.prototypes()["rwkv7_head_eval_bf16"]
    assert restype is ctypes.c_int and len(argtypes) == 12
    assert argtypes[:3] == [ctypes.c_long, ctypes.c_int, ctypes.c_long] and argtypes[5:8] == [ctypes.c_long, ctypes.c_int, ctypes.c_float]
    assert hasattr(hip_lib, "rwkv7_head_eval_bf16")


def test_entry_point_rejects_bad_arguments_before_any_launch(hip_lib):
    one = 16   # never dereferenced: the checks fire first

    def call(rows=4, V=11, ld=11, logits=one, labels=one, kind=0, s=0.1, loss=one, correct=one, argmax=None):
        return hip_lib.rwkv7_head_eval_bf16(rows, V, ld, logits, labels, -1, kind, s, loss, correct, argmax, None)

    for name in ("logits", "labels", "loss", "correct"):
        assert call(**{name: None}) == -1, name
    assert call(rows=0) == -1 and call(rows=-3) == -1
    assert call(V=1, ld=1) == -1 and call(V=0) == -1
    assert call(V=11, ld=10) == -1
    assert call(kind=2) == -1 and call(kind=-1) == -1
    for kind in (0, 1):
        for s in (-0.1, 1.0, 1.5, float("nan")):
            assert call(kind=kind, s=s) == -1, (kind, s)


# ---- fused_linear_eval on the CPU ------------------------------------------------------------------------------------------------
def _ce_rows_fp64(x, labels, s, ignore):
    """cross-entropy with label smoothing per row, fp64, written from the formula in include/rwkv7_hip.h"""
    x = x.double()
    valid = labels != ignore
    lse = torch.logsumexp(x, dim=1)
    xy = x.gather(1, labels.clamp(min=0)[:, None])[:, 0]
    return ((1 - s) * (lse - xy) + s * (lse - x.mean(1))) * valid


@pytest.mark.parametrize("kind,s", [(0, 0.0), (0, 0.1), (1, 0.0), (1, 0.1)])
@pytest.mark.parametrize("chunk", [None, 7])
def test_torch_route_against_the_fp64_restatement(kind, s, chunk):
    g = torch.Generator().manual_seed(5)
    B, T, D, V = 2, 9, 16, 23
    h = torch.randn(B, T, D, generator=g)
    lin = nn.Linear(D, V)
    ignore = -100 if kind == 0 else -1
    t = torch.randint(0, V, (B, T), generator=g)
    t[0, :4] = ignore
    logits = lin(h).detach().reshape(-1, V)
    t.view(-1)[5:9] = logits.argmax(1)[5:9]   # some correct rows
    hits = losses.EVAL_HITS[0]
    loss_sum, n_valid, n_correct = losses.fused_linear_eval(h, t, lin.weight, lin.bias, ignore, kind, smoothing=s, chunk=chunk)
    assert losses.EVAL_HITS[0] == hits, "CPU tensors must take the torch route"
    assert (loss_sum.dtype, n_valid.dtype, n_correct.dtype) == (torch.float64, torch.int64, torch.int64)
    assert loss_sum.shape == n_valid.shape == n_correct.shape == (1,) and not loss_sum.requires_grad
    tv = t.reshape(-1)
    want = _ce_rows_fp64(logits, tv, s, ignore) if kind == 0 else exact_rows(logits, tv, s)[0]
    assert abs(loss_sum.item() - want.sum().item()) <= REL * want.sum().item()
    assert n_valid.item() == 14
    assert n_correct.item() == ((logits.argmax(1) == tv) & (tv != ignore)).sum().item() >= 4


def test_fused_linear_eval_rejects_unknown_kind_and_smoothing():
    h, lin, t = torch.randn(3, 8), nn.Linear(8, 5), torch.zeros(3, dtype=torch.long)
    for kind, s in ((2, 0.0), (0, 1.0), (1, -0.1)):
        with pytest.raises(ValueError):
            losses.fused_linear_eval(h, t, lin.weight, lin.bias, -1, kind, smoothing=s)


# ---- the three heads ---------------------------------------------------------------------------------------------------------------
class StubBackbone(nn.Module):
    """CPU stand-in for RWKV7Model: same call and return convention, a causal map of the embeddings."""

    def __init__(self, D, vocab):
        super().__init__()
        self.embeddings = nn.Embedding(vocab, D)
        self.mix = nn.Linear(D, D)

    def forward(self, input_ids=None, attention_mask=None, inputs_embeds=None, past_key_values=None, use_cache=None, **kw):
        x = self.embeddings(input_ids) if inputs_embeds is None else inputs_embeds
        h = torch.tanh(self.mix(x)).cumsum(1) * 0.3
        if attention_mask is not None:
            h = h * attention_mask.unsqueeze(-1).to(h.dtype)
        return ModelOutput(last_hidden_state=h, past_key_values=None)


def _stubbed(model, vocab, seed):
    torch.manual_seed(seed)
    model.model = StubBackbone(128, vocab)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(torch.randn(p.shape) * 0.2)
    return model


def _spark(seed=1):
    cfg = RWKV7SpeechConfig(vocab_size=257, text_vocab_size=300, audio_global_vocab_size=64, **SMALL)
    return _stubbed(RWKV7ForSpeech(cfg), 257, seed)


def _spark_batch(seed, B=2, T=12):
    g = torch.Generator().manual_seed(seed)
    mask = torch.ones(B, T, dtype=torch.long)
    mask[1, :3] = 0
    labels = torch.randint(0, 257, (B, T), generator=g)
    labels[1, :4] = -100
    return dict(inputs_embeds=torch.randn(B, T, 128, generator=g) * 0.5, attention_mask=mask, labels=labels)


def _close(a, b):
    return abs(float(a) - float(b)) <= REL * abs(float(b))


def test_spark_eval_metrics_equals_the_eval_mode_forward():
    m = _spark().train()
    batch = _spark_batch(3)
    got = m.eval_metrics(**batch)
    assert m.training and m.dropout.training, "the previous mode must be restored"
    assert m.eval_metrics(**batch)["loss_sum"].item() == got["loss_sum"].item(), "no dropout: two calls agree exactly"
    m.eval()
    with torch.no_grad():
        out = m(**batch)
    assert m.eval_metrics(**batch)["loss"].item() == got["loss"].item() and not m.training
    shifted = torch.cat((batch["labels"][:, 1:], torch.full((2, 1), -100)), 1)
    valid = shifted != -100
    assert _close(got["loss"], out.loss)
    assert got["tokens"].item() == valid.sum().item() == 2 * 11 - 3
    assert got["correct"].item() == ((out.logits.argmax(-1) == shifted) & valid).sum().item()
    assert got["loss_sum"].shape == got["tokens"].shape == got["correct"].shape == (1,)
    assert _close(got["loss_sum"].item() / got["tokens"].item(), out.loss)


def test_xy_eval_metrics_equals_the_eval_mode_forward():
    cfg = RWKV7XYConfig(vocab_size=120, speech_vocab_size=16, num_channels=4, text_shift_size=100, lsm_weight=0.1, drop_ratio=0.1, **SMALL)
    m = _stubbed(RWKV7XYLM(cfg), 120, 2).train()
    g = torch.Generator().manual_seed(4)
    B, T = 2, 10
    ids = torch.cat([torch.randint(0, 120, (B, T, 1), generator=g), torch.randint(0, 16, (B, T, 3), generator=g)], 2)
    labels = torch.cat([torch.randint(0, 120, (B, T, 1), generator=g), torch.randint(0, 16, (B, T, 3), generator=g)], 2)
    labels[0, :3, :] = -100
    labels[1, 5:, 2] = -100
    got = m.eval_metrics(input_ids=ids, labels=labels)
    assert m.training and m.dropout.training
    m.eval()
    with torch.no_grad():
        out = m(input_ids=ids, labels=labels)
    assert _close(got["loss"], out.loss)
    assert got["loss_sum"].shape == got["tokens"].shape == got["correct"].shape == (4,)
    assert got["tokens"].tolist() == [(labels[:, :, c] != -100).sum().item() for c in range(4)] == [17, 17, 12, 17]
    want = [((out.logits[c].argmax(-1) == labels[:, :, c]) & (labels[:, :, c] != -100)).sum().item() for c in range(4)]
    assert got["correct"].tolist() == want
    assert _close((got["loss_sum"] / got["tokens"]).sum(), out.loss)


def _cosy_batch():
    # unequal lengths; 10 + 1 and 3 + 1 valid targets: 15
    return L.cosy_collate([[3, 4, 5, 6], [7, 8]], [list(range(10, 20)), [20, 21, 22]], pad_to_max_length=False)


@pytest.mark.parametrize("nl", [True, False])
def test_cosy_eval_metrics_equals_the_eval_mode_forward_and_th_accuracy(nl):
    cfg = RWKV7CosyConfig(vocab_size=200, speech_token_size=50, lsm_weight=0.1, length_normalized_loss=nl, drop_ratio=0.1, **SMALL)
    llm = _stubbed(RWKV7CosyLM(cfg), 200, 3).train()
    batch = _cosy_batch()
    got = llm.eval_metrics(batch=batch)
    assert llm.training and llm.dropout.training
    llm.eval()
    with torch.no_grad():
        out = llm(batch=batch)
        labels = llm.build_inputs(batch)[2]
    assert _close(got["loss"], out.loss)
    assert got["tokens"].item() == 15 and got["denom"].item() == (15 if nl else 2)
    acc = losses.th_accuracy(out.logits.reshape(-1, 51), labels, -1)
    assert abs(got["correct"].item() / 15 - acc.item()) < 1e-7
    # the wrapper: its own embeddings, the same head
    torch.manual_seed(9)
    w = RWKV7LM(128, 128, 50, llm, lsm_weight=0.1, length_normalized_loss=nl, drop_ratio=0.1).train()
    gw = w.eval_metrics(batch)
    assert w.training and w.dropout.training
    w.eval()
    with torch.no_grad():
        r = w(batch)
    assert _close(gw["loss"], r["loss"]) and abs(gw["correct"].item() / gw["tokens"].item() - r["acc"].item()) < 1e-7


# ---- DataParallelTrainer.evaluate --------------------------------------------------------------------------------------------------
LR = dict(lr=1e-2, warmup_steps=0, total_steps=100)


def _state(tr):
    r = tr.reducer
    return dict(param=tr.flat.flat_param.clone(), master=tr.master.clone(), exp_avg=tr.exp_avg.clone(), exp_avg_sq=tr.exp_avg_sq.clone(),
                grad=tr.flat.flat_grad.clone(), nan_flag=tr.nan_flag.clone(), step_idx=tr.step_idx, last_lr=tr.last_lr, lr=tr.current_lr(),
                reducer=(list(r.ready_order), r.rebuilt, [list(b) for b in r.buckets], len(r.works), list(r.launched), list(r.summed)),
                rng=torch.get_rng_state().clone(), training=tr.model.training)


def _assert_same_state(a, b):
    for k, v in a.items():
        assert torch.equal(v, b[k]) if torch.is_tensor(v) else v == b[k], k


def _steps(tr, rank, steps):
    for s in steps:
        tr.step(**_spark_batch(100 * s + rank))


def _shard(rank):
    return [_spark_batch(1000 + 10 * rank + i, T=8 + i) for i in range(2)]


def test_evaluate_one_rank_values_and_nothing_moves():
    torch.manual_seed(11)
    tr = trainer.DataParallelTrainer(_spark().train(), **LR)
    _steps(tr, 0, range(2))
    batches = _shard(0) + _shard(1)
    before, digest = _state(tr), tr.digest()
    res = tr.evaluate(iter(batches))
    _assert_same_state(before, _state(tr))
    assert tr.digest() == digest
    per = [tr.model.eval_metrics(**b) for b in batches]
    tokens = sum(p["tokens"].item() for p in per)
    assert res["tokens"] == tokens and isinstance(res["tokens"], int) and isinstance(res["loss"], float)
    assert _close(res["loss"], sum(p["loss_sum"].item() for p in per) / tokens)
    assert res["accuracy"] == sum(p["correct"].item() for p in per) / tokens
    assert "per_channel" not in res
    with pytest.raises(ValueError):
        tr.evaluate([])


def test_three_steps_evaluate_two_steps_equals_five_steps_with_dropout_on():
    def run(evaluate):
        torch.manual_seed(12)
        m = _spark().train()
        assert m.dropout.p == 0.02
        tr = trainer.DataParallelTrainer(m, **LR)
        _steps(tr, 0, range(3))
        if evaluate:
            tr.evaluate(_shard(0))
        _steps(tr, 0, range(3, 5))
        return _state(tr)

    a, b = run(False), run(True)
    _assert_same_state(a, b)
    torch.manual_seed(12)   # the case means something only if dropout draws: another seed gives other parameters
    m = _spark().train()
    torch.manual_seed(13)
    tr = trainer.DataParallelTrainer(m, **LR)
    _steps(tr, 0, range(5))
    assert not torch.equal(tr.flat.flat_param, a["param"])


def test_evaluate_inside_an_accumulation_window_raises():
    tr = trainer.DataParallelTrainer(_spark().train(), **LR)
    tr.accumulate(**_spark_batch(1))
    with pytest.raises(RuntimeError, match="accumulation window"):
        tr.evaluate(_shard(0))
    tr.step(**_spark_batch(2))
    assert tr.evaluate(_shard(0))["tokens"] > 0


def test_evaluate_reports_per_channel_lists_for_xy():
    cfg = RWKV7XYConfig(vocab_size=120, speech_vocab_size=16, num_channels=4, text_shift_size=100, lsm_weight=0.1, **SMALL)
    m = _stubbed(RWKV7XYLM(cfg), 120, 2).train()
    g = torch.Generator().manual_seed(4)
    ids = torch.cat([torch.randint(0, 120, (2, 10, 1), generator=g), torch.randint(0, 16, (2, 10, 3), generator=g)], 2)
    labels = ids.roll(1, 1).clone()
    labels[0, :3, :] = -100
    tr = trainer.DataParallelTrainer(m, **LR)
    res = tr.evaluate([dict(input_ids=ids, labels=labels)] * 2)
    one = m.eval_metrics(input_ids=ids, labels=labels)
    assert res["per_channel"]["tokens"] == [2 * t for t in one["tokens"].tolist()] and res["tokens"] == 2 * one["tokens"].sum().item()
    assert all(_close(a, b) for a, b in zip(res["per_channel"]["loss"], (one["loss_sum"] / one["tokens"]).tolist()))
    assert _close(res["loss"], one["loss"]) and _close(sum(res["per_channel"]["loss"]), res["loss"])
    assert res["per_channel"]["accuracy"] == [c / t for c, t in zip(one["correct"].tolist(), one["tokens"].tolist())]


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    trainer.init_distributed("gloo")
    torch.set_num_threads(1)
    torch.manual_seed(20 + rank)
    ta = trainer.DataParallelTrainer(_spark().train(), bucket_bytes=4096, **LR)
    fresh = ta.evaluate(_shard(rank))            # before any step: the parent holds the same model
    _steps(ta, rank, range(3))
    before, digest = _state(ta), ta.digest(all_ranks=True)
    ta.evaluate(_shard(rank))
    untouched = True
    try:
        _assert_same_state(before, _state(ta))
    except AssertionError:
        untouched = False
    untouched = untouched and ta.digest(all_ranks=True) == digest
    _steps(ta, rank, range(3, 5))
    torch.manual_seed(20 + rank)
    tb = trainer.DataParallelTrainer(_spark().train(), bucket_bytes=4096, **LR)
    _steps(tb, rank, range(5))
    same = all(torch.equal(getattr(ta, n), getattr(tb, n)) for n in ("master", "exp_avg", "exp_avg_sq")) \
        and torch.equal(ta.flat.flat_param, tb.flat.flat_param)
    q.put((rank, fresh, untouched, same))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_evaluate_the_union_of_the_shards_and_nothing_moves():
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
    assert res[0][1] == res[1][1], "every rank returns the global values"
    assert all(r[2] for r in res), "evaluate moved trainer state, the digest or the RNG on some rank"
    assert all(r[3] for r in res), "3 steps + evaluate + 2 steps differs from 5 steps"
    single = trainer.DataParallelTrainer(_spark().train(), **LR).evaluate(_shard(0) + _shard(1))
    got = res[0][1]
    assert got["tokens"] == single["tokens"] and got["accuracy"] == single["accuracy"]
    assert abs(got["loss"] - single["loss"]) <= 1e-12 * abs(single["loss"])   # fp64 sums in another order
