"""CPU: per-utterance scores (losses.fused_linear_score on its torch route, the four heads' score, DataParallelTrainer.score).

The sequences are score_fixture's.  What a sequence's values are compared against:
  * the row losses of the head are losses._eval_rows_torch's (the definition fused_linear_eval already uses); they are first held to
    F.cross_entropy(reduction='none') / the F.kl_div chain on the same fp32 logits within REL = 1e-5 relative (~100 fp32 ulp, the
    bar of test_head_eval.py), and the per-sequence sums built from THOSE rows must agree with loss_sum within REL sum|rows|, the
    maximum within REL (a maximum is 1-Lipschitz in its terms), the counts exactly;
  * the aggregation itself is then exact: against score_fixture.reference on the function's own fp32 rows, tokens / correct /
    worst_row are equal, worst_loss is bit-equal to the maximum of the rows, loss_sum is within n 2^-52 sum|rows| of the row-order sum.
The heads run on test_head_eval's CPU stand-in for the backbone (which has no CPU path); the real one is in test_score_gpu.py."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

import score_fixture as SF
from cosy_head_ref import fp32_chain_rows
from rwkvtts_amd import layouts as L, losses, trainer
from rwkvtts_amd.cosy_llm import RWKV7CosyConfig, RWKV7CosyLM, RWKV7LM
from rwkvtts_amd.xy_llm import RWKV7XYConfig, RWKV7XYLM
from test_head_eval import LR, SMALL, _assert_same_state, _cosy_batch, _spark, _spark_batch, _state, _steps, _stubbed
from test_trainer_dist import _free_port

REL = 1e-5
D = 16
KINDS = [(losses.EVAL_CE, 0.0, -100), (losses.EVAL_CE, 0.1, -100), (losses.EVAL_KL, 0.1, -1)]


@functools.lru_cache(maxsize=None)
def _case(V, kind, s, ignore):
    """One set of the fixture for a head of width V: (hidden, weight, bias, labels, fp32 logits, own rows, own correct, reference)."""
    g = torch.Generator().manual_seed(V + 10 * kind)
    h = torch.randn(SF.SET_ROWS, D, generator=g)
    w = torch.randn(V, D, generator=g) * 0.5
    b = torch.randn(V, generator=g) * 0.1
    lab = SF.labels_for(V, ignore, g)
    logits = F.linear(h, w, b)
    hit = torch.arange(SF.SET_ROWS) % 5 == 0   # a fifth of the valid rows predicted correctly
    lab = torch.where(hit & (lab != ignore), logits.argmax(1), lab)
    rows, ok = losses._eval_rows_torch(logits, lab, ignore, kind, s)
    return h, w, b, lab, logits, rows, ok, SF.reference(SF.seq_start(), rows, ok.int(), lab, ignore)


def _score(h, lab, w, b, ignore, kind, s, st, **kw):
    return dict(zip(losses.SCORE_KEYS, losses.fused_linear_score(h, lab, w, b, ignore, kind, smoothing=s, seq_start=st, **kw)))


# ---- fused_linear_score ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,s,ignore", KINDS)
def test_scores_against_cross_entropy_and_kl_rows(kind, s, ignore):
    h, w, b, lab, logits, rows, ok, _ = _case(SF.V_PADDED, kind, s, ignore)
    valid = lab != ignore
    if kind == losses.EVAL_CE:
        want = F.cross_entropy(logits, lab.clamp(min=0), reduction="none", label_smoothing=s) * valid
    else:
        want = fp32_chain_rows(logits, lab, s, ignore)
    assert bool(((rows - want).abs() <= REL * want.abs()).all()), "the row formula left the fp32 bar"
    hits = losses.SCORE_HITS[0], losses.EVAL_HITS[0]
    got = _score(h, lab, w, b, ignore, kind, s, SF.seq_start())
    assert (losses.SCORE_HITS[0], losses.EVAL_HITS[0]) == hits, "CPU tensors must take the torch route"
    assert all(v.shape == (len(SF.LENS),) and not v.requires_grad for v in got.values())
    ref = SF.reference(SF.seq_start(), want.float(), (logits.argmax(1) == lab).int(), lab, ignore)
    assert torch.equal(got["tokens"], ref["tokens"]) and torch.equal(got["correct"], ref["correct"])
    assert got["tokens"].tolist()[2] == 0 and got["tokens"].tolist()[SF.ALL_IGNORED] == 0 and got["tokens"][0] == 1
    assert got["correct"].sum() > 100
    sum_abs = ref["bar"] / (ref["tokens"].clamp(min=1) * 2.0 ** -52)
    assert bool(((got["loss_sum"] - ref["loss_sum"]).abs() <= REL * sum_abs).all())
    assert bool(((got["worst_loss"] - ref["worst_loss"]).abs() <= REL * ref["worst_loss"].abs()).all())


@pytest.mark.parametrize("kind,s,ignore", KINDS)
def test_one_set_each_sequence_alone_and_33_copies(kind, s, ignore):
    h, w, b, lab, _, _, _, ref = _case(SF.V_PADDED, kind, s, ignore)
    st = SF.seq_start()
    whole = _score(h, lab, w, b, ignore, kind, s, st)
    SF.assert_scores(whole, ref, "one set")
    for k, v in dict(loss_sum=0.0, tokens=0, correct=0, worst_loss=0.0, worst_row=-1).items():   # the empty and the all-ignored one
        assert whole[k][2] == v and whole[k][SF.ALL_IGNORED] == v, k
    for i in range(len(SF.LENS)):   # n_seq = 1
        alone = _score(h, lab, w, b, ignore, kind, s, st[i:i + 2])
        SF.assert_bit_identical(alone, {k: v[i:i + 1] for k, v in whole.items()}, f"sequence {i} alone")
    many = _score(h.repeat(SF.COPIES, 1), lab.repeat(SF.COPIES), w, b, ignore, kind, s, SF.seq_start(SF.COPIES))
    SF.assert_scores(many, {k: v.repeat(SF.COPIES) for k, v in ref.items()}, "33 copies")


def test_a_head_of_8193_classes():
    kind, s, ignore = losses.EVAL_CE, 0.1, -100
    h, w, b, lab, _, _, _, ref = _case(SF.V_ODD, kind, s, ignore)
    SF.assert_scores(_score(h, lab, w, b, ignore, kind, s, SF.seq_start()), ref, "V = 8193")
    rows, ok = losses._eval_rows_torch(F.linear(h, w), lab, ignore, kind, s)   # the Spark head has no bias
    SF.assert_scores(_score(h, lab, w, None, ignore, kind, s, SF.seq_start()), SF.reference(SF.seq_start(), rows, ok.int(), lab, ignore),
                     "V = 8193, no bias")


@pytest.mark.parametrize("kind,s,ignore", KINDS[1:])
def test_chunking_changes_no_bit(kind, s, ignore):
    h, w, b, lab, _, _, _, ref = _case(SF.V_PADDED, kind, s, ignore)
    st = SF.seq_start()
    outs = [_score(h, lab, w, b, ignore, kind, s, st, chunk=c) for c in (7, 64, SF.SET_ROWS)]
    SF.assert_scores(outs[0], ref, "chunk 7")
    SF.assert_bit_identical(outs[0], outs[2], "chunk 7 against N")
    SF.assert_bit_identical(outs[1], outs[2], "chunk 64 against N")


def test_the_earlier_of_two_equal_worst_rows_wins():
    kind, s, ignore = losses.EVAL_CE, 0.0, -100
    h, w, b, lab, _, _, _, ref = _case(SF.V_PADDED, kind, s, ignore)
    st = SF.seq_start().tolist()
    h, lab = h.clone(), lab.clone()
    later = {}
    for i in (6, 7):   # the 257- and the 1025-row sequence
        worst = st[i] + int(ref["worst_row"][i])
        # a copy of the worst row (same hidden state, same label: the same loss to the last bit) behind it, and one in front of it
        # in the other sequence
        dup = st[i + 1] - 1 if i == 6 else st[i]
        assert dup != worst and lab[dup] != ignore
        h[dup], lab[dup] = h[worst], lab[worst]
        later[i] = (worst - st[i], dup - st[i])
    got = _score(h, lab, w, b, ignore, kind, s, SF.seq_start(), chunk=64)
    for i, (worst, dup) in later.items():
        assert got["worst_row"][i] == min(worst, dup), i
        assert got["worst_loss"][i].view(torch.int32) == ref["worst_loss"][i].view(torch.int32), i
    assert later[6][1] > later[6][0] and later[7][1] < later[7][0], "one duplicate behind and one in front of the original"


def test_seq_start_is_required_and_clamped_to_the_rows():
    kind, s, ignore = losses.EVAL_CE, 0.0, -100
    h, w, b, lab, _, _, _, ref = _case(SF.V_PADDED, kind, s, ignore)
    with pytest.raises(TypeError):
        losses.fused_linear_score(h, lab, w, b, ignore, kind)
    for bad in (None, torch.zeros(1, dtype=torch.int64), torch.zeros(2, 2, dtype=torch.int64)):
        with pytest.raises(ValueError):
            losses.fused_linear_score(h, lab, w, b, ignore, kind, seq_start=bad)
    with pytest.raises(ValueError):
        losses.fused_linear_score(h, lab, w, b, ignore, 2, seq_start=SF.seq_start())
    st = SF.seq_start()
    far = _score(h, lab, w, b, ignore, kind, s, torch.tensor([-5, st[1], st[2], 10 ** 9]))   # the last sequence: every other row
    assert far["tokens"].tolist() == [1, ref["tokens"][1].item(), ref["tokens"][2:].sum().item()]


# ---- the heads ---------------------------------------------------------------------------------------------------------------------
def _sums_match(score, metrics, channels=None):
    """tokens and correct summed over the utterances equal eval_metrics' counts; loss_sum within n 2^-52 |loss_sum| (the head's row
    losses are positive, so |loss_sum| is sum|rows| and this is the fixture's bar)."""
    assert set(score) == set(losses.SCORE_KEYS)
    tokens, correct, loss_sum = score["tokens"].sum(-1), score["correct"].sum(-1), score["loss_sum"].sum(-1)
    assert torch.equal(tokens.reshape(-1), metrics["tokens"]) and torch.equal(correct.reshape(-1), metrics["correct"])
    bar = metrics["tokens"] * 2.0 ** -52 * metrics["loss_sum"].abs()
    assert bool(((loss_sum.reshape(-1) - metrics["loss_sum"]).abs() <= bar).all())
    assert bool((score["worst_loss"] * score["tokens"] >= score["loss_sum"] * (1 - 1e-6)).all()), "the maximum is below the mean"
    assert bool(((score["worst_row"] >= 0) == (score["tokens"] > 0)).all())


def test_spark_score_padded():
    m = _spark().train()
    batch = _spark_batch(3)
    got = m.score(**batch)
    assert m.training and m.dropout.training, "the previous mode must be restored"
    assert all(v.shape == (2,) for v in got.values())
    _sums_match(got, m.eval_metrics(**batch))
    shifted = torch.cat((batch["labels"][:, 1:], torch.full((2, 1), -100)), 1)
    assert got["tokens"].tolist() == (shifted != -100).sum(1).tolist() == [11, 8]
    m.eval()
    with torch.no_grad():
        rows = F.cross_entropy(m(**batch).logits.reshape(24, -1), shifted.reshape(-1), reduction="none", ignore_index=-100).reshape(2, 12)
    assert bool(((got["loss_sum"] - rows.double().sum(1)).abs() <= REL * rows.double().sum(1)).all())
    assert got["worst_row"].tolist() == rows.argmax(1).tolist()
    assert not m.training and all(v.shape == (2,) for v in m.score(**batch).values())


def test_spark_score_packed_cu_seqlens():
    m = _spark().train()
    g = torch.Generator().manual_seed(8)
    cu = torch.tensor([0, 5, 5, 18, 26])   # four utterances, one empty; two rows behind cu_seqlens[-1]
    labels = torch.randint(0, 257, (1, 28), generator=g)
    labels[0, [4, 17, 25]] = -100          # what the builder leaves at the end of an utterance
    batch = dict(inputs_embeds=torch.randn(1, 28, 128, generator=g) * 0.5, labels=labels, cu_seqlens=cu)
    got = m.score(**batch)
    assert all(v.shape == (4,) for v in got.values())
    _sums_match(got, m.eval_metrics(**batch))
    shifted = torch.cat((labels[0, 1:], torch.tensor([-100])))
    want = [int((shifted[a:b] != -100).sum()) for a, b in zip(cu[:-1].tolist(), cu[1:].tolist())]
    assert got["tokens"].tolist() == want and want[1] == 0 and got["worst_row"][1] == -1
    m.config.strict_reference_loss = True   # eval_metrics then counts the rows behind cu_seqlens[-1]: they are one more utterance
    strict = m.score(**batch)
    assert all(v.shape == (5,) for v in strict.values()) and strict["tokens"][4] == 1
    _sums_match(strict, m.eval_metrics(**batch))


def test_xy_score_stacks_the_channels():
    cfg = RWKV7XYConfig(vocab_size=120, speech_vocab_size=16, num_channels=4, text_shift_size=100, lsm_weight=0.1, drop_ratio=0.1, **SMALL)
    m = _stubbed(RWKV7XYLM(cfg), 120, 2).train()
    g = torch.Generator().manual_seed(4)
    B, T = 3, 10
    ids = torch.cat([torch.randint(0, 120, (B, T, 1), generator=g), torch.randint(0, 16, (B, T, 3), generator=g)], 2)
    labels = torch.cat([torch.randint(0, 120, (B, T, 1), generator=g), torch.randint(0, 16, (B, T, 3), generator=g)], 2)
    labels[0, :3, :] = -100
    labels[1, :, 2] = -100   # utterance 1 has nothing to score on channel 2
    got = m.score(input_ids=ids, labels=labels)
    assert m.training and all(v.shape == (4, B) for v in got.values())
    _sums_match(got, m.eval_metrics(input_ids=ids, labels=labels))   # per channel
    assert got["tokens"].tolist() == [[7, 10, 10], [7, 10, 10], [7, 0, 10], [7, 10, 10]]
    assert got["worst_row"][2, 1] == -1 and bool((got["worst_row"][:, 0] >= 3).all())


@pytest.mark.parametrize("nl", [True, False])
def test_cosy_score_one_sequence_per_utterance(nl):
    cfg = RWKV7CosyConfig(vocab_size=200, speech_token_size=50, lsm_weight=0.1, length_normalized_loss=nl, drop_ratio=0.1, **SMALL)
    llm = _stubbed(RWKV7CosyLM(cfg), 200, 3).train()
    batch = _cosy_batch()
    got = llm.score(batch=batch)
    assert llm.training and got["tokens"].tolist() == [11, 4]
    _sums_match(got, llm.eval_metrics(batch=batch))
    torch.manual_seed(9)
    w = RWKV7LM(128, 128, 50, llm, lsm_weight=0.1, length_normalized_loss=nl, drop_ratio=0.1).train()
    gw = w.score(batch)
    assert w.training and gw["tokens"].tolist() == [11, 4]
    _sums_match(gw, w.eval_metrics(batch))


# ---- DataParallelTrainer.score -----------------------------------------------------------------------------------------------------
def _shard(rank):
    return [_spark_batch(1000 + 10 * rank + i, T=8 + i) for i in range(2)]


def test_trainer_score_values_order_and_nothing_moves():
    torch.manual_seed(11)
    tr = trainer.DataParallelTrainer(_spark().train(), **LR)
    _steps(tr, 0, range(2))
    batches = _shard(0) + _shard(1)
    before, digest = _state(tr), tr.digest()
    res = tr.score(iter(batches))
    _assert_same_state(before, _state(tr))
    assert tr.digest() == digest and tr.model.training
    per = [tr.model.score(**b) for b in batches]
    assert set(res) == set(losses.SCORE_KEYS) | {"mean_loss"}
    for k in losses.SCORE_KEYS:
        want = torch.cat([p[k] for p in per]).numpy()
        assert isinstance(res[k], np.ndarray) and res[k].dtype == want.dtype and res[k].shape == (8,) and np.array_equal(res[k], want), k
    assert np.array_equal(res["mean_loss"], res["loss_sum"] / np.maximum(res["tokens"], 1)) and res["mean_loss"].dtype == np.float64
    ev = tr.evaluate(batches)
    assert res["tokens"].sum() == ev["tokens"] and abs(res["loss_sum"].sum() / ev["tokens"] - ev["loss"]) <= 1e-12 * ev["loss"]
    with pytest.raises(ValueError):
        tr.score([])


def test_three_steps_score_two_steps_equals_five_steps_with_dropout_on():
    def run(score):
        torch.manual_seed(12)
        m = _spark().train()
        assert m.dropout.p == 0.02
        tr = trainer.DataParallelTrainer(m, **LR)
        _steps(tr, 0, range(3))
        if score:
            tr.score(_shard(0))
            assert tr.model.training and tr.model.dropout.training
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


def test_score_inside_an_accumulation_window_raises():
    tr = trainer.DataParallelTrainer(_spark().train(), **LR)
    tr.accumulate(**_spark_batch(1))
    with pytest.raises(RuntimeError, match="accumulation window"):
        tr.score(_shard(0))
    tr.step(**_spark_batch(2))
    assert tr.score(_shard(0))["tokens"].sum() > 0 and tr.model.training


def test_trainer_score_of_a_multi_channel_head_keeps_the_channel_axis():
    cfg = RWKV7XYConfig(vocab_size=120, speech_vocab_size=16, num_channels=4, text_shift_size=100, lsm_weight=0.1, **SMALL)
    m = _stubbed(RWKV7XYLM(cfg), 120, 2).train()
    g = torch.Generator().manual_seed(4)
    ids = torch.cat([torch.randint(0, 120, (2, 10, 1), generator=g), torch.randint(0, 16, (2, 10, 3), generator=g)], 2)
    labels = ids.roll(1, 1).clone()
    labels[0, :3, :] = -100
    res = trainer.DataParallelTrainer(m, **LR).score([dict(input_ids=ids, labels=labels)] * 2)
    one = m.score(input_ids=ids, labels=labels)
    assert res["tokens"].shape == (4, 4) and np.array_equal(res["loss_sum"], torch.cat([one["loss_sum"]] * 2, 1).numpy())


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    trainer.init_distributed("gloo")
    torch.set_num_threads(1)
    torch.manual_seed(20 + rank)
    ta = trainer.DataParallelTrainer(_spark().train(), bucket_bytes=4096, **LR)
    fresh = ta.score(_shard(rank))               # before any step: the parent holds the same model
    _steps(ta, rank, range(3))
    before, digest = _state(ta), ta.digest(all_ranks=True)
    ta.score(_shard(rank) if rank == 0 else _shard(rank)[:1])   # no collective: the ranks need not submit the same number of batches
    untouched = ta.model.training
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
def test_two_ranks_score_their_own_batches_and_nothing_moves():
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
    assert all(r[2] for r in res), "score moved trainer state, the digest, the RNG or the mode on some rank"
    assert all(r[3] for r in res), "3 steps + score + 2 steps differs from 5 steps"
    single = trainer.DataParallelTrainer(_spark().train(), **LR)
    for rank in range(world):   # every rank got the scores of its own batches, nothing of the other's
        want = single.score(_shard(rank))
        assert all(np.array_equal(res[rank][1][k], want[k]) for k in want), rank
