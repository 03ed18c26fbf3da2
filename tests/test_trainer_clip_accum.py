"""CPU: gradient clipping by global norm and fp32 micro-batch accumulation in rwkvtts_amd/trainer.py, on the toy fp32 network of
test_trainer_dist.py (the torch fallback of the trainer: the scheduling -- when the fold runs, what the reducer sees, which flag
is reduced -- is the same code as on the GPU, only the four passes are torch instead of HIP).

References: torch.optim.AdamW + torch.nn.utils.clip_grad_norm_ on a twin (what third_party/cosyvoice/utils/train_utils.py:283-291
does), and one step on the concatenated batch for accumulation (`accum_grad`, train_utils.py:87-89).  Bars: those of
test_trainer_dist.py for the same comparisons (allclose atol 1e-6 / 2e-6 with rtol 1e-5)."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from rwkvtts_amd import trainer
from test_trainer_dist import Toy, _data, _free_port

LR = dict(lr=1e-2, warmup_steps=0, total_steps=100)


def _flat(model):
    return torch.cat([torch.nn.functional.pad(p.detach().reshape(-1), (0, (-p.numel()) % 128)) for p in model.parameters()])


def _twin_step(model, opt, step, batches, max_norm=None):
    """One torch.optim.AdamW step of `model` on the mean loss of `batches`; returns clip_grad_norm_'s norm (None without)."""
    opt.zero_grad()
    loss = sum(model(x, y).loss for x, y in batches) / len(batches)
    loss.backward()
    model.unused.grad = torch.zeros_like(model.unused)
    norm = None
    if max_norm is not None:
        norm = torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)
    for g_ in opt.param_groups:
        g_["lr"] = trainer.linear_warmup_decay(step, 100, 0, 1e-2, 1e-5)
    opt.step()
    return norm


def _adamw(model):
    return torch.optim.AdamW(model.parameters(), lr=1e-2, betas=(0.9, 0.95), eps=1e-18, weight_decay=0.0)


def test_clipped_steps_equal_torch_adamw_with_clip_grad_norm():
    m1, m2 = Toy(), Toy()
    x, y = _data(0, 0)
    m2(x, y).loss.backward()
    observed = torch.sqrt(sum(p.grad.double().pow(2).sum() for p in m2.parameters() if p.grad is not None)).item()
    max_norm = 0.5 * observed            # below the observed norm: the clip is active
    m2 = Toy()
    tr = trainer.DataParallelTrainer(m1, max_grad_norm=max_norm, **LR)
    opt = _adamw(m2)
    for step in range(3):
        x, y = _data(0, step)
        tr.step(x=x, y=y)
        norm = _twin_step(m2, opt, step, [(x, y)], max_norm)
        assert norm.item() > max_norm, "the case must clip"
        assert tr.last_grad_norm.shape == () and tr.last_grad_norm.dtype == torch.float32
        assert torch.allclose(tr.last_grad_norm, norm, rtol=1e-5, atol=1e-6), (step, tr.last_grad_norm, norm)
        for (n, a), b in zip(m1.named_parameters(), m2.parameters()):
            assert torch.allclose(a, b, atol=2e-6, rtol=1e-5), (step, n, (a - b).abs().max())
    # measure only: the norm is reported, the update is the unclipped one
    m3, m4 = Toy(), Toy()
    t3 = trainer.DataParallelTrainer(m3, max_grad_norm=float("inf"), **LR)
    t4 = trainer.DataParallelTrainer(m4, **LR)
    assert t4.last_grad_norm is None
    x, y = _data(0, 0)
    t3.step(x=x, y=y)
    t4.step(x=x, y=y)
    assert torch.equal(t3.flat.flat_param, t4.flat.flat_param)
    assert abs(t3.last_grad_norm.item() - observed) <= 1e-5 * observed


def test_three_micro_batches_equal_one_step_on_the_concatenated_batch():
    m1, m2 = Toy(), Toy()
    tr = trainer.DataParallelTrainer(m1, **LR)
    ref = trainer.DataParallelTrainer(m2, **LR)
    for step in range(2):
        mbs = [_data(k, step) for k in range(3)]
        assert tr._acc_count == 0
        losses = [tr.accumulate(x=mbs[0][0], y=mbs[0][1]), tr.accumulate(x=mbs[1][0], y=mbs[1][1])]
        assert tr._acc_count == 2 and tr.step_idx == step, "accumulate() must not step"
        losses.append(tr.step(x=mbs[2][0], y=mbs[2][1]))
        l = ref.step(x=torch.cat([b[0] for b in mbs]), y=torch.cat([b[1] for b in mbs]))
        assert torch.allclose(sum(losses) / 3, l, atol=1e-6)
        assert tr._acc_count == 0 and tr.step_idx == step + 1
        assert torch.allclose(tr.flat.flat_grad, ref.flat.flat_grad, atol=1e-6), (tr.flat.flat_grad - ref.flat.flat_grad).abs().max()
        assert torch.allclose(tr.flat.flat_param, ref.flat.flat_param, atol=1e-6), step
    # a plain step afterwards runs today's path again: same update as the reference trainer
    x, y = _data(0, 5)
    tr.step(x=x, y=y)
    ref.step(x=x, y=y)
    assert torch.allclose(tr.flat.flat_param, ref.flat.flat_param, atol=1e-6)


@pytest.mark.parametrize("clip", [False, True])
def test_nan_loss_in_the_middle_micro_batch_makes_a_zero_gradient_step_and_clears_the_accumulator(clip):
    kw = dict(max_grad_norm=1.0) if clip else {}
    m1, m2 = Toy(), Toy()
    tr = trainer.DataParallelTrainer(m1, **LR, **kw)
    ref = trainer.DataParallelTrainer(m2, **LR, **kw)
    x, y = _data(0, 0)
    tr.step(x=x, y=y)
    ref.step(x=x, y=y)                    # moments are non-zero: a zero-gradient step moves the parameters
    mbs = [_data(k, 1) for k in range(3)]
    tr.accumulate(x=mbs[0][0], y=mbs[0][1])
    ln = tr.accumulate(x=mbs[1][0], y=mbs[1][1], poison=True)
    assert not torch.isfinite(ln)
    tr.step(x=mbs[2][0], y=mbs[2][1])
    ref.step(x=x, y=y, poison=True)       # what a zero-gradient step does today
    assert torch.isfinite(tr.flat.flat_param).all() and torch.isfinite(tr.exp_avg).all() and torch.isfinite(tr.exp_avg_sq).all()
    assert torch.equal(tr.flat.flat_param, ref.flat.flat_param)
    assert torch.equal(tr.exp_avg, ref.exp_avg) and torch.equal(tr.exp_avg_sq, ref.exp_avg_sq)
    assert tr._acc_count == 0
    # the accumulator and the flag are clear: the next window is a clean mean of its own micro-batches
    mbs = [_data(k, 2) for k in range(2)]
    tr.accumulate(x=mbs[0][0], y=mbs[0][1])
    tr.step(x=mbs[1][0], y=mbs[1][1])
    ref.step(x=torch.cat([b[0] for b in mbs]), y=torch.cat([b[1] for b in mbs]))
    assert torch.allclose(tr.flat.flat_param, ref.flat.flat_param, atol=1e-6)


def test_accumulate_leaves_the_reducer_as_if_the_pass_had_not_happened():
    """One rank over gloo with the collectives forced on: an accumulate() before the very first step() must neither record the
    gradient-ready order nor count down the buckets, and the fold runs once per run of every bucket, before its exchange."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        m1, m2 = Toy(), Toy()
        tr = trainer.DataParallelTrainer(m1, bucket_bytes=4096, force_allreduce=True, **LR)
        ref = trainer.DataParallelTrainer(m2, **LR)
        r = tr.reducer
        assert r.enabled and len(r.buckets) > 2
        pending = list(r.pending)
        a, b = _data(0, 0), _data(1, 0)
        tr.accumulate(x=a[0], y=a[1])
        assert r.ready_order == [] and not r.rebuilt and r.pending == pending and r.next_bucket == 0 and not r.works
        assert tr.flat.on_ready == r._ready
        folded, sent = [], []
        fold, exch = tr._fold, r._exchange
        tr._fold = lambda lo, hi, inv: (folded.append((lo, hi, inv)), fold(lo, hi, inv))
        r._exchange = lambda s, e, b=-1: (sent.append((s, e)), exch(s, e, b))
        runs = [x_ for rs in r.runs for x_ in rs]
        tr.step(x=b[0], y=b[1])
        assert [(lo, hi) for lo, hi, _ in folded] == sent and sorted(sent) == sorted(runs) and all(i == 0.5 for _, _, i in folded)
        assert r.rebuilt and r.pre_exchange is None
        ref.step(x=torch.cat([a[0], b[0]]), y=torch.cat([a[1], b[1]]))
        assert torch.allclose(tr.flat.flat_param, ref.flat.flat_param, atol=1e-6)
        folded.clear()
        tr.step(x=a[0], y=a[1])          # no accumulate before it: no fold
        assert folded == []
    finally:
        dist.destroy_process_group()


def _worker(rank, world, port, q, shard):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    trainer.init_distributed("gloo")
    torch.set_num_threads(1)
    model = Toy()
    tr = trainer.DataParallelTrainer(model, bucket_bytes=4096, shard_optimizer=shard, max_grad_norm=MAX_NORM, **LR)
    norms = []
    for step in range(3):
        a, b = _data(rank, 10 + step), _data(rank, 20 + step)
        tr.accumulate(x=a[0], y=a[1])
        tr.step(x=b[0], y=b[1])
        norms.append(tr.last_grad_norm.item())
    # a NaN micro-batch on ONE rank: the running max travels in the flag all-reduce, both ranks take the zero-gradient step
    before = tr.flat.flat_param.clone()
    a, b = _data(rank, 13), _data(rank, 23)
    tr.accumulate(x=a[0], y=a[1], poison=(rank == 1))
    tr.step(x=b[0], y=b[1])
    q.put((rank, tr.flat.flat_param.numpy().copy(), before.numpy().copy(), norms))
    dist.barrier()
    dist.destroy_process_group()


MAX_NORM = 0.5


@pytest.mark.timeout(300)
@pytest.mark.parametrize("shard", [False, True])
def test_two_ranks_with_clipping_and_accumulation_match_the_single_process_mean(shard):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, shard)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert all(torch.equal(torch.from_numpy(res[0][1]), torch.from_numpy(r[1])) for r in res), "replicas diverged"
    assert all(torch.equal(torch.from_numpy(res[0][2]), torch.from_numpy(r[2])) for r in res), "replicas diverged"
    assert all(r[3] == res[0][3] for r in res), "the ranks report different norms"
    model = Toy()
    opt = _adamw(model)
    for step in range(3):
        batches = [_data(r, 10 + step) for r in range(world)] + [_data(r, 20 + step) for r in range(world)]
        norm = _twin_step(model, opt, step, batches, MAX_NORM)
        assert norm.item() > MAX_NORM, "the case must clip"
        assert abs(res[0][3][step] - norm.item()) <= 1e-5 * norm.item() + 1e-6, (step, res[0][3][step], norm.item())
    before, after = torch.from_numpy(res[0][2]), torch.from_numpy(res[0][1])
    assert torch.allclose(_flat(model), before, atol=1e-6), (_flat(model) - before).abs().max()
    assert torch.isfinite(after).all() and not torch.equal(after, before)
