"""GPU (-m gpu): DataParallelTrainer(max_grad_norm=...) and accumulate() around the 2-layer bf16 Spark model and the batches of
test_trainer_gpu.py (hidden_size 128, B = 2, T = 2048: the smallest shape that takes the in-place split weight gradients), through
the HIP passes of csrc/grad_ops.hip.  That file already relies on run-to-run bit reproducibility of the step; so does this one."""
import ctypes
import math
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_trainer_gpu import _batch, _free_port, _model

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
KW = dict(lr=1e-3, warmup_steps=0, total_steps=10)


def _one_rank_rccl():
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=DEV)


@pytest.fixture(scope="module")
def first_step():
    """One plain step of the plain trainer on batch (0, 0), computed once: its gradient, the float64 norm of it, and the optimizer
    state it leaves.  Read-only for the tests that share it."""
    from rwkvtts_amd import trainer
    m = _model(DEV)
    t = trainer.DataParallelTrainer(m, **KW)
    p0 = t.master.clone()
    t.step(**_batch(m, 0, 0))
    torch.cuda.synchronize()
    g = t.flat.flat_grad.clone()
    # premise of the torch restatement below: the kernels flush fp32 denormals (the library's build flag), torch does not, so a
    # gradient whose scaled square is denormal (|g| < ~1e-18) would be a zero to one side and a full-size Adam step to the other
    nz = g.float().abs()
    nz = nz[nz > 0]
    print(f"first step: {nz.numel()} non-zero gradient elements of {g.numel()}, smallest {nz.min().item():.3e}")
    assert nz.min().item() > 1e-17
    return dict(p0=p0, grad=g, norm=g.double().pow(2).sum().sqrt().item(), master=t.master.clone(), exp_avg=t.exp_avg.clone(),
                exp_avg_sq=t.exp_avg_sq.clone(), param=t.flat.flat_param.clone())


def _adamw_restated(p0, g, lr=1e-3, b1=0.9, b2=0.95, eps=1e-18):
    """The first AdamW step (zero moments, no decay: param_groups=None) on the fp32 gradient g, restated in torch."""
    m = (1 - b1) * g
    v = (1 - b2) * g * g
    p = p0 - (lr / (1 - b1)) * m / (v.sqrt() / math.sqrt(1 - b2) + eps)
    return p, m, v


@pytest.mark.timeout(120)
def test_clip_off_equals_today(first_step):
    """max_grad_norm far above the norm: three steps leave flat_param and flat_grad torch.equal to a trainer without the argument,
    and last_grad_norm is within 1e-5 relative of the float64 norm of flat_grad (the bar of the sum-of-squares kernel's own test;
    the square root halves the relative error)."""
    from rwkvtts_amd import trainer
    m1, m2 = _model(DEV), _model(DEV)
    t1 = trainer.DataParallelTrainer(m1, max_grad_norm=1e30, **KW)
    t2 = trainer.DataParallelTrainer(m2, **KW)
    for step in range(3):
        l1 = t1.step(**_batch(m1, 0, step))
        l2 = t2.step(**_batch(m2, 0, step))
        assert torch.equal(l1, l2)
        want = t1.flat.flat_grad.double().pow(2).sum().sqrt().item()
        got = t1.last_grad_norm.item()
        print(f"step {step}: norm {got!r} float64 {want!r} rel {abs(got - want) / want:.3e}")
        assert t1.last_grad_norm.shape == () and t1.last_grad_norm.dtype == torch.float32 and t1.last_grad_norm.is_cuda
        assert abs(got - want) <= 1e-5 * want
    assert torch.equal(t1.flat.flat_param, t2.flat.flat_param) and torch.equal(t1.flat.flat_grad, t2.flat.flat_grad)
    assert torch.equal(t1.master, t2.master) and torch.equal(t1.exp_avg_sq, t2.exp_avg_sq)
    assert not torch.equal(t2.master, first_step["p0"])


@pytest.mark.timeout(120)
@pytest.mark.parametrize("mode", ["plain", "allreduce", "shard"])
def test_clipping_at_half_the_norm_moves_the_update_as_restated_in_torch(mode, first_step):
    """max_grad_norm = half the first observed norm: master, exp_avg, exp_avg_sq after one step equal the torch restatement of the
    step on flat_grad.float() * coef -- master at 2e-6 * max(1, |want|max), the moments within 3e-5 relative (the bars of the clip
    entry's own test).  allreduce / shard: the same under force_allreduce=True in a one-rank RCCL group (where the clip runs behind
    the bucket exchange, and in shard mode behind the one-element all_reduce of the sum)."""
    from rwkvtts_amd import trainer
    norm = first_step["norm"]
    max_norm = 0.5 * norm
    if mode != "plain":
        _one_rank_rccl()
    try:
        m = _model(DEV)
        kw = {} if mode == "plain" else dict(bucket_bytes=64 << 10, force_allreduce=True, shard_optimizer=(mode == "shard"))
        t = trainer.DataParallelTrainer(m, max_grad_norm=max_norm, **KW, **kw)
        assert t.reducer.enabled == (mode != "plain") and t.shard_optimizer == (mode == "shard")
        t.step(**_batch(m, 0, 0))
        torch.cuda.synchronize()
        assert torch.equal(t.flat.flat_grad, first_step["grad"]), "the gradient buffer itself is left unscaled"
        assert abs(t.last_grad_norm.item() - norm) <= 1e-5 * norm
        coef = max_norm / (norm + 1e-6)
        wp, wm, wv = _adamw_restated(first_step["p0"], first_step["grad"].float() * coef)
        print(f"{mode}: master {(t.master - wp).abs().max().item():.3e}")
        assert (t.master - wp).abs().max().item() <= 2e-6 * max(1.0, wp.abs().max().item())
        assert torch.equal(t.flat.flat_param, t.master.bfloat16())
        assert ((t.exp_avg - wm).abs() <= 3e-5 * wm.abs()).all() and ((t.exp_avg_sq - wv).abs() <= 3e-5 * wv).all()
        assert not torch.equal(t.exp_avg, first_step["exp_avg"]), "the clip did nothing"
    finally:
        if mode != "plain":
            dist.destroy_process_group()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("forced", [False, True], ids=["no-exchange", "per-bucket-fold"])
def test_two_micro_batches_fold_into_the_gradient_of_their_mean(forced):
    """accumulate(a) + step(b): flat_grad after the step is torch.equal to the fold, in torch, of the two gradients obtained from two
    separate armed passes on a twin model, and the parameters equal those of a twin stepped once on that folded gradient.  forced:
    force_allreduce=True in a one-rank RCCL group, so that the fold runs bucket by bucket from the reducer's hook."""
    from rwkvtts_amd import _lib, trainer
    if forced:
        _one_rank_rccl()
    try:
        m1, m2 = _model(DEV), _model(DEV)
        kw = dict(bucket_bytes=64 << 10, force_allreduce=True) if forced else {}
        t1 = trainer.DataParallelTrainer(m1, **KW, **kw)
        t2 = trainer.DataParallelTrainer(m2, **KW)
        grads = []
        for mb in range(2):               # the twin: two armed passes, nothing stepped
            t2.flat.arm()
            m2(**_batch(m2, mb, 0)).loss.backward()
            t2.flat.finish_backward()
            grads.append(t2.flat.flat_grad.clone())
        folded = ((grads[0].float() + grads[1].float()) * 0.5).bfloat16()
        la = t1.accumulate(**_batch(m1, 0, 0))
        assert t1.step_idx == 0 and t1._acc_count == 1 and torch.isfinite(la)
        torch.cuda.synchronize()
        assert torch.equal(t1.flat.flat_grad, grads[0]) and torch.equal(t1._acc32, grads[0].float())
        if forced:
            assert t1.reducer.ready_order == [] and not t1.reducer.works
        t1.step(**_batch(m1, 1, 0))
        torch.cuda.synchronize()
        assert t1._acc_count == 0 and t1.reducer.pre_exchange is None
        assert torch.equal(t1.flat.flat_grad, folded)
        # the twin, stepped once on the folded gradient through the plain optimizer entry
        t2.flat.flat_grad.copy_(folded)
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        f = ctypes.c_float
        rc = _lib.lib().rwkv7_adamw_groups_bf16(
            ctypes.c_long(t2.flat.numel), P(t2.master), P(t2.flat.flat_grad), P(t2.exp_avg), P(t2.exp_avg_sq), P(t2.flat.flat_param),
            P(t2.slab_group), P(t2.group_tab), len(t2.group_defs), P(t2.nan_flag), f(1e-3), f(0.9), f(0.95), f(1e-18), 1,
            ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(t1.flat.flat_param, t2.flat.flat_param) and torch.equal(t1.master, t2.master)
        assert torch.equal(t1.exp_avg, t2.exp_avg) and torch.equal(t1.exp_avg_sq, t2.exp_avg_sq)
    finally:
        if forced:
            dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_nan_loss_in_the_first_of_two_micro_batches_leaves_parameters_unchanged():
    """As test_nan_loss_step_on_the_hip_model_leaves_parameters_unchanged checks it: after the window the moments have decayed as
    for a zero gradient, nothing is NaN, and the next clean window trains."""
    from rwkvtts_amd import trainer
    from rwkvtts_amd.spark_llm import RWKV7ForSpeech, RWKV7SpeechConfig
    cfg = RWKV7SpeechConfig(hidden_size=128, num_hidden_layers=2, vocab_size=257, text_vocab_size=300, audio_global_vocab_size=64,
                            decay_low_rank_dim=32, a_low_rank_dim=32, v_low_rank_dim=16, gate_low_rank_dim=32)
    model = RWKV7ForSpeech(cfg).init_weights(seed=0).to(DEV).to(torch.bfloat16).train()
    tr = trainer.DataParallelTrainer(model, max_grad_norm=1.0, **KW)
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(2, 64, 128, generator=g) * 0.5).to(DEV, torch.bfloat16)
    labels = torch.randint(0, 256, (2, 64), generator=g).to(DEV)
    assert torch.isfinite(tr.step(inputs_embeds=x, labels=labels))
    ea, eq = tr.exp_avg.clone(), tr.exp_avg_sq.clone()
    xn = x.clone()
    xn[0, 5, 7] = float("nan")
    assert not torch.isfinite(tr.accumulate(inputs_embeds=xn, labels=labels))
    assert torch.isfinite(tr.step(inputs_embeds=x, labels=labels))       # the clean micro-batch comes last: the flag is the running max
    assert torch.isfinite(tr.flat.flat_param.float()).all() and torch.isfinite(tr.master).all()
    assert torch.isfinite(tr.exp_avg).all() and torch.isfinite(tr.exp_avg_sq).all()
    b1, b2 = tr.betas
    assert torch.allclose(tr.exp_avg, ea * b1, rtol=1e-6, atol=0) and torch.allclose(tr.exp_avg_sq, eq * b2, rtol=1e-6, atol=0)
    assert not math.isfinite(tr.last_grad_norm.item())
    ea = tr.exp_avg.clone()
    tr.accumulate(inputs_embeds=x, labels=labels)
    assert torch.isfinite(tr.step(inputs_embeds=x, labels=labels))
    assert math.isfinite(tr.last_grad_norm.item()) and torch.isfinite(tr.master).all()
    assert not torch.allclose(tr.exp_avg, ea * b1, rtol=1e-6, atol=0), "the clean window did not train"


def _worker(rank, world, port, q, max_norm):
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    from rwkvtts_amd import trainer
    trainer.init_distributed("gloo")
    torch.cuda.set_device(DEV)
    model = _model(DEV)
    tr = trainer.DataParallelTrainer(model, bucket_bytes=64 << 10, shard_optimizer=True, max_grad_norm=max_norm, **KW)
    norms = []
    for step in range(2):
        tr.step(**_batch(model, rank, step))
        norms.append(tr.last_grad_norm.item())
    torch.cuda.synchronize()
    q.put((rank, tr.flat.flat_param.float().cpu().numpy().copy(), norms))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_sharing_one_gpu_over_gloo_shard_mode_with_clipping(first_step):
    """Two fresh processes on GPU 0, bucket exchange over gloo, shard mode: each rank measures its own slab, the one-element
    all_reduce makes the sum global -- replicas bit-identical, the norms equal on both ranks, and the clip active."""
    max_norm = 0.25 * first_step["norm"]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, max_norm)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=500) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert torch.equal(torch.from_numpy(res[0][1]), torch.from_numpy(res[1][1])), "replicas diverged"
    assert res[0][2] == res[1][2], "the ranks report different norms"
    assert all(math.isfinite(v) and v > max_norm for v in res[0][2])
