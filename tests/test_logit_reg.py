"""CPU: the z-loss and max-logit regularisers of the cross-entropy head (losses.fused_linear_cross_entropy(z_loss, max_logit, stats),
the Spark / XY configs, DataParallelTrainer.last_logit_stats) on the torch route, and the C ABI of
rwkv7_ce_reg_fwd_bwd_bf16.  The kernel itself is in test_logit_reg_gpu.py.

The head models are the real classes with `.model` replaced by test_head_eval's CPU stand-in (the HIP backbone cannot run on the CPU).

fp32 against fp64 autograd: the torch route keeps fp32 logits, so loss and gradients carry a few fp32 roundings per term; REL = 1e-5 of
the largest reference magnitude is ~100 ulp (test_head_eval.py's bar for the same chain)."""
import ctypes
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from rwkvtts_amd import _lib, losses, trainer
from rwkvtts_amd.cosy_llm import RWKV7CosyConfig
from rwkvtts_amd.spark_llm import RWKV7ForSpeech, RWKV7SpeechConfig
from rwkvtts_amd.xy_llm import RWKV7XYConfig, RWKV7XYLM
from test_head_eval import LR, SMALL, _spark_batch, _stubbed
from test_trainer_dist import _free_port

REL = 1e-5
NAME = "rwkv7_ce_reg_fwd_bwd_bf16"
Z, C = 1e-2, 5e-2


def _case(seed=3, N=10, D=16, V=23, bias=True):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(N, D, generator=g, requires_grad=True)
    w = (torch.randn(V, D, generator=g) * 0.5).requires_grad_()
    b = (torch.randn(V, generator=g) * 0.5).requires_grad_() if bias else None
    lab = torch.randint(0, V, (N,), generator=g)
    lab[2] = -100
    lab[7] = -100
    lab[4] = 0
    return h, w, b, lab


def _run(h, w, b, lab, **kw):
    for t in (h, w, b):
        if t is not None:
            t.grad = None
    loss = losses.fused_linear_cross_entropy(h, lab, w, b, -100, **kw)
    loss.backward()
    return loss.detach(), h.grad.clone(), w.grad.clone(), None if b is None else b.grad.clone()


# ---- the entry point -------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_and_the_library_exports_it(hip_lib):
    assert NAME in _lib.exported_symbols() and hasattr(hip_lib, NAME)
    restype, argtypes = _lib.prototypes()[NAME]
    f, l, p = ctypes.c_float, ctypes.c_long, ctypes.c_void_p
    assert restype is ctypes.c_int
    assert argtypes == [l, ctypes.c_int, l, p, p, l, f, p, f, f, f, p, p, p]


def test_entry_point_rejects_bad_arguments_before_any_launch(hip_lib):
    one = 16   # never dereferenced: the checks fire first

    def call(rows=4, V=11, ld=11, logits=one, labels=one, loss=one, ls=0.1, z=0.1, c=0.1, lse=None, mx=None):
        return getattr(hip_lib, NAME)(rows, V, ld, logits, labels, -100, 1.0, loss, ls, z, c, lse, mx, None)

    for name in ("logits", "labels", "loss"):
        assert call(**{name: None}) == -1, name
    assert call(rows=0) == -1 and call(V=0) == -1 and call(V=11, ld=10) == -1
    for bad in (-0.1, float("inf"), float("nan")):
        assert call(z=bad) == -1 and call(c=bad) == -1, bad
    for ls in (-0.1, 1.0, float("nan")):
        assert call(ls=ls) == -1, ls


# ---- 1: the defaults --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("ls", [0.0, 0.1])
def test_default_coefficients_are_bit_identical_to_omitting_them(bias, ls):
    case = _case(bias=bias)
    want = _run(*case, label_smoothing=ls, chunk=4)
    got = _run(*case, label_smoothing=ls, chunk=4, z_loss=0, max_logit=0)
    also = _run(*case, label_smoothing=ls, chunk=4, z_loss=0.0, max_logit=0.0, stats=None)
    for a, b, c in zip(want, got, also):
        assert (a is None and b is None and c is None) or (torch.equal(a, b) and torch.equal(a, c))
    # a stats tensor alone changes no bit of the loss or the gradients either
    seen = _run(*case, label_smoothing=ls, chunk=4, stats=torch.zeros(4))
    for a, b in zip(want, seen):
        assert (a is None and b is None) or torch.equal(a, b)


def test_bad_coefficients_and_stats_raise():
    h, w, b, lab = _case()
    for kw in (dict(z_loss=-1.0), dict(max_logit=-1e-3), dict(z_loss=float("nan")), dict(max_logit=float("inf")),
               dict(stats=torch.zeros(3)), dict(stats=torch.zeros(4, dtype=torch.float64))):
        with pytest.raises(ValueError):
            losses.fused_linear_cross_entropy(h, lab, w, b, -100, **kw)


# ---- 2: against autograd on the materialised fp64 objective ------------------------------------------------------------------------------
def _fp64_objective(h, w, b, lab, ls, z, c):
    """(returned loss, full objective) in fp64 from materialised logits, means over the valid rows: CE (torch's own, with its label
    smoothing) + z lse^2 [+ 0.5 c m^2 in the objective alone]."""
    x = torch.nn.functional.linear(h, w, b)
    valid = lab != -100
    ce = torch.nn.functional.cross_entropy(x, lab, ignore_index=-100, label_smoothing=ls, reduction="sum")
    lse = torch.logsumexp(x, dim=1)
    m = x.max(dim=1).values
    n = valid.sum()
    ret = (ce + z * (lse * lse * valid).sum()) / n
    return ret, ret + 0.5 * c * (m * m * valid).sum() / n


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("ls", [0.0, 0.1])
@pytest.mark.parametrize("chunk", [None, 3])
def test_loss_and_gradients_match_autograd_on_the_fp64_objective(bias, ls, chunk):
    h, w, b, lab = _case(bias=bias)
    loss, dh, dw, db = _run(h, w, b, lab, label_smoothing=ls, chunk=chunk, z_loss=Z, max_logit=C)
    h64, w64 = h.detach().double().requires_grad_(), w.detach().double().requires_grad_()
    b64 = None if b is None else b.detach().double().requires_grad_()
    ret, full = _fp64_objective(h64, w64, b64, lab, ls, Z, C)
    full.backward()
    assert abs(loss.item() - ret.item()) <= REL * abs(ret.item()), "the returned loss is CE + z lse^2"
    assert abs(full.item() - ret.item()) > 100 * REL * abs(ret.item()), "the case means something only if the c term is visible"
    for got, want in ((dh, h64.grad), (dw, w64.grad), (db, None if b is None else b64.grad)):
        if want is not None:
            assert (got.double() - want).abs().max().item() <= REL * want.abs().max().item()
    # each coefficient alone moves the gradient, and differently
    only_z = _run(h, w, b, lab, label_smoothing=ls, chunk=chunk, z_loss=Z)[1]
    only_c = _run(h, w, b, lab, label_smoothing=ls, chunk=chunk, max_logit=C)[1]
    plain = _run(h, w, b, lab, label_smoothing=ls, chunk=chunk)[1]
    assert not torch.equal(only_z, plain) and not torch.equal(only_c, plain) and not torch.equal(only_z, only_c)


def test_the_max_logit_bump_lands_on_the_lowest_index_among_equal_maxima():
    """hidden = one-hot rows and a weight whose columns hold the logits: row 1's maximum appears at columns 3 and 9."""
    V = 12
    x = torch.linspace(-1, 1, V).repeat(3, 1)
    x[1, 3] = x[1, 9] = 2.0
    h = torch.eye(3, requires_grad=True)
    w = x.t().clone().requires_grad_()      # logits = h @ w.t() = x
    lab = torch.tensor([5, 5, -100])
    # hidden is the identity, so dW = dlogits^T h is d loss / d logits transposed, exactly
    plain = torch.autograd.grad(losses.fused_linear_cross_entropy(h, lab, w, None, -100), w)[0].t()
    bump = torch.autograd.grad(losses.fused_linear_cross_entropy(h, lab, w, None, -100, max_logit=C), w)[0].t()
    want = torch.zeros(3, V)
    want[0, V - 1] = C * 1.0 / 2     # c m / n_valid
    want[1, 3] = C * 2.0 / 2
    assert (bump - plain - want).abs().max().item() < 1e-7
    assert (bump - plain)[1, 9].item() == 0.0 and (bump - plain)[2].abs().max().item() == 0.0


# ---- 3: stats -----------------------------------------------------------------------------------------------------------------
def test_stats_accumulate_over_calls_and_over_a_chunked_walk():
    h, w, b, lab = _case()
    x = torch.nn.functional.linear(h, w, b).detach().double()
    valid = lab != -100
    lse, m = torch.logsumexp(x, 1)[valid], x.max(1).values[valid]
    want = torch.stack((valid.sum().double(), lse.sum(), (lse * lse).sum(), m.sum()))
    one, walk = torch.zeros(4), torch.zeros(4)
    l1 = losses.fused_linear_cross_entropy(h, lab, w, b, -100, z_loss=Z, max_logit=C, stats=one)
    l3 = losses.fused_linear_cross_entropy(h, lab, w, b, -100, z_loss=Z, max_logit=C, stats=walk, chunk=3)
    assert one[0].item() == walk[0].item() == 8
    for got in (one, walk):
        assert ((got.double() - want).abs() <= REL * want.abs()).all(), (got, want)
    assert abs(l1.item() - l3.item()) <= REL * abs(l1.item())
    losses.fused_linear_cross_entropy(h, lab, w, b, -100, stats=one)   # a second call adds; coefficients are not needed for stats
    assert ((one.double() - 2 * want).abs() <= REL * 2 * want.abs()).all()
    nothing = torch.zeros(4)
    losses.fused_linear_cross_entropy(h, torch.full_like(lab, -100), w, b, -100, stats=nothing)
    assert nothing.tolist() == [0.0, 0.0, 0.0, 0.0]


# ---- 4: configs, models, trainer -----------------------------------------------------------------------------------------------------
def _spark(z=Z, c=C, seed=1):
    cfg = RWKV7SpeechConfig(vocab_size=257, text_vocab_size=300, audio_global_vocab_size=64, z_loss=z, max_logit=c, **SMALL)
    return _stubbed(RWKV7ForSpeech(cfg), 257, seed)


def test_configs_default_off_round_trip_and_reject(tmp_path):
    assert RWKV7SpeechConfig(**SMALL).z_loss == 0.0 == RWKV7SpeechConfig(**SMALL).max_logit
    assert RWKV7XYConfig(**SMALL).z_loss == 0.0 == RWKV7XYConfig(**SMALL).max_logit
    m = RWKV7ForSpeech(RWKV7SpeechConfig(vocab_size=257, text_vocab_size=300, audio_global_vocab_size=64, z_loss=Z, max_logit=C, **SMALL))
    m.save_pretrained(str(tmp_path / "spark"))
    back = RWKV7ForSpeech.from_pretrained(str(tmp_path / "spark"))
    assert (back.config.z_loss, back.config.max_logit) == (Z, C)
    import json
    stored = json.load(open(tmp_path / "spark" / "config.json"))
    assert stored["z_loss"] == Z and stored["max_logit"] == C
    xy = RWKV7XYConfig(vocab_size=120, speech_vocab_size=16, num_channels=4, text_shift_size=100, z_loss=Z, max_logit=C, **SMALL)
    again = RWKV7XYConfig.from_dict(xy.to_dict())
    assert (again.z_loss, again.max_logit) == (Z, C) and "z_loss" not in again.extra
    for cls in (RWKV7SpeechConfig, RWKV7XYConfig):
        with pytest.raises(ValueError):
            cls(z_loss=-1.0, **SMALL)
    for kw in (dict(z_loss=Z), dict(max_logit=C)):
        with pytest.raises(ValueError):
            RWKV7CosyConfig(vocab_size=200, speech_token_size=50, **kw, **SMALL)
    RWKV7CosyConfig(vocab_size=200, speech_token_size=50, z_loss=0.0, max_logit=0.0, **SMALL)   # zeros are not a request


def test_spark_forward_passes_the_coefficients_to_the_head():
    m = _spark().train()
    m.dropout.p = 0.0
    batch = _spark_batch(3)
    got = m(**batch).loss
    m.config.z_loss = m.config.max_logit = 0.0
    plain = m(**batch).loss
    hidden = m.model(inputs_embeds=batch["inputs_embeds"], attention_mask=batch["attention_mask"])[0]
    shifted = torch.cat((batch["labels"][:, 1:], torch.full((2, 1), -100)), 1)
    x = m.lm_head(hidden).detach().double().reshape(-1, 257)
    lse = torch.logsumexp(x, 1)[shifted.reshape(-1) != -100]
    want = plain.item() + Z * (lse * lse).mean().item()
    assert abs(got.item() - want) <= REL * abs(want) and got.item() != plain.item()


def test_xy_forward_passes_the_coefficients_per_channel_with_bias_and_smoothing():
    cfg = RWKV7XYConfig(vocab_size=120, speech_vocab_size=16, num_channels=4, text_shift_size=100, lsm_weight=0.1, z_loss=Z, max_logit=C,
                        **SMALL)
    m = _stubbed(RWKV7XYLM(cfg), 120, 2).train()
    g = torch.Generator().manual_seed(4)
    ids = torch.cat([torch.randint(0, 120, (2, 10, 1), generator=g), torch.randint(0, 16, (2, 10, 3), generator=g)], 2)
    labels = ids.roll(1, 1).clone()
    labels[0, :3, :] = -100
    m.logit_stats = torch.zeros(4)
    got = m(input_ids=ids, labels=labels).loss
    hidden = m.model(inputs_embeds=m.embed(ids))[0].detach().double()
    want, tokens = 0.0, 0
    for i in range(4):
        head = m.heads[i]
        ret, _ = _fp64_objective(hidden.reshape(-1, 128), head.weight.detach().double(), head.bias.detach().double(),
                                 labels[:, :, i].reshape(-1), 0.1, Z, C)
        want, tokens = want + ret.item(), tokens + (labels[:, :, i] != -100).sum().item()
    assert abs(got.item() - want) <= REL * abs(want)
    assert m.logit_stats[0].item() == tokens, "every channel adds its rows"


def test_trainer_keeps_the_statistics_per_optimizer_step():
    torch.manual_seed(11)
    tr = trainer.DataParallelTrainer(_spark().train(), **LR)
    assert tr.last_logit_stats is None and tr.model.logit_stats is not None, "non-zero coefficients switch the statistics on"
    tr.model.dropout.p = 0.0
    b1, b2 = _spark_batch(5), _spark_batch(6)

    def fp64_sums(batch):
        with torch.no_grad():
            hidden = tr.model.model(inputs_embeds=batch["inputs_embeds"], attention_mask=batch["attention_mask"])[0]
            x = tr.model.lm_head(hidden).double().reshape(-1, 257)
        valid = torch.cat((batch["labels"][:, 1:], torch.full((2, 1), -100)), 1).reshape(-1) != -100
        lse, m = torch.logsumexp(x, 1)[valid], x.max(1).values[valid]
        return torch.stack((valid.sum().double(), lse.sum(), (lse * lse).sum(), m.sum()))

    want = fp64_sums(b1) + fp64_sums(b2)     # before the step: both micro-batches see the same parameters
    tr.accumulate(**b1)
    tr.step(**b2)
    got = tr.last_logit_stats
    assert set(got) == {"mean_lse", "mean_lse_sq", "mean_max", "tokens"}
    assert got["tokens"].item() == want[0].item()
    for key, i in (("mean_lse", 1), ("mean_lse_sq", 2), ("mean_max", 3)):
        ref = (want[i] / want[0]).item()
        assert abs(got[key].item() - ref) <= REL * abs(ref), key
    want = fp64_sums(b1)
    tr.step(**b1)
    assert tr.last_logit_stats["tokens"].item() == want[0].item(), "zeroed at the start of every optimizer step"
    assert got["tokens"].item() != 0 and got is not tr.last_logit_stats, "the earlier step's values are the caller's to keep"


def test_trainer_statistics_alone_change_no_parameter_and_need_a_cross_entropy_model():
    def run(**kw):
        torch.manual_seed(12)
        tr = trainer.DataParallelTrainer(_spark(0.0, 0.0).train(), **LR, **kw)
        for s in range(3):
            tr.step(**_spark_batch(20 + s))
        return tr
    a, b = run(), run(logit_stats=True)
    assert a.last_logit_stats is None and a.model.logit_stats is None
    assert b.last_logit_stats["tokens"].item() > 0
    assert torch.equal(a.flat.flat_param, b.flat.flat_param) and torch.equal(a.exp_avg_sq, b.exp_avg_sq) and a.digest() == b.digest()
    with pytest.raises(ValueError):
        trainer.DataParallelTrainer(torch.nn.Linear(128, 128), logit_stats=True, **LR)


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    trainer.init_distributed("gloo")
    torch.set_num_threads(1)
    torch.manual_seed(20 + rank)
    tr = trainer.DataParallelTrainer(_spark().train(), bucket_bytes=4096, **LR)
    for s in range(2):
        tr.step(**_spark_batch(100 * s + rank))
    q.put((rank, tr.digest(), tr.flat.flat_param.clone(), {k: v.item() for k, v in tr.last_logit_stats.items()}))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_gloo_ranks_stay_bit_identical_with_the_coefficients_on():
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
    assert res[0][1] == res[1][1] and torch.equal(res[0][2], res[1][2]), "replicas differ"
    for r in res:
        assert r[3]["tokens"] == 2 * 11 - 3 and r[3]["mean_lse"] > 0 and r[3]["mean_lse_sq"] >= r[3]["mean_lse"] ** 2 * (1 - REL)
    assert res[0][3]["mean_lse"] != res[1][3]["mean_lse"], "the statistics are this rank's rows only: no collective"
