"""GPU (-m gpu): rwkv7_head_eval_bf16 and what is built on it (losses.fused_linear_eval, the heads' eval_metrics,
DataParallelTrainer.evaluate).

Kernel:
  loss_rows    : bit-equal to rwkv7_ce_fwd_bwd_ld_bf16 (kind 0) / rwkv7_kl_acc_fwd_bwd_bf16 (kind 1) run in place on a copy of the same
                 buffer (same address modulo 16 bytes), and within the bar test_cosy_head_gpu.py applies to the KL entry's loss against
                 the fp64 restatement on the same bf16 logits:  2 max_rows|fp32_chain - exact| + V 2^-24 max(|x|, lse) of the row
  correct_rows : bit-equal to the KL entry's;  argmax_rows : torch.argmax of the logits moved to the CPU
  the buffer   : byte-identical after the call, pad columns and a canary row on each side included
Heads: eval_metrics (bf16, HIP path) against the existing eval-mode forward(labels=...).  Both losses are fp32 arithmetic on bf16 logits of
  the same GEMM operands; if the two GEMM calls round a logit differently it moves by one bf16 ulp (2^-8 relative), and a row's loss is
  1-Lipschitz in the max-norm of its logits up to the factor 2 of the label term: bar = 2 * 2^-8 max|logit| + 1e-5 |loss|.  A row whose
  two largest logits are within two bf16 ulps may flip its argmax: the correct count may differ by the number of such rows."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from cosy_head_ref import exact_rows, fp32_chain_rows
from rwkvtts_amd import layouts as L, losses, trainer
from rwkvtts_amd.cosy_llm import RWKV7CosyConfig, RWKV7CosyLM, RWKV7LM
from rwkvtts_amd.spark_llm import RWKV7ForSpeech, RWKV7SpeechConfig
from rwkvtts_amd.xy_llm import RWKV7XYConfig, RWKV7XYLM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN_BITS = 0x7FC1   # a quiet NaN with a payload: pad columns and canary rows must keep it bit for bit
VS = [2, 1025, 6562, 8192, 8193, 66661]
ROWS = [1, 3, 4, 5, 67]
P = ctypes.c_void_p


def _bits(t):
    return t.view(torch.int16)


class Buf:
    """[rows, ld] bf16 logits inside a NaN-filled allocation: `offset` elements, a canary row, the rows, a canary row."""

    def __init__(self, rows, V, ld, offset, fill):
        self.rows, self.V, self.ld = rows, V, ld
        self.flat = torch.full((offset + (rows + 2) * ld,), NAN_BITS, dtype=torch.int16, device=DEV).view(torch.bfloat16)
        self.x = self.flat[offset + ld:offset + ld + rows * ld].view(rows, ld)
        self.x[:, :V] = fill.to(DEV)
        assert self.x.data_ptr() % 16 == (2 * (offset + ld)) % 16

    def copy(self):
        c = Buf.__new__(Buf)
        c.rows, c.V, c.ld = self.rows, self.V, self.ld
        c.flat = self.flat.clone()
        off = (self.x.data_ptr() - self.flat.data_ptr()) // 2
        c.x = c.flat[off:off + self.rows * self.ld].view(self.rows, self.ld)
        assert c.x.data_ptr() % 16 == self.x.data_ptr() % 16
        return c


def _labels(rows, V, g, ignore):
    labels = torch.randint(0, V, (rows,), generator=g)
    labels[0] = 0
    if rows > 1:
        labels[1] = V - 1
    labels[2::3] = ignore   # a third of the rows ignored
    return labels.to(DEV)


def _stream():
    return P(torch.cuda.current_stream().cuda_stream)


def _eval(lib, b, rows, labels, ignore, kind, s, want_argmax=True):
    loss = torch.full((rows,), -1.0, dtype=torch.float32, device=DEV)
    corr = torch.full((rows,), -1, dtype=torch.int32, device=DEV)
    amax = torch.full((rows,), -1, dtype=torch.int32, device=DEV) if want_argmax else None
    rc = lib.rwkv7_head_eval_bf16(rows, b.V, b.ld, b.x.data_ptr(), labels.data_ptr(), ignore, kind, s, loss.data_ptr(), corr.data_ptr(),
                                  amax.data_ptr() if want_argmax else None, _stream())
    assert rc == 0
    return loss, corr, amax


def _train_entries(lib, b, rows, labels, ignore, kind, s):
    """(loss_rows of the kind's training entry, correct_rows of the KL entry), each in place on its own copy of the buffer"""
    kl = b.copy()
    kl_loss = torch.empty(rows, dtype=torch.float32, device=DEV)
    corr = torch.empty(rows, dtype=torch.int32, device=DEV)
    assert lib.rwkv7_kl_acc_fwd_bwd_bf16(rows, b.V, b.ld, kl.x.data_ptr(), kl.x.data_ptr(), labels.data_ptr(), ignore, s, 1.0,
                                         kl_loss.data_ptr(), corr.data_ptr(), _stream()) == 0
    if kind == 1:
        return kl_loss, corr
    ce = b.copy()
    ce_loss = torch.empty(rows, dtype=torch.float32, device=DEV)
    assert lib.rwkv7_ce_fwd_bwd_ld_bf16(rows, b.V, b.ld, ce.x.data_ptr(), labels.data_ptr(), ignore, 1.0, ce_loss.data_ptr(), s,
                                        _stream()) == 0
    return ce_loss, corr


def _exact(x, labels, ignore, kind, s):
    """fp64 (loss_rows, bar) from the same bf16 logits; bar: the KL entry's loss bar of test_cosy_head_gpu.py with the kind's fp32 chain"""
    valid = labels != ignore
    xd = x.double()
    lse = torch.logsumexp(xd, dim=1)
    if kind == 1:
        assert ignore == -1
        e_loss = exact_rows(x, labels, s)[0]
        chain = fp32_chain_rows(x, labels, s).double()
    else:
        xy = xd.gather(1, labels.clamp(min=0)[:, None])[:, 0]
        e_loss = ((1 - s) * (lse - xy) + s * (lse - xd.mean(1))) * valid
        chain = (F.cross_entropy(x.float(), labels.clamp(min=0), reduction="none", label_smoothing=s) * valid).double()
    bar = 2 * (chain - e_loss).abs().max() + x.shape[1] * 2.0 ** -24 * torch.maximum(xd.abs().max(1).values, lse.abs())
    return e_loss, bar


def _check(lib, tag, b, labels, ignore, kind, s, rows_list=None):
    pristine = b.flat.clone()
    x = b.x[:, :b.V]
    e_loss, bar = _exact(x, labels, ignore, kind, s)
    cpu_argmax = x.cpu().float().argmax(1)
    for rows in rows_list or [b.rows]:
        loss, corr, amax = _eval(lib, b, rows, labels, ignore, kind, s)
        t_loss, t_corr = _train_entries(lib, b, rows, labels, ignore, kind, s)
        torch.cuda.synchronize()
        name = f"{tag} kind={kind} s={s} rows={rows}"
        assert torch.equal(_bits(b.flat), _bits(pristine)), f"{name}: the logits buffer changed"
        assert torch.equal(loss.view(torch.int32), t_loss.view(torch.int32)), f"{name}: loss_rows differs from the training entry's bits"
        assert torch.equal(corr, t_corr), f"{name}: correct_rows differs from the KL entry's"
        assert torch.equal(amax.cpu().long(), cpu_argmax[:rows]), f"{name}: argmax_rows"
        ign = labels[:rows] == ignore
        assert (loss[ign] == 0).all() and (corr[ign] == 0).all(), f"{name}: ignored rows"
        assert torch.equal(corr.long(), ((amax.long() == labels[:rows]) & ~ign).long()), name
        ratio = ((loss.double() - e_loss[:rows]).abs() / bar[:rows]).max().item()
        print(f"RATIO {name} loss_rows {ratio:.3f}")
        assert torch.isfinite(loss).all() and ratio <= 1.0, f"{name}: loss_rows {ratio} x the bar"
    l2, c2, _ = _eval(lib, b, b.rows, labels, ignore, kind, s, want_argmax=False)   # argmax_rows = NULL
    assert torch.equal(l2, loss) and torch.equal(c2, corr)


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("V", VS)
def test_kernel_against_the_training_entries_and_fp64_rows(hip_lib, V, kind):
    g = torch.Generator().manual_seed(V + kind)
    ignore = -100 if kind == 0 else -1
    fill = (torch.randn(67, V, generator=g) * 3.0).bfloat16()
    labels = _labels(67, V, g, ignore)
    for ld in (V, -(-V // 8) * 8 + 8):
        for offset in (0, 1):   # offset 1: the base pointer one element into the allocation -- rows not 16-byte aligned
            b = Buf(67, V, ld, offset, fill)
            for s in (0.0, 0.1):
                _check(hip_lib, f"V={V} ld={ld} off={offset}", b, labels, ignore, kind, s, ROWS)


@pytest.mark.parametrize("kind", [0, 1])
def test_kernel_all_rows_ignored(hip_lib, kind):
    V, ignore = 6562, -100 if kind == 0 else -1
    g = torch.Generator().manual_seed(1)
    b = Buf(5, V, 6576, 0, (torch.randn(5, V, generator=g) * 3.0).bfloat16())
    labels = torch.full((5,), ignore, device=DEV)
    _check(hip_lib, "all-ignored", b, labels, ignore, kind, 0.1)


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("V,ld,offset", [(1025, 1025, 0), (8193, 8208, 0), (8193, 8208, 1)])
def test_kernel_logits_of_magnitude_80(hip_lib, V, ld, offset, kind):
    g = torch.Generator().manual_seed(80)
    ignore = -100 if kind == 0 else -1
    fill = (torch.randn(7, V, generator=g) * 30.0).clamp(-80, 80).bfloat16()
    fill[0, 1], fill[0, 0] = 80.0, -80.0    # label 0 at -80 under a maximum of +80
    fill[1, V - 1] = 80.0                   # label V - 1 is the maximum
    fill[3, :] = -80.0                      # a whole row at -80
    fill[4, :] = 80.0                       # ... and one at +80
    labels = _labels(7, V, g, ignore)
    _check(hip_lib, f"pm80 V={V} ld={ld} off={offset}", Buf(7, V, ld, offset, fill), labels, ignore, kind, 0.1)


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("V,ld", [(6562, 6562), (6562, 6576), (8193, 8193)])
def test_kernel_planted_ties(hip_lib, V, ld, kind):
    g = torch.Generator().manual_seed(7)
    ignore = -100 if kind == 0 else -1
    fill = (torch.randn(12, V, generator=g) * 3.0).bfloat16()
    labels = torch.randint(0, V, (12,), generator=g)
    top = 40.0
    plant = [((5, 6000), 5, 1), ((5, 6000), 6000, 0),            # two maxima: first piece against a late piece
             ((100, V - 1), 100, 1), ((100, V - 1), V - 1, 0),    # a piece against the last single element
             ((3000, 3001), 3000, 1), ((3000, 3001), 3001, 0),    # neighbours inside one 16-byte piece
             ((0, 1, V - 1), 0, 1), ((0, 1, V - 1), 1, 0), ((7, 4000, 6001), 6001, 0)]   # three maxima
    for r, (cols, lab, _) in enumerate(plant):
        for c in cols:
            fill[r, c] = top
        labels[r] = lab
    fill[9, :] = 1.0
    labels[9] = 0          # the whole row tied: index 0 wins
    fill[10, :] = 1.0
    labels[10] = 17
    labels[11] = ignore
    want = [w for _, _, w in plant] + [1, 0, 0]
    assert (fill.float().argmax(1) == labels).long().tolist()[:11] == want[:11]   # torch.argmax on the CPU
    b = Buf(12, V, ld, 0, fill)
    labels = labels.to(DEV)
    _check(hip_lib, f"ties V={V} ld={ld}", b, labels, ignore, kind, 0.1)
    assert _eval(hip_lib, b, 12, labels, ignore, kind, 0.1)[1].tolist() == want


def test_every_einval_case_returns_without_a_launch(hip_lib):
    V = 11
    b = Buf(4, V, V, 0, torch.zeros(4, V).bfloat16())
    labels = torch.zeros(4, dtype=torch.long, device=DEV)
    loss = torch.full((4,), -7.0, dtype=torch.float32, device=DEV)
    corr = torch.full((4,), -7, dtype=torch.int32, device=DEV)
    amax = torch.full((4,), -7, dtype=torch.int32, device=DEV)

    def call(rows=4, V=V, ld=V, logits=b.x.data_ptr(), lab=labels.data_ptr(), kind=0, s=0.1, lo=loss.data_ptr(), co=corr.data_ptr()):
        return hip_lib.rwkv7_head_eval_bf16(rows, V, ld, logits, lab, -1, kind, s, lo, co, amax.data_ptr(), _stream())

    cases = [dict(logits=None), dict(lab=None), dict(lo=None), dict(co=None), dict(rows=0), dict(rows=-3), dict(V=1, ld=1), dict(V=0),
             dict(ld=V - 1), dict(kind=2), dict(kind=-1), dict(s=-0.1), dict(s=1.0), dict(s=float("nan")), dict(kind=1, s=1.0)]
    for kw in cases:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (loss == -7).all() and (corr == -7).all() and (amax == -7).all(), "an output was written"
    assert call() == 0
    torch.cuda.synchronize()
    assert (loss != -7).all() and (amax == 0).all()


# ---- fused_linear_eval and the heads on the HIP path --------------------------------------------------------------------------------
SMALL = dict(hidden_size=128, num_hidden_layers=2, decay_low_rank_dim=32, a_low_rank_dim=32, v_low_rank_dim=16, gate_low_rank_dim=32)


def _to(batch, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}


def _loss_bar(logits, loss):
    return 2 * 2.0 ** -8 * max(l.abs().max().item() for l in logits) + 1e-5 * abs(loss)


def _uncertain(logits, valid):
    """rows among `valid` whose two largest logits are within two bf16 ulps of each other"""
    top2 = logits.float().topk(2, dim=-1).values
    return ((top2[..., 0] - top2[..., 1] <= 2.0 ** -7 * top2[..., 0].abs()) & valid).sum().item()


def test_fused_linear_eval_hip_route_in_chunks(hip_lib):
    rows, D, V = 300, 128, 51
    g = torch.Generator().manual_seed(11)
    h = torch.randn(rows, D, generator=g).bfloat16().to(DEV)
    w = (torch.randn(V, D, generator=g) * 0.2).bfloat16().to(DEV)
    bias = (torch.randn(V, generator=g) * 0.1).bfloat16().to(DEV)
    labels = torch.randint(0, V, (rows,), generator=g)
    labels[torch.randperm(rows, generator=g)[:100]] = -1
    labels = labels.to(DEV)
    for kind, s, bb in ((0, 0.0, None), (0, 0.1, bias), (1, 0.1, bias)):
        hits = losses.EVAL_HITS[0]
        loss_sum, n_valid, n_correct = losses.fused_linear_eval(h, labels, w, bb, -1, kind, smoothing=s, chunk=128)
        assert losses.EVAL_HITS[0] == hits + 3, "the HIP kernel was not launched once per chunk (128, 128, 44 rows)"
        whole = losses.fused_linear_eval(h, labels, w, bb, -1, kind, smoothing=s)
        assert losses.EVAL_HITS[0] == hits + 4
        logits = F.linear(h, w, bb)
        per, ok = losses._eval_rows_torch(logits, labels, -1, kind, s)
        assert n_valid.item() == whole[1].item() == 200
        total = per.double().sum().item()
        bar = 200 * _loss_bar([logits], 0.0) + 1e-5 * abs(total)   # 200 valid rows, each within the per-row bar
        for got in (loss_sum, whole[0]):
            assert abs(got.item() - total) <= bar
        slack = _uncertain(logits, labels != -1)
        assert abs(n_correct.item() - ok.sum().item()) <= slack and abs(whole[2].item() - ok.sum().item()) <= slack


def _spark(seed=3, vocab=257):
    cfg = RWKV7SpeechConfig(vocab_size=vocab, text_vocab_size=300, audio_global_vocab_size=64, **SMALL)
    return RWKV7ForSpeech(cfg).init_weights(seed=seed).to(DEV).to(torch.bfloat16)


def test_spark_eval_metrics_against_the_eval_mode_forward(hip_lib):
    m = _spark().train()
    batch = L.synthetic_spark_batch(m, 2, 256, seed=5, n_text=31, n_global=8)
    hits = losses.EVAL_HITS[0]
    got = m.eval_metrics(**batch)
    assert losses.EVAL_HITS[0] == hits + 1 and m.training
    m.eval()
    with torch.no_grad():
        out = m(**batch)
    shifted = torch.cat((batch["labels"][:, 1:], torch.full_like(batch["labels"][:, :1], -100)), 1)
    valid = shifted != -100
    assert got["tokens"].item() == valid.sum().item()
    print(f"RATIO spark loss {abs(got['loss'].item() - out.loss.item()) / _loss_bar([out.logits], out.loss.item()):.3f}")
    assert abs(got["loss"].item() - out.loss.item()) <= _loss_bar([out.logits], out.loss.item())
    want = ((out.logits.argmax(-1) == shifted) & valid).sum().item()
    assert abs(got["correct"].item() - want) <= _uncertain(out.logits, valid)


def test_xy_eval_metrics_against_the_eval_mode_forward(hip_lib):
    cfg = RWKV7XYConfig(vocab_size=120, speech_vocab_size=16, num_channels=4, text_shift_size=100, lsm_weight=0.1, **SMALL)
    m = RWKV7XYLM(cfg).init_weights(seed=2)
    with torch.no_grad():
        for h in m.heads:
            h.bias.normal_(0, 0.1)
    m = m.to(DEV).to(torch.bfloat16).train()
    g = torch.Generator().manual_seed(0)
    text = [[101 + i for i in range(5)], [90, 91, 92]]
    audio = [torch.randint(0, 15, (4, n), generator=g).tolist() for n in (9, 5)]
    batch = _to(L.XYDataProcessor(120, 4, 100, 16).process_batch(text, audio), DEV)
    hits = losses.EVAL_HITS[0]
    got = m.eval_metrics(**batch)
    assert losses.EVAL_HITS[0] == hits + 4 and m.training
    m.eval()
    with torch.no_grad():
        out = m(**batch)
    labels = batch["labels"]
    assert got["tokens"].tolist() == [(labels[:, :, c] != -100).sum().item() for c in range(4)]
    bar = 4 * _loss_bar(out.logits, out.loss.item() / 4)   # a sum of four means
    print(f"RATIO xy loss {abs(got['loss'].item() - out.loss.item()) / bar:.3f}")
    assert abs(got["loss"].item() - out.loss.item()) <= bar
    for c in range(4):
        valid = labels[:, :, c] != -100
        want = ((out.logits[c].argmax(-1) == labels[:, :, c]) & valid).sum().item()
        assert abs(got["correct"][c].item() - want) <= _uncertain(out.logits[c], valid)


@pytest.mark.parametrize("nl", [True, False])
def test_cosy_eval_metrics_against_the_eval_mode_forward(hip_lib, nl):
    cfg = RWKV7CosyConfig(vocab_size=200, speech_token_size=50, lsm_weight=0.1, length_normalized_loss=nl, **SMALL)
    llm = RWKV7CosyLM(cfg).init_weights(seed=4).to(torch.bfloat16).to(DEV).train()
    batch = _to(L.cosy_collate([[3, 4, 5, 6], [7, 8]], [list(range(10, 20)), [20, 21, 22]], pad_to_max_length=False), DEV)
    hits = losses.EVAL_HITS[0]
    got = llm.eval_metrics(batch=batch)
    assert losses.EVAL_HITS[0] == hits + 1 and llm.training
    llm.eval()
    with torch.no_grad():
        out = llm(batch=batch)
        labels = llm.build_inputs(batch)[2]
    valid = labels != -1
    assert got["tokens"].item() == 15 and got["denom"].item() == (15 if nl else 2)
    # the loss is a sum over 15 rows divided by the denominator
    bar = 15 / got["denom"].item() * _loss_bar([out.logits], out.loss.item())
    print(f"RATIO cosy nl={nl} loss {abs(got['loss'].item() - out.loss.item()) / bar:.3f}")
    assert abs(got["loss"].item() - out.loss.item()) <= bar
    want = ((out.logits.argmax(-1) == labels) & valid).sum().item()
    assert abs(got["correct"].item() - want) <= _uncertain(out.logits, valid)
    torch.manual_seed(4)
    w = RWKV7LM(128, 128, 50, llm, lsm_weight=0.1, length_normalized_loss=nl).to(torch.bfloat16).to(DEV).train()
    gw = w.eval_metrics(batch)
    assert w.training and gw["tokens"].item() == 15
    w.eval()
    seen = {}
    hook = llm.lm_head.register_forward_hook(lambda mod, args, o: seen.__setitem__("logits", o.detach()))
    with torch.no_grad():
        r = w(batch)
    hook.remove()
    assert abs(gw["loss"].item() - r["loss"].item()) <= 15 / gw["denom"].item() * _loss_bar([seen["logits"]], r["loss"].item())
    assert abs(gw["correct"].item() - round(r["acc"].item() * 15)) <= _uncertain(seen["logits"], valid)


def test_eval_metrics_never_holds_the_logits(hip_lib, monkeypatch):
    """Spark head, rows = 4096, V = 8193, chunk forced to 512: the peak over eval_metrics stays below HALF the bytes of the bf16 logits;
    the existing eval-mode forward on the same batch exceeds ALL of them."""
    rows, V = 4096, 8193
    m = _spark(vocab=V).train()
    batch = L.synthetic_spark_batch(m, 2, rows // 2, seed=5, n_text=31, n_global=8)
    monkeypatch.setattr(losses, "EVAL_CHUNK_ROWS", 512)
    m.eval_metrics(**batch)   # first call: one-time allocations (workspaces) are not the feature's
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    hits = losses.EVAL_HITS[0]
    got = m.eval_metrics(**batch)
    torch.cuda.synchronize()
    peak_eval = torch.cuda.max_memory_allocated() - base
    assert losses.EVAL_HITS[0] == hits + 8
    del got
    m.eval()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with torch.no_grad():
        out = m(**batch)
    torch.cuda.synchronize()
    peak_fwd = torch.cuda.max_memory_allocated() - base
    print(f"PEAK eval_metrics {peak_eval} forward {peak_fwd} logits {rows * V * 2}")
    assert peak_eval < rows * V * 2 // 2
    assert peak_fwd > rows * V * 2
    assert torch.isfinite(out.loss)


# ---- DataParallelTrainer.evaluate on the HIP AdamW path -------------------------------------------------------------------------------
KW = dict(lr=1e-3, warmup_steps=0, total_steps=10)


def _advance(tr, steps):
    for step in steps:
        tr.step(**L.synthetic_spark_batch(tr.model, 2, 256, seed=100 * step, n_text=31, n_global=8))


def _state(tr):
    torch.cuda.synchronize()
    return dict(param=tr.flat.flat_param.clone(), master=tr.master.clone(), exp_avg=tr.exp_avg.clone(), exp_avg_sq=tr.exp_avg_sq.clone(),
                grad=tr.flat.flat_grad.clone(), nan_flag=tr.nan_flag.clone(), step_idx=tr.step_idx, last_lr=tr.last_lr, lr=tr.current_lr(),
                rng=torch.get_rng_state(), cuda_rng=torch.cuda.get_rng_state(DEV), training=tr.model.training)


def _same(a, b):
    for k, v in a.items():
        assert torch.equal(v, b[k]) if torch.is_tensor(v) else v == b[k], k


@pytest.mark.timeout(120)
def test_three_steps_evaluate_two_steps_equals_five_steps_on_the_hip_path(hip_lib):
    def run(evaluate):
        torch.manual_seed(11)
        m = _spark().train()
        assert m.dropout.p == 0.02
        tr = trainer.DataParallelTrainer(m, **KW)
        assert tr.hip_adamw
        _advance(tr, range(3))
        res = None
        if evaluate:
            shard = [L.synthetic_spark_batch(m, 2, 256, seed=900 + i, n_text=31, n_global=8) for i in range(2)]
            before, digest = _state(tr), tr.digest()
            hits = losses.EVAL_HITS[0]
            res = tr.evaluate(shard)
            assert losses.EVAL_HITS[0] == hits + 2
            _same(before, _state(tr))
            assert tr.digest() == digest
        _advance(tr, range(3, 5))
        return _state(tr), res

    (a, _), (b, res) = run(False), run(True)
    _same(a, b)
    assert res["tokens"] == 2 * 2 * (256 - 3 - 31 - 8)   # two batches of two samples, every semantic position once
    assert 0.0 <= res["accuracy"] <= 1.0 and res["loss"] > 0
