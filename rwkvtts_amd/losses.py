"""Loss heads of the three layouts.

fused_linear_cross_entropy : stands in for rwkvfla's FusedLinearCrossEntropyLoss (model/llm/spark_llm.py:8,146-160):
    lm_head GEMM + softmax-CE computed chunk by chunk over the tokens so the [B*T, V] logits (512 MiB at
    B=8,T=4096,V=8193 bf16) are never materialised; gradients w.r.t. hidden and weight are produced in the
    same pass and scaled by the incoming grad in backward.
label_smoothing_kl         : third_party/cosyvoice/transformer/label_smoothing_loss.py:21-96 (Cosy layout).
th_accuracy                : third_party/cosyvoice/utils/common.py:76-95.
fused_linear_kl_accuracy   : the two above on the head GEMM's bf16 logits chunk by chunk through rwkv7_kl_acc_fwd_bwd_bf16 (opt-in:
    RWKV7LM(fused_loss=True)); label_smoothing_kl_fused: the loss alone on logits the caller keeps (RWKV7CosyConfig(fused_loss=True)).
fused_linear_eval          : forward-only loss sum / valid count / correct count of a head for held-out evaluation, chunk by chunk
    through rwkv7_head_eval_bf16 (the heads' eval_metrics, DataParallelTrainer.evaluate).
fused_linear_score         : the same rows reduced per SEQUENCE instead of per batch (loss sum, tokens, correct, worst token): the
    per-row outputs of rwkv7_head_eval_bf16 kept for the whole batch, then one rwkv7_seq_scores_f32 launch (the heads' score,
    DataParallelTrainer.score).
fused_linear_seq_logprob   : that loss sum, negated, UNDER AUTOGRAD with an upstream gradient per sequence (the heads' sequence_logprobs,
    DataParallelTrainer.preference_step): backward runs the head GEMM again chunk by chunk and rwkv7_ce_seq_bwd_bf16 on each chunk.
fused_linear_policy        : the token-level clipped policy objective (PPO-clip / GRPO, optional k3 KL to a reference) UNDER AUTOGRAD (the
    heads' policy_loss, DataParallelTrainer.policy_step): rwkv7_ce_policy_fwd_bwd_bf16 writes d loss / d logits in the forward chunk walk.
"""
import contextlib
import math
import os

import torch
import torch.nn.functional as F

from . import _lib

HIP_CE = os.environ.get("RWKV7_HIP_CE", "1") == "1"   # A/B switch: 0 = the torch chain for every head
CHECK_LABELS = os.environ.get("RWKV7_CHECK_LABELS", "0") == "1"
PADDED_HEAD = os.environ.get("RWKV7_PADDED_HEAD", "1") == "1"   # A/B switch (see _FusedLinearCE.forward)
PADDED_HEAD_HITS = [0]


def _check_labels(labels, V, ignore_index):
    """RWKV7_CHECK_LABELS=1: labels must be < V or == ignore_index, since the head kernels index x[label] unchecked (one host sync per
    call, debugging only)."""
    if CHECK_LABELS:
        bad = (labels != ignore_index) & ((labels < 0) | (labels >= V))
        assert not bool(bad.any()), f"labels outside [0, {V}) that are not ignore_index={ignore_index}"


def _hip_gate(x, labels, *more):
    """The HIP head kernels apply: bf16 CUDA x (hidden states or logits) and every tensor of `more` (weight, bias) that is not None,
    int64 labels, and the A/B switch on."""
    return (HIP_CE and x.is_cuda and x.dtype == torch.bfloat16 and labels.dtype == torch.int64
            and all(m is None or (m.is_cuda and m.dtype == torch.bfloat16) for m in more))


# ---- what every head shares: the chunk walk, the reused logits buffer, the gradient accumulator --------------------------------------
def _chunk_plan(N, V, esize, hip, chunk, align=1, overlap_last=False):
    """The walk of every head over N rows: (rows per chunk, [(s, rows, skip) of every chunk]) -- the chunk is rows s .. s + rows - 1,
    of which the first `skip` belong to its predecessor already.  chunk: rows per round (None: EVAL_CHUNK_ROWS if set, else
    auto_chunk).  On the HIP route it is rounded up to a multiple of `align`, and with overlap_last a shorter last chunk is taken as
    the LAST `chunk` rows, so that every GEMM call has `chunk` rows: skip is non-zero for that chunk alone."""
    if chunk is None:
        # torch route: fp32 logits and one fp32 temporary of that size
        chunk = EVAL_CHUNK_ROWS or auto_chunk(N, V, esize if hip else 8)
    if hip:
        chunk = -(-max(1, chunk) // align) * align
    chunk = max(1, min(chunk, N))
    starts = list(range(0, N, chunk))
    if hip and overlap_last:
        starts[-1] = N - chunk   # N rows when one chunk holds them all
    walk, done = [], 0
    for s in starts:
        rows = min(chunk, N - s)
        walk.append((s, rows, done - s))
        done = s + rows
    return chunk, walk


def _logits_buffer(chunk, weight):
    """(buf, wt) of the routes that keep ONE bf16 logits buffer for all chunks: buf [chunk, ld], ld = V rounded up to 16-byte rows."""
    return torch.empty(chunk, -(-weight.shape[0] // 8) * 8, dtype=weight.dtype, device=weight.device), weight.t()


def _fill_logits(buf, h, wt, bias):
    """F.linear(h, wt.t(), bias) into the first rows of buf: the GEMM writes the V logits of a row, nothing reads the rest of it."""
    logits = buf[:h.shape[0], :wt.shape[1]]
    if bias is None:
        torch.mm(h, wt, out=logits)
    else:
        torch.addmm(bias, h, wt, out=logits)
    return logits


class _HeadGrads:
    """dh, dw and db of a head (each None where needs_input_grad says so), accumulated chunk by chunk from pd = d loss / d logits.
    What the three nodes keep apart, because another leading dimension or output type can make the library take another GEMM kernel,
    with other bits and another speed:
      _FusedLinearCE         : logits by F.linear into a fresh tensor per chunk (padded head: rwkv7_gemm_nt_bf16 into a fresh
                               [rows, Vp], `weight` here the zero-padded [Vp, D] copy, dw[:V] taken at the end); bf16 GEMMs
      _FusedLinearKLAcc      : logits by F.linear; fp32 GEMMs (fp32=True: dh is an fp32 buffer, no bf16 rounding of a chunk's dw)
      _FusedLinearSeqLogprob : logits in the reused [chunk, ld] buffer (_logits_buffer, overlapping last chunk); bf16 GEMMs"""

    def __init__(self, need, hidden, weight, bias, fp32=False):
        self.weight, self.fp32 = weight, fp32
        self.dh = torch.empty_like(hidden, dtype=torch.float32 if fp32 else hidden.dtype) if need[0] else None
        self.dw = torch.zeros_like(weight, dtype=torch.float32) if need[1] else None
        self.db = torch.zeros_like(bias, dtype=torch.float32) if (bias is not None and need[2]) else None

    def add(self, pd, h, lo, hi, p32=None):
        """Rows lo .. hi - 1: pd [hi - lo, V] and their hidden states h.  p32: the fp32 rows pd was rounded from, where the caller has
        them (the torch routes): db sums those."""
        if self.dh is not None:
            self.dh[lo:hi] = torch.mm(pd, self.weight, out_dtype=torch.float32) if self.fp32 else pd @ self.weight
        if self.dw is not None:
            self.dw += torch.mm(pd.t(), h, out_dtype=torch.float32) if self.fp32 else (pd.t() @ h).float()
        if self.db is not None:
            self.db += pd.sum(0, dtype=torch.float32) if p32 is None else p32.sum(0)

    @staticmethod
    def scaled(dh, dw, db, g, hdtype, wdtype):
        """The backward triple: scaled in fp32 and rounded once -- rounding the scalar to bf16 first would put a systematic error of
        up to 2^-9 on every hidden-state gradient relative to the (fp32-scaled) head-weight gradient."""
        return ((dh.float() * g).to(hdtype) if dh is not None else None,
                (dw * g).to(wdtype) if dw is not None else None,
                (db * g).to(wdtype) if db is not None else None)


class _FusedLinearCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hidden, weight, bias, labels, ignore_index, chunk, label_smoothing, z_loss=0.0, max_logit=0.0, stats=None):
        N, D = hidden.shape
        # the logit regularisers (fused_linear_cross_entropy's z_loss / max_logit / stats).  Off -- both
        # coefficients 0 and no stats tensor -- every line below runs as it did before they existed.
        reg = z_loss != 0 or max_logit != 0 or stats is not None
        if reg:
            reg_sums = torch.zeros(3, dtype=torch.float32, device=hidden.device)   # sum lse, sum lse^2, sum m over the valid rows
        valid = labels != ignore_index
        n_valid = valid.sum().clamp(min=1)
        inv = 1.0 / n_valid.float()
        loss = torch.zeros((), dtype=torch.float32, device=hidden.device)
        need = ctx.needs_input_grad
        # bias and label smoothing (the XY heads, xy_llm.py:233-240) ride on the same kernel since round 4: at configs[3] the torch
        # chain behind them (fp32 logits, logsumexp, softmax, scatter, casts) was ~40 ms of a 417 ms step
        # NUMERICS of the HIP path (also for the XY heads since round 4): the logits are the bf16 output of the head GEMM -- logsumexp,
        # softmax and the smoothing mean term sum(x)/V are computed in fp32 FROM those bf16 logits, where the torch chain below keeps
        # fp32 logits.  The formula is torch's CrossEntropyLoss(label_smoothing, ignore_index); tests/test_heads_reference.py holds
        # bias + smoothing to the training tolerance against the reference's own forward.  Labels must be < V or == ignore_index
        # (the kernel indexes x[label]); RWKV7_CHECK_LABELS=1 asserts it.
        _check_labels(labels, weight.shape[0], ignore_index)
        hip_ce = _hip_gate(hidden, labels, weight, bias) and 0 <= label_smoothing < 1
        # Round 6 (late): a vocabulary that is not a multiple of 256 (the Spark head: 8 193) makes every row of the logits start on a 2-byte
        # boundary and gives the three head GEMMs an odd leading dimension (0.75 PF/s in the library).  With PADDED_HEAD the logits live in
        # a [rows, Vp] buffer, Vp = V rounded up to 256, the weight in a zero-padded [Vp, D] copy: the logits GEMM runs on the own kernel
        # (rwkv7_gemm_nt_bf16: Vp % 256 == 0), the padding columns are exactly 0 before and after the loss kernel (which never touches them),
        # so the two gradient GEMMs run over Vp with aligned operands and give the same sums.
        V = weight.shape[0]
        Vp = -(-V // 256) * 256
        padded = (hip_ce and PADDED_HEAD and bias is None and Vp != V and D % 1024 == 0 and N % 256 == 0 and chunk % 256 == 0
                  and hidden.is_contiguous())
        if padded:
            w_pad = torch.zeros(Vp, D, dtype=weight.dtype, device=weight.device)
            w_pad[:V].copy_(weight)
            PADDED_HEAD_HITS[0] += 1
        grads = _HeadGrads(need, hidden, w_pad if padded else weight, bias)   # padded: dw is [Vp, D] until the end
        for s, rows, _ in _chunk_plan(N, V, hidden.element_size(), hip_ce, chunk)[1]:
            h, lab = hidden[s:s + rows], labels[s:s + rows]
            if hip_ce:
                # bf16 logits straight from the GEMM; one kernel turns them into per-row losses and d loss / d logits
                if padded:
                    pd = torch.empty(rows, Vp, dtype=h.dtype, device=h.device)
                    _lib.call("rwkv7_gemm_nt_bf16", h, rows, Vp, D, h, w_pad, pd, 0)
                else:
                    pd = F.linear(h, weight, bias)   # bf16 logits as nn.Linear gives them (the bias inside the GEMM's fp32 epilogue)
                loss_rows = torch.empty(rows, dtype=torch.float32, device=pd.device)
                if reg:
                    # the same kernel text with the regularisers in the gradient; loss_rows stays the plain CE, the row's lse and
                    # maximum come out beside it (0 on ignored rows, so plain sums are sums over the valid rows)
                    side = torch.empty(2, rows, dtype=torch.float32, device=pd.device)
                    _lib.call("rwkv7_ce_reg_fwd_bwd_bf16", pd, rows, V, pd.shape[1], pd, lab.contiguous(), ignore_index, 1.0, loss_rows,
                              float(label_smoothing), float(z_loss), float(max_logit), side[0], side[1])
                    LOGIT_REG_HITS[0] += 1
                    reg_sums += torch.stack((side[0].sum(), (side[0] * side[0]).sum(), side[1].sum()))
                else:
                    _lib.call("rwkv7_ce_fwd_bwd_ld_bf16", pd, rows, V, pd.shape[1], pd, lab.contiguous(), ignore_index, 1.0, loss_rows,
                              float(label_smoothing))
                loss += loss_rows.sum()
                grads.add(pd, h, s, s + rows)
                continue
            logits = (h @ weight.t()).float()
            if bias is not None:
                logits = logits + bias.float()
            lse = torch.logsumexp(logits, dim=-1)
            vmask = lab != ignore_index
            safe = lab.clamp(min=0)
            tgt = logits.gather(1, safe.unsqueeze(1)).squeeze(1)
            nll = lse - tgt
            if label_smoothing > 0:
                smooth = lse - logits.mean(dim=-1)
                per = (1 - label_smoothing) * nll + label_smoothing * smooth
            else:
                per = nll
            loss += (per * vmask).sum()
            row_reg = None
            if reg:
                a = logits.argmax(dim=-1)   # the lowest index among the maxima
                m = logits.gather(1, a.unsqueeze(1)).squeeze(1)
                reg_sums += torch.stack(((lse * vmask).sum(), (lse * lse * vmask).sum(), (m * vmask).sum()))
                if z_loss != 0 or max_logit != 0:
                    row_reg = (1 + 2 * z_loss * lse, a, max_logit * m)
            if need[0] or need[1]:
                p = _grad_rows_torch(logits, lab, label_smoothing, vmask * inv, row_reg)
                grads.add(p.to(hidden.dtype), h, s, s + rows, p)
        # the HIP path leaves dh / dw unscaled (scale = 1 in the kernel: 1/n_valid lives on the device); backward folds
        # 1/n_valid into the incoming gradient
        ctx.save_for_backward(grads.dh, grads.dw[:V] if need[1] else None, grads.db, inv if hip_ce else None)
        ctx.hdtype, ctx.wdtype = hidden.dtype, weight.dtype
        if reg:
            if stats is not None:
                stats += torch.cat((valid.sum().float().reshape(1), reg_sums))
            if z_loss != 0:
                loss = loss + z_loss * reg_sums[1]
        return loss * inv

    @staticmethod
    def backward(ctx, g):
        dh, dw, db, post = ctx.saved_tensors
        if post is not None:
            g = g * post
        return _HeadGrads.scaled(dh, dw, db, g, ctx.hdtype, ctx.wdtype) + (None,) * 7


def check_logit_reg(z_loss, max_logit, who):
    """The configs' validation of the two coefficients: finite floats >= 0."""
    z, c = float(z_loss), float(max_logit)
    if not (z >= 0 and c >= 0 and math.isfinite(z) and math.isfinite(c)):
        raise ValueError(f"{who}: z_loss and max_logit must be finite and >= 0, got {z_loss}, {max_logit}")
    return z, c


LOGIT_REG_HITS = [0]   # launches of rwkv7_ce_reg_fwd_bwd_bf16 (one per chunk): how a test sees which route a call took
LOGITS_CHUNK_BYTES = int(os.environ.get("RWKV7_CE_CHUNK_BYTES", str(1 << 30)))


def auto_chunk(rows, V, esize=2):
    """Rows per chunk of the head GEMMs: as many as keep the chunk's logits under LOGITS_CHUNK_BYTES (1 GiB of the GPU's 288), in
    multiples of 4096.  The first cut used 4096 rows whatever the vocabulary: eight rounds of three 69-GFLOP GEMMs for the Spark head
    (V = 8193), each too small to fill the chip (0.69-0.80 PF/s, 2.96 ms per step for the node, profiles/r05q_ce_head_probe.txt); the
    whole batch as ONE chunk is 0.54 GB of logits.  The 66 661-wide XY head keeps 4096-row chunks (0.55 GB each)."""
    c = max(4096, (LOGITS_CHUNK_BYTES // (esize * V)) // 4096 * 4096)
    return rows if c >= rows else c


def fused_linear_cross_entropy(hidden, labels, weight, bias=None, ignore_index=-100, chunk=None,
                               label_smoothing=0.0, z_loss=0.0, max_logit=0.0, stats=None):
    """hidden [..., D], labels [...] (already shifted by the caller) -> mean CE over labels != ignore_index.
    chunk: rows per round of head GEMMs (None: auto_chunk).
    z_loss, max_logit (>= 0): two regularisers of the logits' scale.  With lse the row's logsumexp and m its
    largest logit, the gradients are those of the mean over the valid rows of  CE + z_loss lse^2 + 0.5 max_logit m^2  (m's gradient
    lands on the lowest index among the row's maxima; the reference's L2Wrap, rwkv_s2s_single_ffn.py:261-273, is max_logit =
    factor x rows).  The RETURNED loss is (sum CE + z_loss sum lse^2) / n_valid: the 0.5 max_logit m^2 term is gradient-only, as
    in the reference, whose L2Wrap returns the loss unchanged.
    stats: a caller-owned fp32 [4] tensor on hidden's device; the call ADDS (n_valid, sum lse, sum lse^2, sum m) over its valid rows
    into it, with no host read (DataParallelTrainer.last_logit_stats).
    With both coefficients 0 and stats None the call is what it was before these arguments existed, bit for bit.  Otherwise the HIP
    route (padded head included) runs rwkv7_ce_reg_fwd_bwd_bf16 -- the cross-entropy kernel's text with the two terms in the gradient
    -- on the same bf16 logits, and the torch route (fp32 models, RWKV7_HIP_CE=0, the CPU) the same arithmetic from fp32 logits."""
    z_loss, max_logit = check_logit_reg(z_loss, max_logit, "fused_linear_cross_entropy")
    if stats is not None and not (stats.dtype == torch.float32 and stats.shape == (4,) and stats.device == hidden.device):
        raise ValueError("fused_linear_cross_entropy: stats must be an fp32 [4] tensor on the hidden states' device")
    D = hidden.shape[-1]
    if chunk is None:
        # the HIP kernel path keeps ONE bf16 logits tensor per chunk; the torch chain (RWKV7_HIP_CE=0, fp32 models, int32 labels, a
        # non-bf16 bias) keeps fp32 logits, an fp32 softmax and a copy in the hidden dtype: budget 3 x 4 bytes per logit there
        hip = _hip_gate(hidden, labels, weight, bias)
        chunk = auto_chunk(hidden.numel() // D, weight.shape[0], hidden.element_size() if hip else 12)
    if z_loss == 0 and max_logit == 0 and stats is None:
        return _FusedLinearCE.apply(hidden.reshape(-1, D), weight, bias, labels.reshape(-1), ignore_index, chunk,
                                    label_smoothing)
    return _FusedLinearCE.apply(hidden.reshape(-1, D), weight, bias, labels.reshape(-1), ignore_index, chunk,
                                label_smoothing, z_loss, max_logit, stats)


def label_smoothing_kl(logits, target, size, padding_idx, smoothing, normalize_length=False):
    """LabelSmoothingLoss.forward (cosyvoice/transformer/label_smoothing_loss.py:68-96): KL(true_dist || softmax)
    with true_dist = smoothing/(size-1) off-target, 1-smoothing on target; ignored rows zeroed; divided by the
    number of valid tokens (normalize_length) or by the batch size."""
    B = logits.shape[0]
    x = logits.reshape(-1, size)
    t = target.reshape(-1)
    ignore = t == padding_idx
    total = t.numel() - ignore.sum()
    t = t.masked_fill(ignore, 0)
    true_dist = torch.full_like(x, smoothing / (size - 1), dtype=torch.float32)
    true_dist.scatter_(1, t.unsqueeze(1), 1.0 - smoothing)
    kl = F.kl_div(torch.log_softmax(x.float(), dim=1), true_dist, reduction="none")
    denom = total if normalize_length else B
    return kl.masked_fill(ignore.unsqueeze(1), 0).sum() / denom


def th_accuracy(pad_outputs, pad_targets, ignore_label):
    """cosyvoice/utils/common.py:76-95."""
    pred = pad_outputs.view(pad_targets.size(0), pad_targets.size(1), pad_outputs.size(1)).argmax(2)
    mask = pad_targets != ignore_label
    num = torch.sum(pred.masked_select(mask) == pad_targets.masked_select(mask))
    return (num / torch.sum(mask)).detach()


KL_ACC_HITS = [0]   # launches of rwkv7_kl_acc_fwd_bwd_bf16 (one per chunk): how a test sees which route a call took


def _kl_acc_rows(logits, dlogits, labels, V, ignore_index, smoothing, scale=1.0):
    """rwkv7_kl_acc_fwd_bwd_bf16 on 2-D bf16 logits [rows, ld] (unit column stride; columns V.. untouched): writes
    (softmax - true_dist) * scale into dlogits (which may BE logits) and returns (loss_rows fp32 [rows], correct_rows int32 [rows])."""
    rows, ld = logits.shape[0], logits.stride(0)
    assert logits.stride(1) == 1 and dlogits.stride() == logits.stride() and dlogits.shape == logits.shape
    _check_labels(labels, V, ignore_index)
    lab = labels.contiguous()
    loss_rows = torch.empty(rows, dtype=torch.float32, device=logits.device)
    correct = torch.empty(rows, dtype=torch.int32, device=logits.device)
    _lib.call("rwkv7_kl_acc_fwd_bwd_bf16", logits, rows, V, ld, logits, dlogits, lab, ignore_index, float(smoothing), scale, loss_rows,
              correct)
    KL_ACC_HITS[0] += 1
    return loss_rows, correct


class _FusedLinearKLAcc(torch.autograd.Function):
    """_FusedLinearCE's shape for the Cosy head: per chunk of rows the bf16 logits of F.linear, the KL/accuracy kernel IN PLACE, then
    dh, dw and db from the overwritten buffer.  A denominator the HOST knows (the batch size, or n_valid when the caller counted the
    valid tokens while it built the targets) goes into the kernel's `scale`: d loss / d logits is then rounded to bf16 from the same
    fp32 value as in the torch chain, and backward multiplies by the incoming gradient alone (exact for the usual 1.0).  A valid-token
    count that exists on the device only stays there -- no host synchronisation -- and is folded into the incoming gradient in
    backward: d loss / d logits is then rounded before the division instead of after it (the same relative precision, other values).
    Either way dh [N, D], dw and db are kept in fp32 until backward (the GEMMs write fp32): each is scaled and rounded to bf16 ONCE,
    like the output of the parent's bf16 GEMMs."""

    @staticmethod
    def forward(ctx, hidden, weight, bias, labels, batch_size, smoothing, normalize_length, ignore_index, chunk, n_valid):
        N, V = hidden.shape[0], weight.shape[0]
        total = (labels != ignore_index).sum()
        host_denom = (n_valid or None) if normalize_length else batch_size   # nothing valid: the device route gives the pair's nan
        scale = 1.0 / host_denom if host_denom is not None else 1.0
        need = ctx.needs_input_grad
        loss = torch.zeros((), dtype=torch.float32, device=hidden.device)
        ncorrect = torch.zeros((), dtype=torch.int64, device=hidden.device)
        # fp32 out of the GEMMs: dh (4 N D bytes: small next to a chunk's [rows, V]) is rounded after the scale
        grads = _HeadGrads(need, hidden, weight, bias, fp32=True)
        for s, rows, _ in _chunk_plan(N, V, hidden.element_size(), True, chunk)[1]:
            h = hidden[s:s + rows]
            pd = F.linear(h, weight, bias)   # bf16 logits as nn.Linear gives them
            loss_rows, correct = _kl_acc_rows(pd, pd, labels[s:s + rows], V, ignore_index, smoothing, scale)
            loss += loss_rows.sum()
            ncorrect += correct.sum()
            grads.add(pd, h, s, s + rows)
        denom = total if normalize_length else batch_size
        ctx.save_for_backward(grads.dh, grads.dw, grads.db, total)
        ctx.on_device, ctx.wdtype, ctx.hdtype = host_denom is None, weight.dtype, hidden.dtype
        acc = ncorrect / total
        ctx.mark_non_differentiable(acc)
        return loss / denom, acc

    @staticmethod
    def backward(ctx, g, _gacc):
        dh, dw, db, total = ctx.saved_tensors
        g = g.float() / total if ctx.on_device else g.float()
        return _HeadGrads.scaled(dh, dw, db, g, ctx.hdtype, ctx.wdtype) + (None,) * 7


def fused_linear_kl_accuracy(hidden, labels, weight, bias, batch_size, smoothing, normalize_length, ignore_index=-1, chunk=None,
                             n_valid=None):
    """hidden [..., D], labels [...] -> (loss, acc) of the Cosy head: label_smoothing_kl and th_accuracy of F.linear(hidden, weight, bias)
    without the [rows, V] logits or any fp32 tensor of that size (bf16 CUDA hidden / weight / bias, int64 labels: the HIP kernel on one
    chunk of bf16 logits at a time).  Anything else computes the same two values from materialised logits.  batch_size: the denominator
    when normalize_length is false.  chunk: rows per round of head GEMMs (None: auto_chunk).  n_valid (optional, a Python int): the
    number of labels != ignore_index when the caller knows it on the host; it only moves the division in front of the gradient's bf16
    rounding (see _FusedLinearKLAcc) and must be the true count."""
    D, V = hidden.shape[-1], weight.shape[0]
    h2, lab = hidden.reshape(-1, D), labels.reshape(-1)
    if not (_hip_gate(h2, lab, weight, bias) and 0 <= smoothing < 1):
        logits = F.linear(h2, weight, bias)
        loss = label_smoothing_kl(logits.unsqueeze(0), lab.unsqueeze(0), V, ignore_index, smoothing, normalize_length)   # "batch" of 1
        return loss if normalize_length else loss / batch_size, th_accuracy(logits, lab.unsqueeze(0), ignore_index)
    if chunk is None:
        chunk = auto_chunk(h2.shape[0], V, h2.element_size())
    return _FusedLinearKLAcc.apply(h2, weight, bias, lab, batch_size, float(smoothing), normalize_length, ignore_index, chunk, n_valid)


class _KLFromLogits(torch.autograd.Function):
    """The loss alone on logits the caller keeps: the kernel out of place (d loss / d logits into its own bf16 buffer, scale = 1).
    backward multiplies that buffer by the incoming gradient / denominator in fp32, a slab of rows at a time (the fp32 temporary is
    at most 256 MiB, never [rows, V]): unless that factor is a power of two, d loss / d logits is rounded to bf16 twice -- within one
    bf16 ulp of the fp32 value instead of half of one, an RMS rounding error of at most sqrt(2) times the single rounding's.  (One rounding would need the factor
    at launch time: a host read of a device scalar in every backward.)"""

    @staticmethod
    def forward(ctx, logits2, labels, batch_size, smoothing, normalize_length, ignore_index):
        total = (labels != ignore_index).sum()
        dlogits = torch.empty_like(logits2)
        loss_rows, _ = _kl_acc_rows(logits2, dlogits, labels, logits2.shape[1], ignore_index, smoothing)
        ctx.save_for_backward(dlogits, total)
        ctx.by_tokens, ctx.batch_size = bool(normalize_length), batch_size
        return loss_rows.sum() / (total if normalize_length else batch_size)

    @staticmethod
    def backward(ctx, g):
        dlogits, total = ctx.saved_tensors
        g = g.float() / (total if ctx.by_tokens else ctx.batch_size)
        out = torch.empty_like(dlogits)
        step = max(1, (1 << 26) // dlogits.shape[1])   # 2^26 fp32 elements per slab
        for r in range(0, dlogits.shape[0], step):
            out[r:r + step] = dlogits[r:r + step].float() * g
        return out, None, None, None, None, None


def label_smoothing_kl_fused(logits, target, size, padding_idx, smoothing, normalize_length=False):
    """label_smoothing_kl with the fp32 chain replaced by the HIP kernel where it applies (bf16 CUDA logits, int64 target); the logits
    are left as they are."""
    x, t = logits.reshape(-1, size), target.reshape(-1)
    if not (_hip_gate(x, t) and 0 <= smoothing < 1 and x.is_contiguous()):
        return label_smoothing_kl(logits, target, size, padding_idx, smoothing, normalize_length)
    return _KLFromLogits.apply(x, t, logits.shape[0], float(smoothing), normalize_length, padding_idx)


# ---- held-out evaluation ---------------------------------------------------------------------------------
EVAL_HITS = [0]   # launches of rwkv7_head_eval_bf16 (one per chunk): how a test sees which route a call took
EVAL_CE, EVAL_KL = 0, 1   # `kind` of rwkv7_head_eval_bf16: cross-entropy with label smoothing / the Cosy label-smoothing KL
EVAL_CHUNK_ROWS = int(os.environ.get("RWKV7_EVAL_CHUNK_ROWS", "0"))   # rows per chunk where the caller names none (0: auto_chunk)


@contextlib.contextmanager
def eval_mode(module):
    """module.eval() under torch.no_grad() for the block; the previous mode is restored afterwards.  Dropout draws nothing in eval
    mode, so the host and device random streams are where they were."""
    was_training = module.training
    module.eval()
    try:
        with torch.no_grad():
            yield
    finally:
        module.train(was_training)


def scored_forward(fn, *tensors):
    """fn(*tensors) as the scores see it, differentiable all the same: the pass runs under no_grad now -- the kernels, and so the bits,
    of eval_metrics / score, whose backbone chooses other (fused training) nodes when autograd is on -- and once more with autograd
    when backward arrives (torch.utils.checkpoint in its re-entrant form: the host and device random streams of the first pass are
    replayed for the second and put back afterwards).  The price is one more forward pass of fn.  Gradients reach fn's parameters and
    the tensors given here through .backward() only (torch.autograd.grad on the result is not supported by that form).  Without
    autograd it is fn(*tensors)."""
    if not torch.is_grad_enabled():
        return fn(*tensors)
    from torch.utils.checkpoint import checkpoint
    tape = torch.zeros((), requires_grad=True)   # puts the node on the tape even if no tensor of the batch requires a gradient
    return checkpoint(lambda _tape, *t: fn(*t), tape, *tensors, use_reentrant=True)


def _eval_rows_torch(logits, labels, ignore_index, kind, smoothing):
    """The two row formulas of rwkv7_head_eval_bf16 in torch, fp32 from the logits as given: (loss_rows fp32, correct_rows bool)."""
    x = logits.float()
    V = x.shape[1]
    valid = labels != ignore_index
    y = labels.clamp(min=0).unsqueeze(1)
    lse = torch.logsumexp(x, dim=1)
    xy = x.gather(1, y).squeeze(1)
    if kind == EVAL_CE:
        per = lse - xy
        if smoothing > 0:
            per = (1 - smoothing) * per + smoothing * (lse - x.mean(dim=1))
    else:
        per = -(1 - smoothing) * (xy - lse)
        if smoothing > 0:
            C = (1 - smoothing) * math.log(1 - smoothing) + smoothing * math.log(smoothing / (V - 1))
            per = per + C - smoothing / (V - 1) * ((x.sum(dim=1) - xy) - (V - 1) * lse)
    correct = (x.argmax(dim=1) == labels) & valid   # torch.argmax: the lowest index among the maxima
    return per.masked_fill(~valid, 0.0), correct


def _grad_rows_torch(logits, labels, smoothing, row_scale, row_reg=None):
    """d (row loss) / d logits of the cross-entropy with label smoothing in torch, fp32 [rows, V] from fp32 logits: (softmax - smoothed
    one-hot) * row_scale[row]; row_scale fp32 [rows] carries the upstream scale and the 0 of an ignored row.
    row_reg: None, or (k, a, cm) per row -- rwkv7_ce_reg_fwd_bwd_bf16's regularisers: softmax_j becomes softmax_j k + [j == a] cm."""
    p = torch.softmax(logits, dim=-1)
    if row_reg is not None:
        k, a, cm = row_reg
        p = p * k.unsqueeze(1)
        p.scatter_add_(1, a.unsqueeze(1), cm.unsqueeze(1))
    if smoothing > 0:
        p = p - smoothing / logits.shape[-1]
    p.scatter_add_(1, labels.clamp(min=0).unsqueeze(1), torch.full_like(p[:, :1], -(1 - smoothing)))
    return p * row_scale.unsqueeze(1)


def _eval_chunks(hidden, labels, weight, bias, ignore_index, kind, smoothing, chunk, *, align=1, overlap_last=False, out=None):
    """The forward-only chunk walk under fused_linear_eval and _score_rows: yields (hip, loss_rows fp32 [rows], correct_rows [rows]) of
    F.linear(hidden, weight, bias) for one chunk of rows after the other; hip: which route the call takes.
    HIP route (_hip_gate): the head GEMM into ONE reused bf16 buffer of [chunk, ld] logits (ld = V rounded up to 16-byte rows), then
    rwkv7_head_eval_bf16 on it (correct_rows int32).  Anything else: _eval_rows_torch of the chunk's logits (correct_rows bool).
    chunk, align, overlap_last: the walk (_chunk_plan).
    out: None -- on the HIP route the yielded rows live in chunk-sized buffers that the next round overwrites; or full-length
    (loss_rows fp32 [N], correct_rows int32 [N]), which every round fills at its rows' positions (the kernel writes there directly)."""
    if kind not in (EVAL_CE, EVAL_KL) or not 0 <= smoothing < 1:
        raise ValueError(f"head evaluation: kind must be 0 (CE) or 1 (KL) and smoothing in [0, 1), got {kind}, {smoothing}")
    D, V = hidden.shape[-1], weight.shape[0]
    h2, lab = hidden.reshape(-1, D), labels.reshape(-1)
    N, dev = h2.shape[0], h2.device
    hip = _hip_gate(h2, lab, weight, bias)
    chunk, walk = _chunk_plan(N, V, h2.element_size(), hip, chunk, align, overlap_last)
    whole = out is not None
    if hip:
        _check_labels(lab, V, ignore_index)
        buf, wt = _logits_buffer(chunk, weight)
        if not whole:
            out = (torch.empty(chunk, dtype=torch.float32, device=dev), torch.empty(chunk, dtype=torch.int32, device=dev))
        lab = lab.contiguous()
    for s, rows, _ in walk:
        h, lb = h2[s:s + rows], lab[s:s + rows]
        if hip:
            o = s if whole else 0
            per, ok = out[0][o:o + rows], out[1][o:o + rows]
            _fill_logits(buf, h, wt, bias)
            _lib.call("rwkv7_head_eval_bf16", buf, rows, V, buf.stride(0), buf, lb, ignore_index, kind, float(smoothing), per, ok,
                      None)
            EVAL_HITS[0] += 1
        else:
            per, ok = _eval_rows_torch(F.linear(h, weight, bias), lb, ignore_index, kind, smoothing)
            if whole:
                out[0][s:s + rows] = per
                out[1][s:s + rows] = ok
        yield hip, per, ok


@torch.no_grad()
def fused_linear_eval(hidden, labels, weight, bias, ignore_index, kind, smoothing=0.0, chunk=None):
    """Forward-only metrics of a head: hidden [..., D], labels [...] -> device tensors (loss_sum fp64 [1], n_valid int64 [1],
    n_correct int64 [1]) of F.linear(hidden, weight, bias): the sum over the valid rows of the head's per-row training loss (kind
    EVAL_CE: cross-entropy with label smoothing, as fused_linear_cross_entropy; EVAL_KL: the Cosy label-smoothing KL, as
    fused_linear_kl_accuracy), the number of labels != ignore_index, and the number of valid rows whose argmax (lowest index among the
    maxima) is the label.  No autograd, no host synchronisation.
    bf16 CUDA hidden / weight / bias with int64 labels: chunk by chunk over the rows, the head GEMM into ONE reused bf16 buffer of
    [chunk, ld] logits (ld = V rounded up to 16-byte rows), then rwkv7_head_eval_bf16 on it -- nothing larger than chunk x ld logits is
    ever held, and the per-row losses are bit for bit those of the training kernels.  Anything else: the same values from fp32 logits
    in torch, chunk by chunk as well.  chunk: rows per round (None: EVAL_CHUNK_ROWS if set, else auto_chunk)."""
    lab = labels.reshape(-1)
    loss_sum = torch.zeros(1, dtype=torch.float64, device=hidden.device)
    n_correct = torch.zeros(1, dtype=torch.int64, device=hidden.device)
    n_valid = (lab != ignore_index).sum().reshape(1)
    for _, per, ok in _eval_chunks(hidden, lab, weight, bias, ignore_index, kind, smoothing, chunk):
        loss_sum += per.sum(dtype=torch.float64)   # chunk by chunk: loss_sum's bits depend on this order
        n_correct += ok.sum()
    return loss_sum, n_valid, n_correct


# ---- per-utterance scores -----------------------------------------------------------------------------------
SCORE_HITS = [0]   # launches of rwkv7_seq_scores_f32 (one per call): how a test sees which route a call took
SCORE_KEYS = ("loss_sum", "tokens", "correct", "worst_loss", "worst_row")
SCORE_CHUNK_ALIGN = 64   # HIP route: rows per head GEMM call are a multiple of this (see _score_rows)


def _score_rows(hidden, labels, weight, bias, ignore_index, kind, smoothing, chunk):
    """(loss_rows fp32 [N], correct_rows int32 [N], labels int64 [N] contiguous, hip) of F.linear(hidden, weight, bias) for ALL N rows,
    filled chunk by chunk by the walk fused_linear_eval uses (_eval_chunks): the same gate, the same GEMM into one reused [chunk, ld]
    bf16 buffer, rwkv7_head_eval_bf16 writing into slices of the full-length arrays (HIP route), or _eval_rows_torch per chunk.
    HIP route: the library GEMM takes another kernel, with another rounding of a few logits, for calls of a handful of rows (measured:
    up to 15; from 16 rows on a row's logits did not depend on the number of rows in the call).  So that the chunk size changes no bit
    of the scores, no call is that small: the chunk is rounded up to a multiple of SCORE_CHUNK_ALIGN = 64 rows, and a shorter last
    chunk is taken as the LAST `chunk` rows (it overlaps its predecessor, whose rows get the same values again)."""
    lab = labels.reshape(-1).contiguous()
    loss_rows = torch.empty(lab.numel(), dtype=torch.float32, device=hidden.device)
    correct_rows = torch.empty(lab.numel(), dtype=torch.int32, device=hidden.device)
    hip = False
    for hip, _, _ in _eval_chunks(hidden, lab, weight, bias, ignore_index, kind, smoothing, chunk, align=SCORE_CHUNK_ALIGN,
                                  overlap_last=True, out=(loss_rows, correct_rows)):
        pass   # every round has written its rows of the two arrays
    return loss_rows, correct_rows, lab, hip


def _seq_scores_torch(seq_start, loss_rows, correct_rows, labels, ignore_index):
    """rwkv7_seq_scores_f32's definitions in torch, sequence by sequence (seq_start is read on the host): the fp64 sum in row order
    (a cumulative sum), the counts, the maximum (NaN largest) and the first row that attains it."""
    st = seq_start.tolist()
    n_seq, dev = len(st) - 1, loss_rows.device
    loss_sum = torch.zeros(n_seq, dtype=torch.float64, device=dev)
    tokens = torch.zeros(n_seq, dtype=torch.int64, device=dev)
    correct = torch.zeros(n_seq, dtype=torch.int64, device=dev)
    worst_loss = torch.zeros(n_seq, dtype=torch.float32, device=dev)
    worst_row = torch.full((n_seq,), -1, dtype=torch.int64, device=dev)
    valid = labels != ignore_index
    for s in range(n_seq):
        idx = valid[st[s]:st[s + 1]].nonzero().squeeze(1)   # rows of the sequence that count, relative to its start
        if idx.numel() == 0:
            continue
        v = loss_rows[st[s]:st[s + 1]][idx]
        loss_sum[s] = v.double().cumsum(0)[-1]
        tokens[s] = idx.numel()
        correct[s] = correct_rows[st[s]:st[s + 1]][idx].sum()
        worst_loss[s] = v.max()
        worst_row[s] = idx[v.argmax()]   # torch.argmax: the lowest index among the maxima, a NaN counts as the largest
    return loss_sum, tokens, correct, worst_loss, worst_row


@torch.no_grad()
def fused_linear_score(hidden, labels, weight, bias, ignore_index, kind, smoothing=0.0, *, seq_start, chunk=None):
    """Per-sequence scores of a head: hidden [..., D], labels [...] (N rows once flattened), seq_start int64 [n_seq + 1] (non-decreasing
    row offsets into the flattened rows; sequence s owns rows seq_start[s] .. seq_start[s + 1] - 1; values are clamped to [0, N]) ->
    five device tensors of length n_seq over each sequence's rows with label != ignore_index:
      loss_sum fp64 (the sum of the head's per-row loss, the rows and formulas of fused_linear_eval), tokens int64, correct int64,
      worst_loss fp32 (the largest row loss), worst_row int64 (the first row, relative to the sequence's start, that attains it);
      a sequence without such a row gives 0, 0, 0, 0.0, -1.
    No autograd.  bf16 CUDA hidden / weight / bias with int64 labels: the chunked head GEMM and rwkv7_head_eval_bf16 of
    fused_linear_eval, each chunk writing its slice of full-length loss_rows / correct_rows (16 bytes per row with the labels; the
    logits are never kept), then ONE rwkv7_seq_scores_f32 launch whose summation order depends on a sequence's length alone -- no host
    synchronisation.  Anything else: the same definitions in torch (_eval_rows_torch per chunk, then a row-order fp64 sum and a
    max / first argmax per sequence; this route reads seq_start on the host).  chunk: as in fused_linear_eval; on the HIP route it is
    rounded up to a multiple of 64 rows and the last chunk overlaps its predecessor (_score_rows), so that the outputs are
    bit-identical for every chunk size as long as the library GEMM gives a row the same logits whatever the number of rows in the
    call -- observed from 16 rows per call on, not promised by the library."""
    if seq_start is None or seq_start.dim() != 1 or seq_start.numel() < 2:
        raise ValueError("fused_linear_score: seq_start must be a 1-D tensor of n_seq + 1 >= 2 row offsets")
    return _seq_scores(hidden, labels, weight, bias, ignore_index, kind, smoothing, seq_start, chunk)[0]


def _seq_scores(hidden, labels, weight, bias, ignore_index, kind, smoothing, seq_start, chunk):
    """fused_linear_score's body: (its five outputs, labels int64 [N] contiguous, seq_start as used -- int64 on the device, clamped
    to [0, N] -- and hip: which route the call took)."""
    loss_rows, correct_rows, lab, hip = _score_rows(hidden, labels, weight, bias, ignore_index, kind, smoothing, chunk)
    N, dev = lab.numel(), lab.device
    st = seq_start.to(device=dev, dtype=torch.int64).clamp(0, N).contiguous()   # the kernel checks no range: keep every read inside
    if not hip:
        return _seq_scores_torch(st, loss_rows, correct_rows, lab, ignore_index), lab, st, hip
    n_seq = st.numel() - 1
    loss_sum = torch.empty(n_seq, dtype=torch.float64, device=dev)
    tokens, correct, worst_row = (torch.empty(n_seq, dtype=torch.int64, device=dev) for _ in range(3))
    worst_loss = torch.empty(n_seq, dtype=torch.float32, device=dev)
    _lib.call("rwkv7_seq_scores_f32", loss_rows, n_seq, st, loss_rows, correct_rows, lab, ignore_index, loss_sum, tokens, correct,
              worst_loss, worst_row)
    SCORE_HITS[0] += 1
    return (loss_sum, tokens, correct, worst_loss, worst_row), lab, st, hip


def padded_seq_start(B, T, device):
    """seq_start of a padded [B, T] batch flattened row-major: sequence b is the rows b T .. (b + 1) T - 1."""
    return torch.arange(B + 1, dtype=torch.int64, device=device) * T


# ---- per-sequence log-probabilities under autograd ---------------------------------------------------------
SEQLP_HITS = [0]   # launches of rwkv7_ce_seq_bwd_bf16 (one per chunk of a backward pass): how a test sees which route a call took


def _row_scales(seq_start, seq_scale, row0, rows):
    """rwkv7_ce_seq_bwd_bf16's lookup in torch, on the device: fp32 [rows], seq_scale of the sequence of rows row0 .. row0 + rows - 1
    (the largest s with seq_start[s] <= row), 0 for a row in front of seq_start[0] or at / behind seq_start[-1]."""
    r = torch.arange(row0, row0 + rows, dtype=torch.int64, device=seq_start.device)
    s = torch.searchsorted(seq_start, r, right=True) - 1   # the largest index (of n_seq + 1 offsets) with seq_start[s] <= row
    inside = (s >= 0) & (r < seq_start[-1])
    return torch.where(inside, seq_scale[s.clamp(0, seq_scale.numel() - 1)], torch.zeros_like(seq_scale[:1]))


class _FusedLinearSeqLogprob(torch.autograd.Function):
    """Forward: fused_linear_score's loss_sum, negated (no logits kept: hidden, labels and seq_start are what backward needs beside
    the head's own parameters).  Backward: the head GEMM once more, chunk by chunk along the forward's walk, each chunk's logits
    turned in place into (softmax - onehot) * (-g[sequence of the row]) and fed to the three gradient GEMMs."""

    @staticmethod
    def forward(ctx, hidden, weight, bias, labels, seq_start, ignore_index, kind, chunk):
        (loss_sum, *_), lab, st, hip = _seq_scores(hidden, labels, weight, bias, ignore_index, kind, 0.0, seq_start, chunk)
        ctx.save_for_backward(hidden, weight, bias, lab, st)
        ctx.hip, ctx.ignore_index, ctx.chunk = hip, ignore_index, chunk
        return -loss_sum

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        hidden, weight, bias, lab, st = ctx.saved_tensors
        need, hip, ignore_index = ctx.needs_input_grad, ctx.hip, ctx.ignore_index
        N, V = hidden.shape[0], weight.shape[0]
        n_seq = st.numel() - 1
        seq_scale = (-g).float().contiguous()   # d(-loss_sum[s]) / d(row loss) = -1: the kernel's gradient is the loss's
        grads = _HeadGrads(need, hidden, weight, bias)
        chunk, walk = _chunk_plan(N, V, hidden.element_size(), hip, ctx.chunk, SCORE_CHUNK_ALIGN, True)
        if hip:
            buf, wt = _logits_buffer(chunk, weight)
        for s, rows, skip in walk:   # an overlapping last chunk contributes the rows behind its first `skip` only
            h, lo = hidden[s:s + rows], s + skip
            if hip:
                logits = _fill_logits(buf, h, wt, bias)
                _lib.call("rwkv7_ce_seq_bwd_bf16", buf, rows - skip, V, buf.stride(0), buf[skip:], lab[lo:], ignore_index, lo, n_seq,
                          st, seq_scale, None)
                SEQLP_HITS[0] += 1
                grads.add(logits[skip:], h[skip:], lo, s + rows)
            else:
                lb = lab[s:s + rows]
                p = _grad_rows_torch(F.linear(h, weight, bias).float(), lb, 0.0,
                                     _row_scales(st, seq_scale, s, rows) * (lb != ignore_index))
                grads.add(p.to(hidden.dtype), h, s, s + rows, p)
        return (grads.dh, grads.dw.to(weight.dtype) if need[1] else None, grads.db.to(bias.dtype) if grads.db is not None else None,
                None, None, None, None, None)


def seq_token_counts(labels, ignore_index, seq_start):
    """int64 [n_seq] on the labels' device: the number of labels != ignore_index among each sequence's rows (fused_linear_score's
    `tokens`, from a running count of the flattened labels: no host read)."""
    lab = labels.reshape(-1)
    st = seq_start.to(device=lab.device, dtype=torch.int64).clamp(0, lab.numel())
    run = torch.cat((torch.zeros(1, dtype=torch.int64, device=lab.device), (lab != ignore_index).cumsum(0)))
    return (run[st[1:]] - run[st[:-1]]).clamp(min=0)   # a decreasing pair is an empty sequence


def fused_linear_seq_logprob(hidden, labels, weight, bias, ignore_index, *, seq_start, chunk=None, kind=EVAL_CE):
    """Per-sequence sum of log-probabilities of a head under autograd: hidden [..., D], labels [...] (N rows once flattened), seq_start
    as in fused_linear_score -> fp64 [n_seq], sum over the sequence's rows with label != ignore_index of log softmax(F.linear(hidden,
    weight, bias))[label]; differentiable with respect to hidden, weight and bias, with any upstream gradient per sequence (fp64 or
    fp32 [n_seq]).
    Forward: fused_linear_score's loss_sum with smoothing 0, negated -- the same rows, route, chunk walk and launches, so on either
    route the value is bit for bit -fused_linear_score(..., kind, 0.0)[0].  kind: whose row reduction forms the value, EVAL_CE (the
    cross-entropy kernels') or EVAL_KL (the Cosy KL kernel's, which at smoothing 0 is the same -log p in another summation order:
    the Cosy heads pass it so that their value is their own score's).  Nothing of size [N, V] is kept for backward.
    Backward, bf16 CUDA hidden / weight / bias with int64 labels: per chunk of the forward's walk the head GEMM into one reused
    [chunk, ld] bf16 buffer, rwkv7_ce_seq_bwd_bf16 on it in place (the scale -g[s] of the row's sequence applied in fp32 before the
    one bf16 rounding; seq_start and the scales stay on the device: no host synchronisation), then dh = pd W, dW += (pd^T h).float(),
    db += column sums.  An overlapping last chunk contributes only the rows its predecessor did not cover.  Gradients are NOT
    bit-identical across chunk sizes (dW's fp32 sum over chunks).  Anything else: the same definitions from fp32 logits per chunk
    in torch."""
    if seq_start is None or seq_start.dim() != 1 or seq_start.numel() < 2:
        raise ValueError("fused_linear_seq_logprob: seq_start must be a 1-D tensor of n_seq + 1 >= 2 row offsets")
    D = hidden.shape[-1]
    return _FusedLinearSeqLogprob.apply(hidden.reshape(-1, D), weight, bias, labels.reshape(-1), seq_start, ignore_index, kind, chunk)


# ---- token-level clipped policy gradient (GRPO / PPO-clip) ----------------------------------------------------
POLICY_HITS = [0]   # launches of rwkv7_ce_policy_fwd_bwd_bf16 (one per chunk of a forward pass): how a test sees which route a call took


def group_advantages(rewards, group_size, eps=1e-6):
    """GRPO's group-relative advantages: rewards [G * group_size] (the candidates of one prompt are neighbours) ->
    (r - mean_group) / (std_group + eps) in the rewards' floating dtype (fp32 for anything else), std the population standard
    deviation of the group.  A group of equal rewards gives zeros."""
    r = torch.as_tensor(rewards)
    if not r.is_floating_point():
        r = r.float()
    if group_size < 1 or r.dim() != 1 or r.numel() % group_size != 0:
        raise ValueError(f"group_advantages: {tuple(r.shape)} rewards do not form groups of {group_size}")
    g = r.reshape(-1, group_size)
    c = g - g.mean(dim=1, keepdim=True)
    return (c / (c.square().mean(dim=1, keepdim=True).sqrt() + eps)).reshape(-1)


def _row_sequences(seq_start, row0, rows):
    """(s, inside) of rows row0 .. row0 + rows - 1: the sequence index as the head kernels look it up (the largest s with
    seq_start[s] <= row, clamped into [0, n_seq - 1]) and whether the row lies in [seq_start[0], seq_start[-1])."""
    r = torch.arange(row0, row0 + rows, dtype=torch.int64, device=seq_start.device)
    s = torch.searchsorted(seq_start, r, right=True) - 1
    return s.clamp(0, seq_start.numel() - 2), (s >= 0) & (r < seq_start[-1])


def _policy_rows_torch(x, labels, ignore_index, s, inside, adv, seq_w, old, ref, lo, hi, beta):
    """rwkv7_ce_policy_fwd_bwd_bf16's row formulas in torch from fp64 logits x [rows, V]: (lp, l_t, kl, clipped) fp32 [rows] and the
    row's coefficient sc fp64 [rows], zero on ignored rows and on rows outside every sequence.  Like the kernel's closing arithmetic
    this runs in fp64: a rounding of lp (a number of size log V) is a relative error of the whole row's gradient, and coefficients of
    both signs cancel in dW and db.  old / ref: the rows' entries; s, inside: _row_sequences."""
    on = inside & (labels != ignore_index)
    lp = x.gather(1, labels.clamp(min=0).unsqueeze(1)).squeeze(1) - torch.logsumexp(x, dim=1)
    A, rho = adv.double()[s], torch.exp(lp - old.double())
    s1, s2 = rho * A, rho.clamp(lo, hi) * A
    take1 = ~(s1 > s2)   # ties are active; a NaN stays a NaN, as torch.minimum keeps it
    loss, coef = -torch.where(take1, s1, s2), torch.where(take1, s1, torch.zeros_like(s1))
    kl = torch.zeros_like(lp)
    if ref is not None:
        d = ref.double() - lp
        e = torch.exp(d)
        kl = e - d - 1   # the k3 estimator of KL(policy || reference)
        loss, coef = loss + beta * kl, coef - beta * (1 - e)
    zero = torch.zeros_like(lp)
    return tuple(torch.where(on, v, zero).float() for v in (lp, loss, kl, (~take1).double())) + (torch.where(on, seq_w.double()[s] * coef, zero),)


class _FusedLinearPolicy(torch.autograd.Function):
    """_FusedLinearCE's shape for the clipped policy objective: d loss / d logits is written in the FORWARD chunk walk (a row's
    coefficient depends on its own log p(label) and on data known before the launch), the three gradient GEMMs run there too, and
    backward applies the one upstream scalar.  The walk is _FusedLinearSeqLogprob's: one reused [chunk, ld] logits buffer, an
    overlapping last chunk that contributes only the rows its predecessor did not cover."""

    @staticmethod
    def forward(ctx, hidden, weight, bias, labels, seq_start, adv, seq_w, old_logp, ref_logp, ignore_index, eps_lo, eps_hi, beta, chunk):
        N, V = hidden.shape[0], weight.shape[0]
        lo, hi = 1.0 - eps_lo, 1.0 + eps_hi
        dev = hidden.device
        lab = labels.contiguous()
        st = seq_start.to(device=dev, dtype=torch.int64).clamp(0, N).contiguous()   # the kernel checks no range: keep every read inside
        n_seq = st.numel() - 1
        adv, seq_w, old = (t.to(device=dev, dtype=torch.float32).contiguous() for t in (adv, seq_w, old_logp))
        ref = None if ref_logp is None else ref_logp.to(device=dev, dtype=torch.float32).contiguous()
        hip = _hip_gate(hidden, lab, weight, bias)
        need = ctx.needs_input_grad
        grads = _HeadGrads(need, hidden, weight, bias)
        stats = torch.empty(4, N, dtype=torch.float32, device=dev)   # lp, l_t, kl, clipped of every row
        if chunk is None and not hip:
            # this node's torch route holds fp64 logits, an fp64 softmax and the copy in the hidden dtype: 24 bytes per logit, where
            # _chunk_plan budgets the neighbours' fp32 pair
            chunk = EVAL_CHUNK_ROWS or auto_chunk(N, V, 24)
        chunk, walk = _chunk_plan(N, V, hidden.element_size(), hip, chunk, SCORE_CHUNK_ALIGN, True)
        if hip:
            _check_labels(lab, V, ignore_index)
            buf, wt = _logits_buffer(chunk, weight)
        else:
            w64, b64 = weight.double(), None if bias is None else bias.double()
        for s, rows, skip in walk:   # an overlapping last chunk contributes the rows behind its first `skip` only
            h, r0 = hidden[s:s + rows], s + skip
            if hip:
                logits = _fill_logits(buf, h, wt, bias)
                _lib.call("rwkv7_ce_policy_fwd_bwd_bf16", buf, rows - skip, V, buf.stride(0), buf[skip:], lab[r0:], ignore_index, r0,
                          n_seq, st, adv, seq_w, old, ref, eps_lo, eps_hi, beta, stats[0, r0:], stats[1, r0:], stats[2, r0:],
                          stats[3, r0:])
                POLICY_HITS[0] += 1
                grads.add(logits[skip:], h[skip:], r0, s + rows)
            else:
                # fp64 logits: rho = exp(lp - old) turns an ABSOLUTE error of the logits into a relative error of the row's gradient
                logits = F.linear(h.double(), w64, b64)
                lb = lab[s:s + rows]
                sq, inside = _row_sequences(st, s, rows)
                *rows4, sc = _policy_rows_torch(logits, lb, ignore_index, sq, inside, adv, seq_w, old[s:s + rows],
                                                None if ref is None else ref[s:s + rows], lo, hi, beta)
                stats[:, s:s + rows] = torch.stack(rows4)
                if need[0] or need[1]:
                    p = _grad_rows_torch(logits, lb, 0.0, sc)
                    grads.add(p.to(hidden.dtype), h, s, s + rows, p)
        sq, inside = _row_sequences(st, 0, N)
        row_w = torch.where(inside & (lab != ignore_index), seq_w[sq], torch.zeros_like(seq_w[:1]))
        loss = (stats[1].double() * row_w.double()).sum()
        ctx.save_for_backward(grads.dh, grads.dw, grads.db)
        ctx.hdtype, ctx.wdtype = hidden.dtype, weight.dtype
        lp, kl, clipped = stats[0], stats[2], stats[3]
        ctx.mark_non_differentiable(lp, kl, clipped)
        return loss, lp, kl, clipped

    @staticmethod
    def backward(ctx, g, *_):
        dh, dw, db = ctx.saved_tensors
        return _HeadGrads.scaled(dh, dw, db, g.float(), ctx.hdtype, ctx.wdtype) + (None,) * 11


def fused_linear_policy(hidden, labels, weight, bias, ignore_index, *, seq_start, adv, seq_w, old_logp, ref_logp=None, clip=(0.2, 0.2),
                        kl_beta=0.0, chunk=None):
    """The token-level clipped policy objective of a head (PPO-clip / GRPO) under autograd: hidden [..., D], labels [...] (N rows once
    flattened), seq_start as in fused_linear_score (n_seq sequences), adv and seq_w [n_seq] (a sequence's advantage and the weight of
    each of its rows), old_logp and ref_logp [N] (the sampling policy's and a frozen reference's log p(label) of every row; entries of
    ignored rows and of rows outside every sequence are never used) -> (loss, {"logp", "kl", "clipped"}).
    With lp = log softmax(F.linear(hidden, weight, bias))[label] of a row t of sequence s that counts (label != ignore_index):
        rho = exp(lp - old_logp[t]);  s1 = rho adv[s];  s2 = clamp(rho, 1 - clip[0], 1 + clip[1]) adv[s]
        l_t = -min(s1, s2) [+ kl_beta (exp(d) - d - 1),  d = ref_logp[t] - lp,  with ref_logp: the k3 estimator of the KL]
        loss = sum_t seq_w[s] l_t   (fp64 on the device), differentiable with respect to hidden, weight and bias.
    The dict holds detached fp32 [N] vectors, 0 on rows that do not count: logp = lp, kl, clipped = 1.0 where the clipped branch is the
    minimum (no policy gradient flows through that row; at a tie the unclipped branch is taken, as torch.minimum's gradient does).
    Without ref_logp no KL term exists whatever kl_beta says.
    bf16 CUDA hidden / weight / bias with int64 labels: per chunk of rows the head GEMM into ONE reused [chunk, ld] bf16 buffer, then
    rwkv7_ce_policy_fwd_bwd_bf16 turns it in place into d loss / d logits (the row's coefficient in fp64 from its fp32 lp, applied in
    fp32 before the one bf16 rounding) and writes the row's statistics, then dh = pd W, dW += (pd^T h).float(), db += column sums;
    backward multiplies by the upstream scalar.  Nothing of size [N, V] is kept and nothing is read on the host.  The chunk is
    rounded up to a multiple of 64 rows and a shorter last chunk overlaps its predecessor, contributing only the rows that one did not
    cover.  Gradients are NOT bit-identical across chunk sizes (dW's fp32 sum over chunks).  Anything else: the same definitions in
    torch per chunk, from fp64 logits (a row's rows and coefficient in fp64, rounded once to the hidden dtype)."""
    if seq_start is None or seq_start.dim() != 1 or seq_start.numel() < 2:
        raise ValueError("fused_linear_policy: seq_start must be a 1-D tensor of n_seq + 1 >= 2 row offsets")
    D = hidden.shape[-1]
    h2, lab = hidden.reshape(-1, D), labels.reshape(-1)
    n_seq, N = seq_start.numel() - 1, lab.numel()
    eps_lo, eps_hi = float(clip[0]), float(clip[1])
    if not (0.0 <= eps_lo < 1.0 and eps_hi >= 0.0):
        raise ValueError(f"fused_linear_policy: clip must be (eps_lo in [0, 1), eps_hi >= 0), got {clip}")
    if adv.numel() != n_seq or seq_w.numel() != n_seq or old_logp.numel() != N or (ref_logp is not None and ref_logp.numel() != N):
        raise ValueError(f"fused_linear_policy: {n_seq} sequences and {N} rows need adv / seq_w of {n_seq} and old_logp / ref_logp of "
                         f"{N} entries")
    loss, lp, kl, clipped = _FusedLinearPolicy.apply(h2, weight, bias, lab, seq_start, adv.reshape(-1), seq_w.reshape(-1),
                                                     old_logp.reshape(-1), None if ref_logp is None else ref_logp.reshape(-1),
                                                     ignore_index, eps_lo, eps_hi, float(kl_beta), chunk)
    return loss, dict(logp=lp, kl=kl, clipped=clipped)


def policy_objective(hidden, labels, lm_head, ignore_index, seq_start, advantages, old_logps, ref_logps, clip, kl_beta, normalize):
    """policy_loss of the heads from the backbone's hidden states [B, T, D] (with autograd), the labels [B, T] and the utterances'
    seq_start: fused_linear_policy with the row weights of `normalize` ("sequence": 1 / (n_seq * tokens_s); "token": 1 / sum of
    tokens), formed on the device."""
    if normalize not in ("sequence", "token"):
        raise ValueError(f'policy_loss: normalize must be "sequence" or "token", got {normalize!r}')
    dev = hidden.device
    labels = labels.to(dev)
    n_seq = seq_start.numel() - 1
    adv = torch.as_tensor(advantages).to(device=dev, dtype=torch.float32).reshape(-1)
    old = torch.as_tensor(old_logps).to(device=dev, dtype=torch.float32).reshape(-1)
    ref = None if ref_logps is None else torch.as_tensor(ref_logps).to(device=dev, dtype=torch.float32).reshape(-1)
    if adv.numel() != n_seq or old.numel() != labels.numel() or (ref is not None and ref.numel() != labels.numel()):
        raise ValueError(f"policy_loss: {n_seq} utterances over {labels.numel()} rows need {n_seq} advantages and old_logps / ref_logps "
                         f"of {labels.numel()} entries, got {adv.numel()}, {old.numel()}" + ("" if ref is None else f", {ref.numel()}"))
    tokens = seq_token_counts(labels, ignore_index, seq_start).double()
    denom = tokens.clamp(min=1) * n_seq if normalize == "sequence" else tokens.sum().clamp(min=1).expand(n_seq)
    loss, rows = fused_linear_policy(hidden, labels, lm_head.weight, lm_head.bias, ignore_index, seq_start=seq_start, adv=adv,
                                     seq_w=(1.0 / denom).float(), old_logp=old, ref_logp=ref, clip=clip, kl_beta=kl_beta)
    lab = labels.reshape(-1)
    _, inside = _row_sequences(seq_start.to(device=dev, dtype=torch.int64).clamp(0, lab.numel()), 0, lab.numel())
    return dict(loss=loss, valid=inside & (lab != ignore_index), **rows)


@torch.no_grad()
def token_logprob_rows(hidden, labels, lm_head, ignore_index):
    """token_logprobs of the heads: fp32 [rows] log softmax(lm_head(hidden))[label], 0 on ignored rows -- _score_rows' cross-entropy
    row losses (the held-out evaluation walk; smoothing 0), negated."""
    loss_rows, _, lab, _ = _score_rows(hidden, labels.to(hidden.device), lm_head.weight, lm_head.bias, ignore_index, EVAL_CE, 0.0, None)
    return torch.where(lab != ignore_index, -loss_rows, torch.zeros_like(loss_rows))
