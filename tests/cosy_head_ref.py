"""fp64 restatement of the Cosy head's row formulas (include/rwkv7_hip.h, rwkv7_kl_acc_fwd_bwd_bf16), shared by test_cosy_head.py and
test_cosy_head_gpu.py.  Written from the formulas, not from losses.label_smoothing_kl: the tests compare the two."""
import math

import torch


def entropy_constant(V, s):
    """C = sum_j t_j ln t_j of the target distribution, 0 ln 0 = 0."""
    return (1.0 - s) * math.log(1.0 - s) + (s * math.log(s / (V - 1)) if s > 0 else 0.0)


def exact_rows(x, labels, s, ignore=-1):
    """x [rows, V] (any float dtype, taken as given) -> fp64 (loss_rows, dlogits with scale = 1, correct_rows int64, lse)."""
    x = x.double()
    rows, V = x.shape
    valid = labels != ignore
    y = labels.clamp(min=0)
    lse = torch.logsumexp(x, dim=1)
    xy = x.gather(1, y[:, None])[:, 0]
    loss = entropy_constant(V, s) - (1.0 - s) * (xy - lse) - s / (V - 1) * ((x.sum(1) - xy) - (V - 1) * lse)
    t = torch.full_like(x, s / (V - 1))
    t.scatter_(1, y[:, None], 1.0 - s)
    d = torch.exp(x - lse[:, None]) - t
    idx = torch.arange(V, device=x.device).expand(rows, V)
    first = torch.where(x == x.max(1, keepdim=True).values, idx, torch.full_like(idx, V)).min(1).values   # lowest index among the maxima
    correct = ((first == labels) & valid).long()
    return loss * valid, d * valid[:, None], correct, lse


def fp32_chain_rows(x, labels, s, ignore=-1):
    """label_smoothing_kl's per-row arithmetic in fp32 on the same logits (the chain the kernel replaces), before the final sum."""
    import torch.nn.functional as F
    V = x.shape[1]
    ign = labels == ignore
    t = labels.masked_fill(ign, 0)
    true_dist = torch.full_like(x, s / (V - 1), dtype=torch.float32)
    true_dist.scatter_(1, t.unsqueeze(1), 1.0 - s)
    kl = F.kl_div(torch.log_softmax(x.float(), dim=1), true_dist, reduction="none")
    return kl.masked_fill(ign.unsqueeze(1), 0).sum(1)
