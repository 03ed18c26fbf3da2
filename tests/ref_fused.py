"""TEST REFERENCE (not product code): plain PyTorch restatement of the fused elementwise stages, used by
tests/test_fused_gpu.py (fp32 on CPU) and tests/test_fused_rows_gpu.py (fp64 on CPU, evaluated in row slabs) as the reference
for rwkvtts_amd/fused.py (the HIP kernels) and for their gradients via torch.autograd.
Formulas: model/llm/rwkv_s2s_single_ffn.py:160-195,224-229,251-276.

Every function computes in the dtype of its activation inputs (fp32 or fp64); parameters and masks are cast to it.
Where a kernel stores an intermediate in the tensor type and reads it back, the functions take `rt` (the tensor type) and round
at the same point, straight through (`ste_round`: rounded value forward, identity backward; `round_grad`: identity forward,
rounded gradient backward).  rt = None / torch.float32 rounds nothing."""
import torch
import torch.nn.functional as F


def ste_round(x, rt):
    """x rounded to `rt` in the forward pass, the identity in the backward pass."""
    if rt is None or rt == torch.float32 or rt == x.dtype:
        return x
    return x + (x.detach().to(rt).to(x.dtype) - x.detach())


class _RoundGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rt):
        ctx.rt = rt
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.rt).to(g.dtype), None


def round_grad(x, rt):
    """The identity whose backward rounds the gradient to `rt` (a gradient tensor a kernel stores in the tensor type)."""
    if rt is None or rt == torch.float32 or rt == x.dtype:
        return x
    return _RoundGrad.apply(x, rt)


def _shift(x, x_prev):
    """x_{t-1}; zeros (training, rwkv_s2s_single_ffn.py:162 ZeroPad2d) or the carried row at t = 0."""
    if x_prev is None:
        return F.pad(x, (0, 0, 1, -1))
    return torch.cat([x_prev.unsqueeze(1).to(x.dtype), x[:, :-1]], dim=1)


def token_shift_mix6(x, x_prev, x_r, x_w, x_k, x_v, x_a, x_g):
    """xx = shift(x) - x ; x + xx * x_?  for ? in r,w,k,v,a,g   (rwkv_s2s_single_ffn.py:162-169)."""
    return token_shift_mix(x, x_prev, (x_r, x_w, x_k, x_v, x_a, x_g))


def token_shift_mix(x, x_prev, params):
    """The same lerps for any number of coefficient vectors (3: the x_r, x_k, x_v of fused.mix_lora)."""
    xx = _shift(x, x_prev) - x
    return tuple(torch.addcmul(x, xx, p.reshape(1, 1, -1).to(x.dtype)) for p in params)


def token_shift_mix1(x, x_prev, x_k):
    """channel-mix input: x + (shift(x) - x) * x_k   (rwkv_s2s_single_ffn.py:225-227)."""
    xx = _shift(x, x_prev) - x
    return torch.addcmul(x, xx, x_k.reshape(1, 1, -1).to(x.dtype))


def relu_sq(x):
    """relu(x)^2   (rwkv_s2s_single_ffn.py:228)."""
    return torch.relu(x).square()


def tmix_prepare(w_pre, k, v, a_pre, v_pre, v_first, k_k, k_a, mask, H, is_layer0):
    """Everything between the projections and the scan (rwkv_s2s_single_ffn.py:172-190):
        w  = (-softplus(-w_pre) - 0.5) * mask
        k  = k * mask ; v = v * mask
        v  = v + (v_first - v) * sigmoid(v_pre)                    (layers > 0)
        a  = sigmoid(a_pre)
        kk = l2norm_per_head(k * k_k) * mask
        k2 = k * (1 + (a - 1) * k_a) ; v2 = v * mask
    returns w, k2, v2, -kk, kk * a   (the scan's w, k, v, a, b operands)."""
    B, T, D = k.shape
    k_k, k_a = k_k.reshape(1, 1, D).to(k.dtype), k_a.reshape(1, 1, D).to(k.dtype)
    if mask is not None:
        mask = mask.reshape(B, T, 1).to(k.dtype)
    w = -F.softplus(-w_pre) - 0.5
    if mask is not None:
        w, k, v = w * mask, k * mask, v * mask
    if not is_layer0:
        v = v + (v_first - v) * torch.sigmoid(v_pre)
    a = torch.sigmoid(a_pre)
    kk = F.normalize((k * k_k).reshape(B, T, H, -1), dim=-1, p=2.0).reshape(B, T, D)
    if mask is not None:
        kk = kk * mask
    k2 = k * (1 + (a - 1) * k_a)
    if mask is not None:
        v = v * mask
    return w.contiguous(), k2.contiguous(), v.contiguous(), (-kk).contiguous(), (kk * a).contiguous()


def tmix_post(y, r, k, v, g, gn_weight, gn_bias, r_k, H, eps):
    """After the scan (rwkv_s2s_single_ffn.py:192-195): GroupNorm over each head, the (r.k.r_k) v bonus, gate."""
    B, T, D = y.shape
    N = D // H
    dt = y.dtype
    yn = F.group_norm(y.reshape(B * T, D), H, gn_weight.reshape(-1).to(dt), gn_bias.reshape(-1).to(dt), eps).reshape(B, T, D)
    bonus = (r.reshape(B, T, H, N) * k.reshape(B, T, H, N) * r_k.reshape(1, 1, H, N).to(dt)).sum(-1, keepdim=True) * v.reshape(B, T, H, N)
    return (yn + bonus.reshape(B, T, D)) * g


def layer_norm(x, gamma, beta, eps):
    """LayerNorm over the last dim (rwkv_s2s_single_ffn.py:251-259 ln1 / ln2); beta may be None."""
    D = x.shape[-1]
    return F.layer_norm(x, (D,), gamma.reshape(-1).to(x.dtype), None if beta is None else beta.reshape(-1).to(x.dtype), eps)


def add_layer_norm(x, branch, gamma, beta, eps, rt=None):
    """(x1, h) = (x + branch, LayerNorm(x + branch)) (rwkv_s2s_single_ffn.py:262-276); the add is stored in the tensor type `rt`
    before it is normalised (elementwise.hip: "x1 = x + branch (rounded to T, as the separate add would)")."""
    x1 = x if branch is None else ste_round(x + branch, rt)
    return x1, layer_norm(x1, gamma, beta, eps)


def add_layer_norm_mix(x, branch, gamma, beta, eps, mask, params, rt=None):
    """add + LayerNorm -> token-shift lerps of h * mask, as the one-pass kernels compute it: x1 and h are rounded to the tensor type
    `rt` before they are used (elementwise.hip: "h is rounded to the tensor type before it is mixed, as the separate path stores
    it") and so is dh on the way back ("dh = g * mask, rounded to the tensor type as the separate mix_bwd kernel stores it").
    Returns (x1, outs, h): h (rounded, unmasked) is handed out so that a test can read dh from h.grad."""
    B, T, D = x.shape
    x1, h = add_layer_norm(x, branch, gamma, beta, eps, rt)
    h = ste_round(h, rt)
    hm = round_grad(h, rt)
    if mask is not None:
        hm = hm * mask.reshape(B, T, 1).to(x.dtype)
    return x1, token_shift_mix(hm, None, params), h


# ------------------------------------------------------------------------------------------------------
# the time-mix backward pair (fused._TmixCore.backward stages 1 and 3) as the gradient of one surrogate loss
# ------------------------------------------------------------------------------------------------------
def tmix_pair_loss(raw, par, cot, mask, H, eps, is_layer0, rt=None, stored=None, round_post_grads=False):
    """<post(y, r, k2, v2, g), dout> + <w, dw> + <r, dq> + <k2, dk> + <v2, dv> + <a_in, da> + <b_in, db> + <v_first, d_vf_next>
    with (w, k2, v2, a_in, b_in) = tmix_prepare(raw) and y a leaf.
      raw: dict r, w_pre, k, v, a_pre, g, y (+ v_pre, v_first unless layer 0); par: dict k_k, k_a, gn_weight, gn_bias, r_k;
      cot: dict dout, dw, dq, dk, dv, da, db (each a tensor or a list of tensors: several gradient sets are summed here) and
           optionally d_vf_next.
    Its gradients with respect to raw and par are what tmix_post_bwd followed by tmix_prepare_bwd_sum must return.
    Stored roundings (rwkv7_hip.h, fused._TmixCore): k2 and v2 leave tmix_prepare_fwd in the tensor type `rt` and tmix_post reads
    them back -- rounded here straight through, to `stored` = (k2, v2) as the forward kernel wrote them when given, so that a
    rounding that falls the other way in fp32 does not enter the comparison of the BACKWARD kernels; round_post_grads: the
    non-compact post backward stores its d_r, d_k2, d_v2 in the tensor type before the prepare backward adds them (round_grad);
    the compact post backward stores dt = dL/d(GroupNorm + bonus) in the tensor type and the prepare backward forms d_v2 +=
    dt * dot from it (round_grad on that product's path only: the per-head scalars dot and ds stay fp32)."""
    tot = lambda t: sum(t) if isinstance(t, (list, tuple)) else t
    B, T, D = raw["k"].shape
    N = D // H
    dtp = raw["k"].dtype
    w, k2, v2, a_in, b_in = tmix_prepare(raw["w_pre"], raw["k"], raw["v"], raw["a_pre"], raw.get("v_pre"), raw.get("v_first"),
                                         par["k_k"], par["k_a"], mask, H, is_layer0)
    if stored is not None:
        k2s = k2 + (stored[0].to(dtp) - k2.detach())
        v2s = v2 + (stored[1].to(dtp) - v2.detach())
    else:
        k2s, v2s = ste_round(k2, rt), ste_round(v2, rt)
    r = raw["r"]
    if round_post_grads:
        out = tmix_post(raw["y"], round_grad(r, rt), round_grad(k2s, rt), round_grad(v2s, rt), raw["g"], par["gn_weight"],
                        par["gn_bias"], par["r_k"], H, eps)
    else:
        # tmix_post with the bonus split so that the gradient reaching v2 through it is round(dt) * dot while ds = <dt, v2> is not
        yn = F.group_norm(raw["y"].reshape(B * T, D), H, par["gn_weight"].reshape(-1).to(dtp), par["gn_bias"].reshape(-1).to(dtp),
                          eps).reshape(B, T, D)
        dot = (r.reshape(B, T, H, N) * k2s.reshape(B, T, H, N) * par["r_k"].reshape(1, 1, H, N).to(dtp)).sum(-1, keepdim=True)
        v4 = v2s.reshape(B, T, H, N)
        bonus = round_grad(v4 * dot.detach(), rt) + (dot - dot.detach()) * v4.detach()
        out = (yn + bonus.reshape(B, T, D)) * raw["g"]
    loss = (out * cot["dout"]).sum() + (w * tot(cot["dw"])).sum() + (r * tot(cot["dq"])).sum() + (k2 * tot(cot["dk"])).sum() \
        + (v2 * tot(cot["dv"])).sum() + (a_in * tot(cot["da"])).sum() + (b_in * tot(cot["db"])).sum()
    if cot.get("d_vf_next") is not None and not is_layer0:
        loss = loss + (raw["v_first"] * cot["d_vf_next"]).sum()
    return loss


# ------------------------------------------------------------------------------------------------------
# evaluation in row slabs
# ------------------------------------------------------------------------------------------------------
def eval_in_slabs(fn, acts, params, douts, slab_seqs=1, probes=(), dtype=torch.float64, consts=None):
    """fn(acts, params) -> tuple of [B, T, ...] outputs, evaluated with its autograd gradients in slabs of `slab_seqs` whole
    sequences (the stages are independent from row to row apart from the token shift inside a sequence; parameter gradients add
    over slabs), so that the training shape needs a few GB of host memory.
      acts:   dict name -> [B, ...] tensor (sliced along dim 0; gradients for those with a floating dtype) or None
      params: dict name -> tensor shared by all slabs (gradients summed over slabs)
      douts:  list of [B, T, ...] cotangents, one per output (None: the output takes no gradient, e.g. a probe); douts = None:
              fn returns a scalar loss of the slab (the losses add over slabs)
      consts: dict name -> [B, ...] tensor, list of such tensors, or None: sliced and cast like acts, no gradients; fn finds them
              in its first argument next to acts
      probes: indices of outputs whose own .grad (the gradient that reaches them from the OTHER outputs) is returned too
    Returns (outs, act_grads, param_grads, probe_grads), everything in `dtype`."""
    B = next(v.shape[0] for v in acts.values() if v is not None)
    outs, agrads, pgrads, prgrads = None, {}, {}, {i: [] for i in probes}
    P = {k: v.to(dtype) for k, v in params.items()}
    for b0 in range(0, B, slab_seqs):
        sl = slice(b0, min(B, b0 + slab_seqs))
        a = {}
        for k_, v in acts.items():
            if v is None:
                a[k_] = None
            elif v.dtype.is_floating_point:
                a[k_] = v[sl].to(dtype).requires_grad_(True)
            else:
                a[k_] = v[sl]
        act_names = list(a)
        for k_, v in (consts or {}).items():
            a[k_] = [t[sl].to(dtype) for t in v] if isinstance(v, (list, tuple)) else (None if v is None else v[sl].to(dtype))
        p = {k_: v.clone().requires_grad_(True) for k_, v in P.items()}
        res = fn(a, p)
        res = tuple(res) if isinstance(res, (tuple, list)) else (res,)
        for i in probes:
            res[i].retain_grad()
        if douts is None:
            loss = res[0]
        else:
            loss = sum((o * d[sl].to(dtype)).sum() for o, d in zip(res, douts) if d is not None)
        loss.backward()
        if outs is None:
            outs = [[] for _ in res]
        for lst, o in zip(outs, res):
            lst.append(o.detach().reshape(1) if o.dim() == 0 else o.detach())
        for k_ in act_names:
            v = a[k_]
            if v is not None and v.dtype.is_floating_point:
                agrads.setdefault(k_, []).append(v.grad if v.grad is not None else torch.zeros_like(v))
        for k_, v in p.items():
            g = v.grad if v.grad is not None else torch.zeros_like(v)
            pgrads[k_] = g if k_ not in pgrads else pgrads[k_] + g
        for i in probes:
            prgrads[i].append(res[i].grad if res[i].grad is not None else torch.zeros_like(res[i]))
    return ([torch.cat(l) for l in outs], {k_: torch.cat(v) for k_, v in agrads.items()}, pgrads,
            {i: torch.cat(v) for i, v in prgrads.items()})
