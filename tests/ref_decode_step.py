"""TEST REFERENCE (not product code): plain fp64 PyTorch restatement of ONE decode step (T = 1) of the RWKV-7 stack, the
regime generator and the bars of tests/test_decode_step_parity_gpu.py (the HIP side is rwkvtts_amd/csrc/decode_step.hip) and of
tests/test_ref_decode_step.py (CPU: anchor against oracle/rwkv7_ref.py, generator guard, fault sensitivity).
Formulas: model/llm/rwkv_s2s_single_ffn.py:417-445, 482-506, 545-549 as restated in oracle/rwkv7_ref.py, in the order of the
phase list at the top of decode_step.hip.  No kernel code: matmuls, elementwise torch, nothing else.

ref_step(params, states, x_in, case, rounded) -> dict with, per layer, the four observables the step publishes through the cache
it updates in place, the logits, the new states and (for failure messages only) the intermediates w, a, kk, k2, v, y.

    observable (layer l)                       dtype   pins
    att_x_prev[l] after the step               bf16    P0: residual sum of the previous layer's channel-mix, (LN0,) LN1
    att_kv[l] after the step                   fp32    P1 + P2 A-D: projections, low-rank branches, decay, a, value residual,
                                                       kk, k_k, k_a, the state update
    ffn_x_prev[l] after the step               bf16    P2 E + P3 + P4: y, GroupNorm, bonus, gate, output projection, LN2
    att_x_prev[l + 1] / logits (last layer)    bf16/fp32  P5 + P6: channel-mix lerp, key, relu^2, value; tail norm, head (+ bias)

rounded = False: fp64 throughout -- the reference every bar is measured against.
rounded = True: the same with a bf16 round-to-nearest-even where the kernel's contract stores bf16, and nowhere else:

    point                                               kernel buffer            phase
    pre_norm output of layer 0 (the residual stream)    registers -> xb          P0 (layer 0)
    h = LayerNorm1(x): lerp input and att_x_prev        att_x_prev               P0
    the six token-shift lerps r, w, k, v, a, g          mixed                    P0
    low-rank hidden vectors after their activation      LDS hid                  P2 step A
    head-phase output row (y_norm + bonus) * gate       yg                       P2 step E
    h = LayerNorm2(x): lerp input and ffn_x_prev        ffn_x_prev               P4
    the channel-mix lerp                                kx                       P4
    relu(key)^2                                         kact                     P5
    final normed row                                    hfin                     tail
r, k, v, v_first, the up projections, the partial sums and the residual stream after layer 0's pre_norm stay unrounded.

`fault` (tests/test_ref_decode_step.py only) plants ONE wrong formula of the kind a kernel gets wrong; see FAULTS.
"""
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

N = 64                      # head size
LN_EPS, GN_EPS = 1e-5, 64e-5
U24 = 2.0 ** -24            # fp32 unit round-off
W_ABS_ERR = 6e-8            # |error| of the decay exponent w that decode_step.hip's comment on softplus_d declares

REGIMES = ("trained_like", "max_decay", "no_decay", "mixed_decay", "gates_saturated", "large_state_10x", "large_state_100x",
           "small_state", "fresh", "dead_head")

# single faults planted into the rounded reference: what a kernel of this shape gets wrong without a whole-model bar noticing
FAULTS = ("k_a_rot", "r_k_rot", "gn_w_rot", "gn_b_rot", "k_k_rot", "decay_no_tanh", "gate_no_sigmoid", "a_v_blocks_swapped",
          "decay_no_half", "gn_eps_1e-5", "v_first_prev_layer", "xprev_swapped", "lerp_reversed", "xprev_after_lerp",
          "head_bias_dropped", "kk_not_normalised")


@dataclass(frozen=True)
class Case:
    regime: str
    D: int
    B: int
    L: int
    ranks: Tuple[int, int, int, int]   # decay, a, value residual, gate
    F: int
    V: int
    bias: bool

    @property
    def H(self):
        return self.D // N

    @property
    def id(self):
        return f"{self.regime}-D{self.D}-B{self.B}-L{self.L}-R{'.'.join(map(str, self.ranks))}-F{self.F}-V{self.V}{'b' if self.bias else ''}"

    @property
    def seed(self):
        return sum(ord(c) * (i + 1) for i, c in enumerate(self.id)) % (2 ** 31)


def _c(regime, D, B, L, ranks, F=None, V=77, bias=False):
    return Case(regime, D, B, L, ranks, F or 4 * D, V, bias)


# The GPU test's case list.  Every regime at a small width and at the 0.4B width (D = 1024); every D with trained_like and a hard
# regime; B in {1, 2, 3, 31, 32}; L in {2, 3}; ranks distinct per branch; F in {4 D, 5 * 64, 8192}; V in {77, 8193} +- head bias.
CASES = (
    _c("trained_like", 64, 1, 2, (32, 64, 96, 128), bias=True),
    _c("mixed_decay", 64, 32, 3, (64, 32, 128, 96), F=320),
    _c("trained_like", 128, 2, 3, (64, 32, 96, 160)),
    _c("max_decay", 128, 3, 2, (32, 96, 64, 128), F=320, bias=True),
    _c("no_decay", 128, 31, 2, (96, 32, 64, 128), V=8193),
    _c("mixed_decay", 128, 1, 3, (32, 64, 96, 128), bias=True),
    _c("gates_saturated", 128, 3, 3, (64, 96, 32, 160)),
    _c("large_state_10x", 128, 2, 2, (32, 64, 96, 256), F=8192),
    _c("large_state_100x", 128, 1, 3, (96, 64, 32, 128), bias=True),
    _c("small_state", 128, 31, 2, (32, 96, 64, 128)),
    _c("fresh", 128, 32, 3, (64, 32, 96, 128), F=320),
    _c("dead_head", 128, 3, 3, (32, 64, 128, 96), bias=True),
    _c("trained_like", 768, 3, 2, (64, 32, 96, 128)),
    _c("gates_saturated", 768, 2, 3, (96, 64, 32, 160), F=320, bias=True),
    _c("trained_like", 1024, 32, 2, (64, 96, 32, 128), V=8193, bias=True),
    _c("max_decay", 1024, 31, 2, (96, 64, 32, 128)),
    _c("no_decay", 1024, 1, 2, (64, 32, 96, 128), F=320),
    _c("mixed_decay", 1024, 3, 3, (32, 64, 96, 160), bias=True),
    _c("gates_saturated", 1024, 2, 2, (64, 96, 32, 128)),
    _c("large_state_10x", 1024, 3, 2, (32, 64, 96, 128), F=320),
    _c("large_state_100x", 1024, 32, 2, (64, 32, 96, 128), bias=True),
    _c("small_state", 1024, 2, 2, (96, 64, 32, 128)),
    _c("fresh", 1024, 31, 2, (64, 96, 32, 128), V=8193),
    _c("dead_head", 1024, 1, 3, (32, 96, 64, 128), F=320, bias=True),
    _c("trained_like", 2048, 2, 2, (96, 64, 32, 256), F=8192),
    _c("mixed_decay", 2048, 31, 2, (128, 96, 64, 160), F=320, V=8193, bias=True),
    _c("trained_like", 4096, 3, 2, (256, 96, 32, 128), F=320),
    _c("dead_head", 4096, 3, 2, (32, 64, 96, 256), F=320),
)


def bf16_round(x):
    """round-to-nearest-even to bf16, returned in x's dtype"""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


# ----------------------------------------------------------------------------------------------------------------------------
# regime generator: parameters (rwkvfla key layout, bf16-valued fp32), states and the first input rows of a case
# ----------------------------------------------------------------------------------------------------------------------------
def make_case(case: Case):
    """-> params {key: fp32 tensor with bf16 values}, states [att_x_prev, att_kv, ffn_x_prev] * L (bf16-valued fp32 rows, fp32
    att_kv), ids [B] (distinct) of the first input rows.  Every per-channel vector is random and differs from head to head; every
    sequence has its own input row and its own state (except `fresh`, whose definition is the all-zero state)."""
    g = torch.Generator().manual_seed(case.seed)
    D, L, H, F, B, V = case.D, case.L, case.H, case.F, case.B, case.V
    reg = case.regime
    rnd = lambda *shape, std=1.0: torch.randn(*shape, generator=g) * std
    uni = lambda lo, hi, *shape: lo + (hi - lo) * torch.rand(*shape, generator=g)
    p = {}
    small = reg == "small_state"
    p["model.embeddings.weight"] = rnd(V, D, std=0.5e-3 if small else 0.5)
    s = 1.0 / math.sqrt(D)
    for i in range(L):
        pre = f"model.layers.{i}."
        r01, r10 = i / max(L - 1, 1), 1.0 - i / L
        ddd = torch.arange(D, dtype=torch.float32) / D
        lin = torch.arange(D, dtype=torch.float32) / max(D - 1, 1) - 0.5
        zig = ((torch.arange(D) % N).float() - (N - 1) / 2) / ((N - 1) / 2)
        zig = zig * zig.abs()
        www = -6 + 6 * (torch.arange(D, dtype=torch.float32) / max(D - 1, 1)) ** (1 + r01 ** 0.3)
        for nm in (("pre_norm",) if i == 0 else ()) + ("attn_norm", "ffn_norm"):
            p[pre + nm + ".weight"] = 1 + rnd(D, std=0.1)
            p[pre + nm + ".bias"] = rnd(D, std=0.1)
        at = pre + "attn."
        for nm, e in (("r", 0.2), ("w", 0.9), ("k", 0.7), ("v", 0.7), ("a", 0.9), ("g", 0.2)):
            p[at + f"x_{nm}"] = ((1.0 - torch.pow(ddd, e * r10)) + rnd(D, std=0.05)).view(1, 1, D)
        p[at + "k_k"] = 0.71 - lin * 0.1 + rnd(D, std=0.05)
        p[at + "k_a"] = uni(0.85, 1.2, D)
        p[at + "r_k"] = rnd(H, N, std=0.15)
        p[at + "r_proj.weight"] = rnd(D, D, std=s * (0.1 if small else 1.0))
        p[at + "k_proj.weight"] = rnd(D, D, std=s)
        p[at + "v_proj.weight"] = rnd(D, D, std=s * (0.03 if small else 1.0))
        p[at + "o_proj.weight"] = rnd(D, D, std=s)
        # decay bias per channel: the init curve, or one of the two ends of softplus_d
        w_tr = www + 0.5 + zig * 2.5 + rnd(D, std=0.3)
        w_max = uni(8.0, 24.0, D)      # w -> -0.5; beyond 16.6 the kernel's log(1 + e^u) rounds to 0
        w_no = uni(-26.0, -13.0, D)    # w_pre <= -12 with the branch's swing: decay factor 1 - O(1e-6) and below; u > 20 included
        if reg == "max_decay":
            w_bias = w_max
        elif reg == "no_decay":
            w_bias = w_no
        elif reg == "mixed_decay":
            pick = torch.randint(0, 3, (D,), generator=g)
            w_bias = torch.where(pick == 0, w_tr, torch.where(pick == 1, w_max, w_no))
        else:
            w_bias = w_tr
        a_bias = -0.19 + zig * 0.3 + lin * 0.4 + rnd(D, std=0.3)
        v_bias = 0.73 - lin * 0.4 + rnd(D, std=0.3)
        if reg == "gates_saturated":   # +-12 by channel, sign drawn per channel
            a_bias = torch.where(torch.rand(D, generator=g) < 0.5, -12.0, 12.0) + rnd(D, std=0.3)
            v_bias = torch.where(torch.rand(D, generator=g) < 0.5, -12.0, 12.0) + rnd(D, std=0.3)
        ranks = dict(zip("wavg", case.ranks))
        for nm, bias in (("w", w_bias), ("a", a_bias), ("v", v_bias), ("g", None)):
            if nm == "v" and i == 0:
                continue
            R = ranks[nm]
            # the gate branch has no bias: its sigmoid is saturated through the down projection (hidden values ~ N(0, 12^2))
            s0 = s * (12.0 if (reg == "gates_saturated" and nm == "g") else 1.0)
            p[at + f"{nm}_lora.lora.0.weight"] = rnd(R, D, std=s0)
            p[at + f"{nm}_lora.lora.2.weight"] = rnd(D, R, std=0.3 / math.sqrt(R))
            if bias is not None:
                p[at + f"{nm}_lora.lora.2.bias"] = bias
        p[at + "g_norm.weight"] = 1 + rnd(D, std=0.2)
        p[at + "g_norm.bias"] = rnd(D, std=0.2)
        if reg == "dead_head":
            hd = min(1, H - 1)
            p[at + "k_k"][hd * N:(hd + 1) * N] = 0.0
        ff = pre + "ffn."
        p[ff + "x_k"] = (1.0 - torch.pow(ddd, r10 ** 4)) + rnd(D, std=0.05)
        p[ff + "key.weight"] = rnd(F, D, std=s)
        p[ff + "value.weight"] = rnd(D, F, std=1.0 / math.sqrt(F))
    p["model.norm.weight"] = 1 + rnd(D, std=0.1)
    p["model.norm.bias"] = rnd(D, std=0.1)
    p["lm_head.weight"] = rnd(V, D, std=0.05)
    if case.bias:
        p["lm_head.bias"] = rnd(V, std=0.5)
    p = {k: bf16_round(v).contiguous() for k, v in p.items()}
    kv_scale = {"large_state_10x": 5.0, "large_state_100x": 50.0, "small_state": 0.015, "fresh": 0.0}.get(reg, 0.5)
    row_scale = 0.0 if reg == "fresh" else 1.0
    states = []
    for i in range(L):
        states += [bf16_round(rnd(B, D) * row_scale), rnd(B, H, N, N) * kv_scale, bf16_round(rnd(B, D) * row_scale)]
    ids = torch.randperm(V, generator=g)[:B]
    return p, states, ids


# ----------------------------------------------------------------------------------------------------------------------------
# the step
# ----------------------------------------------------------------------------------------------------------------------------
def _ln(x, w, b, eps=LN_EPS):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def _rot(v, D):
    """a per-channel vector read with the head offset one head off"""
    return torch.roll(v.reshape(D), N)


def ref_step(p, states, x_in, case: Case, rounded: bool, fault: Optional[str] = None):
    D, L, H, B = case.D, case.L, case.H, x_in.shape[0]
    Rw, Ra, Rv, Rg = case.ranks
    rd = bf16_round if rounded else (lambda t: t)
    P = lambda k: p[k].double()
    lin = lambda x, k: x @ P(k).t()
    lerp = (lambda h, prev, mu: prev + (h - prev) * mu) if fault == "lerp_reversed" else (lambda h, prev, mu: h + (prev - h) * mu)
    gn_eps = 1e-5 if fault == "gn_eps_1e-5" else GN_EPS
    out = dict(att_x_prev=[], att_kv=[], ffn_x_prev=[], inter=[], states=[])
    x = x_in.double()
    v_first = v_prev = None
    for l in range(L):
        pre = f"model.layers.{l}."
        at, ff = pre + "attn.", pre + "ffn."
        ax_prev, S, fx_prev = (t.double() for t in states[3 * l:3 * l + 3])
        if fault == "xprev_swapped":
            ax_prev, fx_prev = fx_prev, ax_prev
        # ---- P0: (pre_norm,) LayerNorm1, six lerps, att_x_prev <- h
        if l == 0:
            x = rd(_ln(x, P(pre + "pre_norm.weight"), P(pre + "pre_norm.bias")))
        h = rd(_ln(x, P(pre + "attn_norm.weight"), P(pre + "attn_norm.bias")))
        xr, xw, xk, xv, xa, xg = (rd(lerp(h, ax_prev, P(at + f"x_{n}").view(1, D))) for n in "rwkvag")
        ax_new = xr if fault == "xprev_after_lerp" else h
        # ---- P1: projections and low-rank down projections (fp32 partial sums in the kernel: unrounded)
        r, k, v = lin(xr, at + "r_proj.weight"), lin(xk, at + "k_proj.weight"), lin(xv, at + "v_proj.weight")
        hw = lin(xw, at + "w_lora.lora.0.weight")
        hw = rd(hw if fault == "decay_no_tanh" else torch.tanh(hw))
        ha = rd(lin(xa, at + "a_lora.lora.0.weight"))
        hg = lin(xg, at + "g_lora.lora.0.weight")
        hg = rd(hg if fault == "gate_no_sigmoid" else torch.sigmoid(hg))
        hv = rd(lin(xv, at + "v_lora.lora.0.weight")) if l > 0 else None
        if fault == "a_v_blocks_swapped" and l > 0:   # hidden layout [w | a | v | g] read with the a and v blocks exchanged
            cat = torch.cat([hv, ha], -1)
            ha, hv = cat[:, :Ra], cat[:, Ra:]
        # ---- P2 A-D: up projections, decay, a, value residual, kk, state update
        w_pre = lin(hw, at + "w_lora.lora.2.weight") + P(at + "w_lora.lora.2.bias")
        w = -torch.logaddexp(torch.zeros_like(w_pre), -w_pre) - (0.0 if fault == "decay_no_half" else 0.5)
        a = torch.sigmoid(lin(ha, at + "a_lora.lora.2.weight") + P(at + "a_lora.lora.2.bias"))
        v_raw = v
        if l == 0:
            v_first = v
        else:
            vf = v_prev if fault == "v_first_prev_layer" else v_first
            v = v + (vf - v) * torch.sigmoid(lin(hv, at + "v_lora.lora.2.weight") + P(at + "v_lora.lora.2.bias"))
        v_prev = v_raw
        g = lin(hg, at + "g_lora.lora.2.weight")
        k_k, k_a, r_k = P(at + "k_k"), P(at + "k_a"), P(at + "r_k").reshape(D)
        gn_w, gn_b = P(at + "g_norm.weight"), P(at + "g_norm.bias")
        if fault == "k_k_rot":
            k_k = _rot(k_k, D)
        if fault == "k_a_rot":
            k_a = _rot(k_a, D)
        if fault == "r_k_rot":
            r_k = _rot(r_k, D)
        if fault == "gn_w_rot":
            gn_w = _rot(gn_w, D)
        if fault == "gn_b_rot":
            gn_b = _rot(gn_b, D)
        kkr = (k * k_k).view(B, H, N)
        kk = kkr if fault == "kk_not_normalised" else kkr / kkr.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        k2 = (k * (1 + (a - 1) * k_a)).view(B, H, N)
        decay = torch.exp(-torch.exp(w)).view(B, H, N)
        av, rv, vv = a.view(B, H, N), r.view(B, H, N), v.view(B, H, N)
        sa = torch.einsum("bhij,bhj->bhi", S, -kk)          # S[b, h, value i, key j]
        S_new = S * decay.unsqueeze(-2) + sa.unsqueeze(-1) * (kk * av).unsqueeze(-2) + vv.unsqueeze(-1) * k2.unsqueeze(-2)
        # ---- P2 E: y, GroupNorm over the head, bonus, gate
        y = torch.einsum("bhij,bhj->bhi", S_new, rv)
        mu = y.mean(-1, keepdim=True)
        var = ((y - mu) ** 2).mean(-1, keepdim=True)
        yn = ((y - mu) / torch.sqrt(var + gn_eps)).reshape(B, D) * gn_w + gn_b
        bonus = ((rv * k2 * r_k.view(1, H, N)).sum(-1, keepdim=True) * vv).reshape(B, D)
        yg = rd((yn + bonus) * g)
        # ---- P3 + P4: output projection, residual, LayerNorm2, channel-mix lerp, ffn_x_prev <- h
        x = x + lin(yg, at + "o_proj.weight")
        h2 = rd(_ln(x, P(pre + "ffn_norm.weight"), P(pre + "ffn_norm.bias")))
        kx = rd(lerp(h2, fx_prev, P(ff + "x_k").view(1, D)))
        fx_new = kx if fault == "xprev_after_lerp" else h2
        # ---- P5 + P6: key, relu^2, value, residual
        kact = rd(torch.relu(lin(kx, ff + "key.weight")) ** 2)
        x = x + lin(kact, ff + "value.weight")
        out["att_x_prev"].append(ax_new)
        out["att_kv"].append(S_new)
        out["ffn_x_prev"].append(fx_new)
        out["states"] += [ax_new, S_new, fx_new]
        out["inter"].append(dict(w=w, a=a, kk=kk.reshape(B, D), k2=k2.reshape(B, D), v=v, y=y.reshape(B, D), w_pre=w_pre,
                                 var_y=var.reshape(B, H)))
    hfin = rd(_ln(x, P("model.norm.weight"), P("model.norm.bias")))
    logits = lin(hfin, "lm_head.weight")
    if "lm_head.bias" in p and fault != "head_bias_dropped":
        logits = logits + P("lm_head.bias")
    out["logits"] = logits
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# observables and their bars (from the two reference modes alone)
# ----------------------------------------------------------------------------------------------------------------------------
def observables(res, case: Case):
    """[(name, layer or None, tensor)] in pipeline order"""
    obs = []
    for l in range(case.L):
        obs += [("att_x_prev", l, res["att_x_prev"][l]), ("att_kv", l, res["att_kv"][l]), ("ffn_x_prev", l, res["ffn_x_prev"][l])]
    obs.append(("logits", None, res["logits"]))
    return obs


def _ulp(maxabs: float, sig_bits: int) -> float:
    """spacing of a binary format with `sig_bits` significand bits (bf16: 8, fp32: 24) at magnitude maxabs"""
    return 0.0 if maxabs == 0.0 else 2.0 ** (math.floor(math.log2(maxabs)) - (sig_bits - 1))


def bars(exact, rnd_, states, case: Case):
    """{(name, layer): dict(e_round, floor, bar)}:  bar = 2 e_round + floor.
    e_round = max |X_rounded - X_exact|: the kernel's fp32 summation order moves some bf16 roundings to the neighbouring value, so
    its error is a second draw of the same rounding noise, not the same draw -- two draws, each within the noise maximum.
    floor = K 2^-24 max|X_exact| + one ulp of X's storage type at max|X_exact| (the bars are max-norm bars, so the ulp is taken at
    the observable's largest magnitude): the fp32 accumulation the fp64 reference does not have, K = the longest reduction feeding
    X -- D for what is computed before the layer's channel mix (att_kv, ffn_x_prev, att_x_prev of layer 0), max(D, F) behind one
    (att_x_prev of later layers, logits).
    att_kv additionally: the kernel's softplus_d declares |dw| <= 6e-8 where e^u < 2^-24 (u = -w_pre < -16.6, the w -> -0.5 end).
    d/dw exp(-exp(w)) = -exp(w) exp(-exp(w)), so the decay factor moves by at most 6e-8 max(exp(w - exp(w))) and att_kv by that
    times max|S_old|.  It is added where a channel of the layer is in that range, and always for `no_decay` (where the factor
    exp(w) <= e^-12.5 makes it vanish)."""
    out = {}
    ex, rn = observables(exact, case), observables(rnd_, case)
    for (name, l, xe), (_, _, xr) in zip(ex, rn):
        mx = xe.abs().max().item()
        K = case.D if (name in ("att_kv", "ffn_x_prev") or (name == "att_x_prev" and l == 0)) else max(case.D, case.F)
        floor = K * U24 * mx + _ulp(mx, 24 if name in ("att_kv", "logits") else 8)
        if name == "att_kv":
            it = exact["inter"][l]
            if case.regime == "no_decay" or bool((it["w_pre"] > 16.0).any()):
                dfac = W_ABS_ERR * torch.exp(it["w"] - torch.exp(it["w"])).max().item()
                floor += dfac * states[3 * l + 1].abs().max().item()
        e_round = (xr - xe).abs().max().item()
        out[(name, l)] = dict(e_round=e_round, floor=floor, bar=2 * e_round + floor)
    return out


def rms_check_applies(b) -> bool:
    """The closer-to-rounded-than-to-exact check says nothing where the rounding noise is itself at the level of the fp32 floor."""
    return b["e_round"] > b["floor"]


def worst(x, ref):
    """(max |x - ref|, index tuple of the worst element)"""
    d = (x - ref).abs()
    i = int(d.reshape(-1).argmax())
    idx = []
    for n in reversed(d.shape):
        idx.append(i % n)
        i //= n
    return d.max().item(), tuple(reversed(idx))
