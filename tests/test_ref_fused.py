"""CPU: keeps the fp64 / slab reference of tests/test_fused_rows_gpu.py (tests/ref_fused.py) honest without a GPU:
slab evaluation equals whole-tensor evaluation, the fp64 functions agree with the fp32 ones at fp32 accuracy, and the surrogate loss
of the time-mix backward pair reproduces the gradient sums it claims (explicit autograd of the separate pieces)."""
import pytest
import torch

import ref_fused as RF

B, T, H = 5, 7, 2
D = H * 64


def _inputs(seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(dtype)
    raw = dict(r=mk(B, T, D), w_pre=mk(B, T, D, scale=2.0), k=mk(B, T, D), v=mk(B, T, D), a_pre=mk(B, T, D), g=mk(B, T, D),
               y=mk(B, T, D, scale=2.0), v_pre=mk(B, T, D), v_first=mk(B, T, D))
    par = dict(k_k=mk(D, scale=0.3) + 0.7, k_a=mk(D, scale=0.1) + 1.0, gn_weight=mk(D, scale=0.2) + 1.0, gn_bias=mk(D, scale=0.2),
               r_k=mk(H, 64, scale=0.1))
    mask = torch.ones(B, T)
    mask[1, :3] = 0
    mask[2, T - 1] = 0
    mask[4, :] = 0
    return raw, par, mask, mk


def _close(a, b, tol):
    assert a.shape == b.shape
    assert (a - b).abs().max().item() <= tol * max(b.abs().max().item(), 1e-3), (a - b).abs().max().item()


def _whole(fn, acts, params, douts):
    a = {k: (None if v is None else v.clone().requires_grad_(v.dtype.is_floating_point)) for k, v in acts.items()}
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    res = fn(a, p)
    torch.autograd.backward([o for o, d in zip(res, douts) if d is not None], [d for d in douts if d is not None])
    return res, {k: v.grad for k, v in a.items() if v is not None}, {k: v.grad for k, v in p.items()}


@pytest.mark.parametrize("slab_seqs", [1, 2, 5])
@pytest.mark.parametrize("stage", ["mix", "prepare", "post", "add_ln_mix"])
def test_slab_evaluation_equals_whole_tensor_evaluation(stage, slab_seqs):
    raw, par, mask, mk = _inputs(1)
    if stage == "mix":
        acts, params = dict(x=raw["k"], x_prev=mk(B, D)), dict(p0=mk(D), p1=mk(D), p2=mk(D))
        fn = lambda a, p: RF.token_shift_mix(a["x"] * a["mask"].unsqueeze(-1), a["x_prev"], [p["p0"], p["p1"], p["p2"]])
    elif stage == "prepare":
        acts = {k: raw[k] for k in ("w_pre", "k", "v", "a_pre", "v_pre", "v_first")}
        params = dict(k_k=par["k_k"], k_a=par["k_a"])
        fn = lambda a, p: RF.tmix_prepare(a["w_pre"], a["k"], a["v"], a["a_pre"], a["v_pre"], a["v_first"], p["k_k"], p["k_a"], a["mask"], H, False)
    elif stage == "post":
        acts = {k: raw[k] for k in ("y", "r", "k", "v", "g")}
        params = {k: par[k] for k in ("gn_weight", "gn_bias", "r_k")}
        fn = lambda a, p: (RF.tmix_post(a["y"], a["r"], a["k"], a["v"], a["g"], p["gn_weight"], p["gn_bias"], p["r_k"], H, 64e-5),)
    else:
        acts, params = dict(x=raw["k"], branch=raw["v"]), dict(gamma=par["gn_weight"], beta=par["gn_bias"], p0=mk(D), p1=mk(D))
        def fn(a, p):
            x1, outs, h = RF.add_layer_norm_mix(a["x"], a["branch"], p["gamma"], p["beta"], 1e-5, a["mask"], [p["p0"], p["p1"]], torch.bfloat16)
            return (x1, *outs, h)
    consts = dict(mask=mask.double())
    res0 = fn({**acts, **consts}, params)
    n = len(res0) - (1 if stage == "add_ln_mix" else 0)
    douts = [mk(*o.shape) for o in res0[:n]] + [None] * (len(res0) - n)
    probes = tuple(range(n, len(res0)))
    outs, ag, pg, prg = RF.eval_in_slabs(fn, acts, params, douts, slab_seqs=slab_seqs, probes=probes, consts=consts)
    wa = {k: v.clone().requires_grad_(True) for k, v in acts.items()}
    wp = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    res = fn({**wa, **consts}, wp)
    for i in probes:
        res[i].retain_grad()
    torch.autograd.backward(list(res[:n]), douts[:n])
    for o, w in zip(outs, res):
        _close(o, w.detach(), 1e-13)
    for k in acts:
        _close(ag[k], wa[k].grad, 1e-12)
    for k in params:
        _close(pg[k], wp[k].grad, 1e-12)
    for i in probes:
        _close(prg[i], res[i].grad, 1e-12)
        assert torch.equal(prg[i], prg[i].bfloat16().double())       # dh is rounded to the tensor type on the way back


def test_fp64_functions_agree_with_fp32_at_fp32_accuracy():
    raw, par, mask, mk = _inputs(2, torch.float32)
    f64 = lambda d: {k: v.double() for k, v in d.items()}
    r64, p64 = f64(raw), f64(par)
    m3 = mask.unsqueeze(-1)
    pairs = [
        (RF.tmix_prepare(raw["w_pre"], raw["k"], raw["v"], raw["a_pre"], raw["v_pre"], raw["v_first"], par["k_k"], par["k_a"], m3, H, False),
         RF.tmix_prepare(r64["w_pre"], r64["k"], r64["v"], r64["a_pre"], r64["v_pre"], r64["v_first"], p64["k_k"], p64["k_a"], mask, H, False)),
        (RF.tmix_prepare(raw["w_pre"], raw["k"], raw["v"], raw["a_pre"], None, None, par["k_k"], par["k_a"], None, H, True),
         RF.tmix_prepare(r64["w_pre"], r64["k"], r64["v"], r64["a_pre"], None, None, p64["k_k"], p64["k_a"], None, H, True)),
        ((RF.tmix_post(raw["y"], raw["r"], raw["k"], raw["v"], raw["g"], par["gn_weight"], par["gn_bias"], par["r_k"], H, 64e-5),),
         (RF.tmix_post(r64["y"], r64["r"], r64["k"], r64["v"], r64["g"], p64["gn_weight"], p64["gn_bias"], p64["r_k"], H, 64e-5),)),
        (RF.token_shift_mix6(raw["k"], raw["v"][:, 0], *[par["k_k"].view(1, 1, D)] * 6), RF.token_shift_mix6(r64["k"], r64["v"][:, 0], *[p64["k_k"]] * 6)),
        ((RF.token_shift_mix1(raw["k"], None, par["k_a"]), RF.relu_sq(raw["k"])), (RF.token_shift_mix1(r64["k"], None, p64["k_a"]), RF.relu_sq(r64["k"]))),
        (RF.add_layer_norm(raw["k"], raw["v"], par["gn_weight"], par["gn_bias"], 1e-5), RF.add_layer_norm(r64["k"], r64["v"], p64["gn_weight"], p64["gn_bias"], 1e-5)),
        ((torch.nn.functional.layer_norm(raw["k"], (D,), par["gn_weight"], None, 1e-5),), (RF.layer_norm(r64["k"], p64["gn_weight"], None, 1e-5),)),
    ]
    for a32, a64 in pairs:
        for u, v in zip(a32, a64):
            assert u.dtype == torch.float32 and v.dtype == torch.float64
            _close(u.double(), v, 2e-6)


def test_add_layer_norm_mix_is_the_composition_with_the_stored_roundings():
    raw, par, mask, mk = _inputs(3)
    bf = lambda t: t.bfloat16().double()
    x, br = bf(raw["k"]), bf(raw["v"])
    ps = [mk(D), mk(D)]
    x1, outs, h = RF.add_layer_norm_mix(x, br, par["gn_weight"], par["gn_bias"], 1e-5, mask, ps, torch.bfloat16)
    assert torch.equal(x1, bf(x + br))
    assert torch.equal(h, bf(RF.layer_norm(x1, par["gn_weight"], par["gn_bias"], 1e-5)))
    want = RF.token_shift_mix(h * mask.unsqueeze(-1), None, ps)
    for o, w in zip(outs, want):
        assert torch.equal(o, w)
    # without a tensor type nothing is rounded
    x1n, outsn, hn = RF.add_layer_norm_mix(x, br, par["gn_weight"], par["gn_bias"], 1e-5, None, ps, None)
    assert torch.equal(hn, RF.layer_norm(x + br, par["gn_weight"], par["gn_bias"], 1e-5))


@pytest.mark.parametrize("layer0,nsets,masked", [(False, 1, True), (True, 2, False), (False, 2, False)])
def test_surrogate_loss_gives_the_gradient_sums_of_the_separate_pieces(layer0, nsets, masked):
    """d surrogate / d input = (post backward's gradient) + (prepare backward applied to the scan's gradients + post's d_k2, d_v2)
    + the direct terms <r, dq>, <v_first, d_vf_next>: assembled here piece by piece with explicit autograd calls."""
    raw, par, mask, mk = _inputs(4)
    if layer0:
        raw = {k: v for k, v in raw.items() if k not in ("v_pre", "v_first")}
    m = mask if masked else None
    cot = dict(dout=mk(B, T, D), dv=[mk(B, T, D)], **{n: [mk(B, T, D) for _ in range(nsets)] for n in ("dw", "dq", "dk", "da", "db")})
    if not layer0:
        cot["d_vf_next"] = mk(B, T, D)
    a = {k: v.clone().requires_grad_(True) for k, v in raw.items()}
    p = {k: v.clone().requires_grad_(True) for k, v in par.items()}
    RF.tmix_pair_loss(a, p, cot, m, H, 64e-5, layer0).backward()
    # the pieces
    b = {k: v.clone().requires_grad_(True) for k, v in raw.items()}
    q = {k: v.clone().requires_grad_(True) for k, v in par.items()}
    prep = RF.tmix_prepare(b["w_pre"], b["k"], b["v"], b["a_pre"], b.get("v_pre"), b.get("v_first"), q["k_k"], q["k_a"], m, H, layer0)
    k2l, v2l = prep[1].detach().requires_grad_(True), prep[2].detach().requires_grad_(True)
    out = RF.tmix_post(b["y"], b["r"], k2l, v2l, b["g"], q["gn_weight"], q["gn_bias"], q["r_k"], H, 64e-5)
    out.backward(cot["dout"])                                     # post backward: d_y, d_r, d_k2, d_v2, d_g, d gn_w, d gn_b, d r_k
    tot = lambda n: sum(cot[n])
    torch.autograd.backward(list(prep), [tot("dw"), tot("dk") + k2l.grad, tot("dv") + v2l.grad, tot("da"), tot("db")])   # prepare backward
    want = {k: v.grad for k, v in b.items()}
    want["r"] = want["r"] + tot("dq")
    if not layer0:
        want["v_first"] = want["v_first"] + cot["d_vf_next"]
    for k in raw:
        _close(a[k].grad, want[k], 1e-12)
    for k in par:
        _close(p[k].grad, q[k].grad, 1e-12)


def test_surrogate_loss_stored_roundings():
    """compact: the gradient reaching v2 through the bonus is round(dt) * dot, nothing else is rounded; non-compact: post's d_r, d_k2,
    d_v2 are rounded before they are added; `stored` replaces the forward values of k2 / v2 and leaves the gradient path alone."""
    raw, par, mask, mk = _inputs(5)
    bf = lambda t: t.bfloat16().double()
    cot = dict(dout=bf(mk(B, T, D)), dv=[mk(B, T, D)], **{n: [mk(B, T, D)] for n in ("dw", "dq", "dk", "da", "db")})
    raw["g"] = bf(raw["g"])

    def grads(**kw):
        a = {k: v.clone().requires_grad_(True) for k, v in raw.items()}
        RF.tmix_pair_loss(a, par, cot, None, H, 64e-5, False, **kw).backward()
        return {k: v.grad for k, v in a.items()}

    with torch.no_grad():
        _, k2, v2, _, _ = RF.tmix_prepare(raw["w_pre"], raw["k"], raw["v"], raw["a_pre"], raw["v_pre"], raw["v_first"], par["k_k"], par["k_a"], None, H, False)
    plain = grads()
    st = grads(rt=torch.bfloat16, stored=(bf(k2), bf(v2)))
    auto = grads(rt=torch.bfloat16)
    for k in raw:
        _close(st[k], auto[k], 1e-13)                   # rounding k2 / v2 here or taking the stored (rounded) values is the same thing
        _close(st[k], plain[k], 2.0 ** -6)              # and a rounding-level change of the gradients
    assert not torch.equal(st["v"], plain["v"])
    # compact, exact k2 / v2 (stored = the unrounded values): only the v2 path through the bonus sees the rounded dt
    ex = grads(rt=torch.bfloat16, stored=(k2, v2))
    for k in ("y", "g", "r", "k", "a_pre", "w_pre"):
        _close(ex[k], plain[k], 1e-13)
    dt = cot["dout"] * raw["g"]
    assert torch.equal(dt, dt.float().double())         # a product of two bf16 values is exact in fp32: the kernel rounds the same number
    for k in ("v", "v_pre", "v_first"):
        assert not torch.equal(ex[k], plain[k])
        _close(ex[k], plain[k], 2.0 ** -7)
    full = grads(rt=torch.bfloat16, stored=(k2, v2), round_post_grads=True)
    for k in ("y", "g", "w_pre"):
        _close(full[k], plain[k], 1e-13)
    for k in ("r", "k", "v", "a_pre", "v_pre", "v_first"):
        assert not torch.equal(full[k], plain[k])
        _close(full[k], plain[k], 2.0 ** -7)
