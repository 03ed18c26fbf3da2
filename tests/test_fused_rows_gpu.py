"""GPU (-m gpu): the row-stream stages of rwkvtts_amd/csrc/elementwise.hip when a workgroup walks MANY rows, against the fp64
restatement of the reference formulas (tests/ref_fused.py, evaluated on the CPU in slabs of whole sequences), forward and backward.

tests/test_fused_gpu.py checks the same stages at 48-135 rows, where every workgroup handles one row or one run: the second
iteration of the row loops, the carry between the runs of one workgroup, the LDS phase toggle, the prefetch of a row gridDim.x
further on and a parameter-gradient partial that sums several runs are only executed here.  Two families:
  a. the shipped workgroup counts at the shapes training runs (32 768 rows: 32 rows per backward workgroup, 8 runs per mix-backward
     workgroup, partials through the device column sum, relu^2 beyond its 8192-workgroup cap);
  b. a few workgroups (1, 3, 7, 300) and other run lengths on awkward shapes (fused.py's module constants patched).
Section 3 calls the C entry points of the time-mix backward pair directly, as fused._TmixCore.backward does.

Inputs are exactly representable in the tensor type (_mk).  Bars (derived in the header of tests/test_fused_gpu.py):
  fp32 kernels: 2e-5 (forward) / 1e-4 (backward, parameter gradients) of max|ref|;
  bf16 kernels: parameter gradients 2^-6 of max|ref|; every other output within 1 bf16 ulp of the reference (_cmp_bf16, 2^-7
  relative with its floor) where the kernel rounds once.

Stored roundings (an intermediate written in the tensor type and read back; the reference rounds at the same point, straight
through -- ref_fused.ste_round / round_grad):
  x1 = x + branch            add + LayerNorm, all variants (elementwise.hip: "rounded to T, as the separate add would").  The sum of
                             two bf16 values is exact in fp32 and fp64 alike, so the reference reproduces the rounding bit for bit
                             and it costs no ulp: h and dx of add_layer_norm stay at 1 ulp.
  h before the mix           one-pass add + LayerNorm + mix ("h is rounded to the tensor type before it is mixed").  h comes out of
                             fp32 arithmetic in the kernel and fp64 in the reference, so now and then (about 5e-5 of the elements)
                             the rounding falls the other way and h differs by ONE ulp of h.  k = 2 for the mixed outputs: one ulp
                             of the output plus one ulp of the stored h.  An ulp of h is not an ulp of the output where the lerp
                             cancels (out = hm[t] (1 - p) + hm[t-1] p), so the second ulp is taken where it arises and carried
                             through the lerp exactly: 2^-7 (|hm[t]| |1 - p| + |hm[t-1]| |p|)  (_cmp_bf16_stored).  (Measured at
                             32 768 x 2048: up to 5.7 ulp of the output at such elements, so a flat 2 ulp of the output cannot
                             hold for a correct kernel; with the carried form every element of every case is inside.)
  dh between mix backward    the same in the backward, one-pass ("dh = g * mask, rounded to the tensor type") or as two kernels:
  and LayerNorm backward     k = 2 for dx (= d branch): one ulp of dx plus one ulp of the stored dh carried through the LayerNorm
                             backward, 2^-7 rstd (|gamma dh| + mean|gamma dh| + |xhat| mean|gamma dh xhat|).
  k2, v2                     tmix_prepare_fwd -> tmix_post (section 3).  The reference takes the values the forward kernel stored
                             (checked against the reference in section 2), so they cost the backward pair no ulp.
  dt (compact post backward) dt = dout * g is a product of two bf16 values, exact in fp32: the reference reproduces its rounding bit
                             for bit, no ulp.  But the prepare backward rebuilds k2 in fp32 for d_r += ds k2 r_k ("recomputed from k,
                             a, k_a as the forward did") where the exact gradient has the stored k2: half an ulp of k2 carried into
                             d_r, 2^-8 |ds k2 r_k|, on top of the ulp of d_r.
  d_r, d_k2, d_v2            non-compact post backward -> prepare backward (several gradient sets summed on load): k = 2 for every
  (post backward)            gradient that takes one of them in (d_r, d_k, d_a_pre, d_v, d_v_pre, d_v_first): one ulp of the output
                             plus one ulp of the stored gradient carried through the prepare backward, 2^-7 |d out / d s| |s|.
                             (Measured with a flat 2 ulp of the output instead: 1-2 of 1.3 M elements per tensor beyond it, up to
                             3.5 ulp, all where the scan's gradient and the post backward's cancel -- an ulp of the stored
                             addend is then several ulp of the small sum.  The flat form would need k = 4 there and hide a
                             wrong term of that size everywhere else; the carried form does not.)
"""
import ctypes
import types

import pytest
import torch

import ref_fused as RF
from fused_parity import DEV, _cmp, _cmp_bf16, _mk
from rwkvtts_amd import fused

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
EPS_LN, EPS_GN = 1e-5, 64e-5


def _cmp_bf16_stored(got, want, what, prop):
    """_cmp_bf16's one ulp of the output plus `prop`: one ulp of a stored intermediate carried to this output (module docstring)."""
    got = got.detach().float().cpu()
    want = want.detach().float()
    floor = want.abs().mean().item() * 0.25 + 1e-6
    tol = 2.0 ** -7 * torch.clamp(want.abs(), min=floor) + prop.float()
    bad = (got - want).abs() > tol
    assert not bad.any(), f"{what}: {bad.sum().item()}/{bad.numel()} beyond 1 bf16 ulp + one ulp of the stored intermediate"


def _figure(got, want, what):
    """Printed before every assertion (pytest -s / a log): max error in units of _cmp_bf16's one-ulp tolerance and of max|ref|."""
    got = got.detach().float().cpu()
    want = want.detach().float()
    d = (got - want).abs()
    floor = want.abs().mean().item() * 0.25 + 1e-6
    ulp = (d / (2.0 ** -7 * torch.clamp(want.abs(), min=floor))).max().item()
    print(f"    {what}: max|d| {d.max().item():.3e} = {d.max().item() / max(want.abs().max().item(), 1e-30):.2e} of max|ref|, {ulp:.2f} ulp")


def _compare(got, want, what, dtype, f32_tol, ulps=1.0, prop=None):
    assert got is not None, what
    assert tuple(got.shape) == tuple(want.shape), (what, got.shape, want.shape)
    _figure(got, want, what)
    if dtype == F32:
        _cmp(got, want, f32_tol, what)
    elif prop is not None:
        _cmp_bf16_stored(got, want, what, prop)
    else:
        _cmp_bf16(got, want, what, ulps=ulps)


def _cmp_param(got, want, what, dtype):
    assert got is not None, what
    _figure(got.reshape(want.shape), want, what)
    _cmp(got.reshape(want.shape), want, 2.0 ** -6 if dtype == BF16 else 1e-4, what)


def _to_dev(d, dtype, grad):
    out = {}
    for k, v in d.items():
        out[k] = None if v is None else (v.to(DEV, dtype).requires_grad_(True) if grad else v.to(DEV, dtype))
    return out


def _norm(p):
    return types.SimpleNamespace(weight=p["gamma"], bias=p["beta"], eps=EPS_LN)


def _mask3(c):
    return None if c.get("mask") is None else c["mask"].unsqueeze(-1)


# ------------------------------------------------------------------------------------------------------
# masks
# ------------------------------------------------------------------------------------------------------
def _mask_left_padding(B, T):
    """Training batches: left padding on some of the sequences."""
    m = torch.ones(B, T)
    m[1, :37] = 0
    m[B - 1, :T // 3] = 0
    return m


def _mask_awkward(B, T, run):
    """Zeros at the first and the last row of a run, at t = 0, at t = T - 1, in the middle of a sequence (packed rows restart the
    shift there), and one fully masked sequence."""
    m = torch.ones(B * T)
    rows = B * T
    for r in (run * (rows // (2 * run)), run * (rows // (3 * run)) + run - 1):   # first / last row of a run
        m[min(r, rows - 1)] = 0
    m = m.view(B, T)
    full = 2 if B > 3 else 0          # not the last sequence: the end of the tensor is a run edge that has to stay visible
    m[B - 1 if full == 0 else 0, 0] = 0
    m[1, T - 1] = 0
    m[1, T // 2] = 0
    m[full, :] = 0
    return m


# ------------------------------------------------------------------------------------------------------
# the stages: acts (sliced into slabs, gradients), params (gradients summed), consts, hip(a, p, c), ref(a, p, rt)
# ------------------------------------------------------------------------------------------------------
def _stage_mix(nmix, B, T, D, dtype, mask, g, with_prev):
    acts = dict(x=_mk((B, T, D), g, 1.0, dtype))
    if with_prev:
        acts["x_prev"] = _mk((B, D), g, 1.0, dtype)   # carried row: the t = 0 branch, also in runs other than a workgroup's first
    params = {f"p{i}": _mk((D,), g, 0.5, dtype) for i in range(nmix)}

    def hip(a, p, c):
        ps = [p[f"p{i}"] for i in range(nmix)]
        if nmix == 6:
            return fused.token_shift_mix6(a["x"], a.get("x_prev"), *ps, _mask3(c))
        if nmix == 1:
            return (fused.token_shift_mix1(a["x"], a.get("x_prev"), ps[0], _mask3(c)),)
        stacked = torch.cat([q.reshape(1, D) for q in ps], 0)          # the x_r, x_k, x_v lerps of fused.mix_lora: mix_fwd / mix_bwd <3>
        return fused._Mix.apply(a["x"], a.get("x_prev"), fused._mask_rows(_mask3(c), a["x"]), stacked)

    def ref(a, p, rt):
        xm = a["x"] if a.get("mask") is None else a["x"] * a["mask"].unsqueeze(-1)
        return RF.token_shift_mix(xm, a.get("x_prev"), [p[f"p{i}"] for i in range(nmix)])

    return types.SimpleNamespace(acts=acts, params=params, consts=dict(mask=mask), hip=hip, ref=ref)


def _stage_prepare(layer0, B, T, D, dtype, mask, g):
    H = D // 64
    acts = dict(w_pre=_mk((B, T, D), g, 2.0, dtype), k=_mk((B, T, D), g, 1.0, dtype), v=_mk((B, T, D), g, 1.0, dtype),
                a_pre=_mk((B, T, D), g, 1.0, dtype))
    if not layer0:   # v_pre / v_first present (layers > 0) or absent (layer 0)
        acts.update(v_pre=_mk((B, T, D), g, 1.0, dtype), v_first=_mk((B, T, D), g, 1.0, dtype))
    params = dict(k_k=(_mk((D,), g, 0.3, dtype) + 0.7).to(dtype).float(), k_a=(_mk((D,), g, 0.1, dtype) + 1.0).to(dtype).float())

    def hip(a, p, c):
        return fused.tmix_prepare(a["w_pre"], a["k"], a["v"], a["a_pre"], a.get("v_pre"), a.get("v_first"), p["k_k"], p["k_a"],
                                  _mask3(c), H, layer0)

    def ref(a, p, rt):
        return RF.tmix_prepare(a["w_pre"], a["k"], a["v"], a["a_pre"], a.get("v_pre"), a.get("v_first"), p["k_k"], p["k_a"],
                               a.get("mask"), H, layer0)

    return types.SimpleNamespace(acts=acts, params=params, consts=dict(mask=mask), hip=hip, ref=ref)


def _post_params(D, dtype, g):
    return dict(gn_weight=(_mk((D,), g, 0.2, dtype) + 1.0).to(dtype).float(), gn_bias=_mk((D,), g, 0.2, dtype),
                r_k=_mk((D // 64, 64), g, 0.1, dtype))


def _stage_post(B, T, D, dtype, g):
    H = D // 64
    acts = dict(y=_mk((B, T, D), g, 2.0, dtype), r=_mk((B, T, D), g, 1.0, dtype), k=_mk((B, T, D), g, 1.0, dtype),
                v=_mk((B, T, D), g, 1.0, dtype), g=_mk((B, T, D), g, 1.0, dtype))

    def hip(a, p, c):
        return (fused.tmix_post(a["y"], a["r"], a["k"], a["v"], a["g"], p["gn_weight"], p["gn_bias"], p["r_k"], H, EPS_GN),)

    def ref(a, p, rt):
        return (RF.tmix_post(a["y"], a["r"], a["k"], a["v"], a["g"], p["gn_weight"], p["gn_bias"], p["r_k"], H, EPS_GN),)

    return types.SimpleNamespace(acts=acts, params=_post_params(D, dtype, g), consts={}, hip=hip, ref=ref)


def _stage_relu_sq(B, T, D, dtype, g, wide):
    acts = dict(x=_mk((B, T, 4 * D if wide else D), g, 1.0, dtype))   # wide: the channel-mix hidden width
    return types.SimpleNamespace(acts=acts, params={}, consts={}, hip=lambda a, p, c: (fused.relu_sq(a["x"]),),
                                 ref=lambda a, p, rt: (RF.relu_sq(a["x"]),))


def _ln_params(D, dtype, g):
    return dict(gamma=(_mk((D,), g, 0.2, dtype) + 1.0).to(dtype).float(), beta=_mk((D,), g, 0.1, dtype))


def _stage_layer_norm(with_branch, B, T, D, dtype, g):
    acts = dict(x=(_mk((B, T, D), g, 1.5, dtype) + 0.3).to(dtype).float())
    if with_branch:
        acts["branch"] = _mk((B, T, D), g, 1.0, dtype)

    def hip(a, p, c):
        if with_branch:
            return fused.add_layer_norm(a["x"], a["branch"], _norm(p))
        return (fused.layer_norm(a["x"], _norm(p)),)

    def ref(a, p, rt):
        x1, h = RF.add_layer_norm(a["x"], a.get("branch"), p["gamma"], p["beta"], EPS_LN, rt)
        return (x1, h) if with_branch else (h,)

    return types.SimpleNamespace(acts=acts, params=_ln_params(D, dtype, g), consts={}, hip=hip, ref=ref)


def _stage_add_ln_mix(nmix, fwd_only, with_branch, B, T, D, dtype, mask, g):
    """One-pass add + LayerNorm + mix.  fwd_only with nmix > 1: rwkv7_add_ln_mix_fwd_h forward (also what add_layer_norm_mix_lora
    launches with nmix = 3), mix_bwd + add_ln_bwd backward; else rwkv7_add_ln_mix_fwd / rwkv7_mix_add_ln_bwd."""
    acts = dict(x=(_mk((B, T, D), g, 1.3, dtype) + 0.2).to(dtype).float())
    if with_branch:
        acts["branch"] = _mk((B, T, D), g, 1.0, dtype)
    params = _ln_params(D, dtype, g)
    params.update({f"p{i}": torch.rand(D, generator=g).to(dtype).float() for i in range(nmix)})

    def hip(a, p, c):
        x1, outs = fused.add_layer_norm_mix(a["x"], a.get("branch"), _norm(p), _mask3(c), tuple(p[f"p{i}"] for i in range(nmix)),
                                            fwd_only=fwd_only)
        return (x1, *outs)

    def ref(a, p, rt):
        x1, outs, h = RF.add_layer_norm_mix(a["x"], a.get("branch"), p["gamma"], p["beta"], EPS_LN, a.get("mask"),
                                            [p[f"p{i}"] for i in range(nmix)], rt)
        return (x1, *outs, h)

    def props(outs_r, probe_grads, st):
        """One ulp of the stored h carried into out_i, one ulp of the stored dh carried into dx (module docstring)."""
        x1, h, dh = outs_r[0].float(), outs_r[-1].float(), probe_grads[nmix + 1].float()
        hm = h.abs() if mask is None else h.abs() * mask.unsqueeze(-1)
        hs = torch.nn.functional.pad(hm, (0, 0, 1, -1))
        po = {1 + i: 2.0 ** -7 * (hm * (1 - st.params[f"p{i}"]).abs() + hs * st.params[f"p{i}"].abs()) for i in range(nmix)}
        var, mu = torch.var_mean(x1, -1, unbiased=False, keepdim=True)
        rs = torch.rsqrt(var + EPS_LN)
        xh = ((x1 - mu) * rs).abs()
        gd = (dh * st.params["gamma"]).abs()
        pdx = 2.0 ** -7 * rs * (gd + gd.mean(-1, keepdim=True) + xh * (gd * xh).mean(-1, keepdim=True))
        return po, dict(x=pdx, branch=pdx)

    return types.SimpleNamespace(acts=acts, params=params, consts=dict(mask=mask), hip=hip, ref=ref, nprobe=1, props=props)


STAGES = ["token_shift_mix6", "token_shift_mix1", "mix_lora_nmix3", "tmix_prepare_layer0", "tmix_prepare_later", "tmix_post", "relu_sq",
          "layer_norm", "add_layer_norm", "add_layer_norm_mix6", "add_layer_norm_mix1", "add_layer_norm_mix6_fwd_only",
          "add_layer_norm_mix1_fwd_only", "add_layer_norm_mix_lora_nmix3_fwd"]


def _build(stage, B, T, D, dtype, mask, g, awkward):
    if stage == "token_shift_mix6":
        return _stage_mix(6, B, T, D, dtype, mask, g, with_prev=awkward)
    if stage == "token_shift_mix1":
        return _stage_mix(1, B, T, D, dtype, mask, g, with_prev=awkward)
    if stage == "mix_lora_nmix3":
        return _stage_mix(3, B, T, D, dtype, mask, g, with_prev=False)
    if stage == "tmix_prepare_layer0":
        return _stage_prepare(True, B, T, D, dtype, mask, g)
    if stage == "tmix_prepare_later":
        return _stage_prepare(False, B, T, D, dtype, mask, g)
    if stage == "tmix_post":
        return _stage_post(B, T, D, dtype, g)
    if stage == "relu_sq":
        return _stage_relu_sq(B, T, D, dtype, g, wide=not awkward)
    if stage == "layer_norm":
        return _stage_layer_norm(False, B, T, D, dtype, g)
    if stage == "add_layer_norm":
        return _stage_layer_norm(True, B, T, D, dtype, g)
    if stage == "add_layer_norm_mix6":
        return _stage_add_ln_mix(6, False, True, B, T, D, dtype, mask, g)
    if stage == "add_layer_norm_mix1":
        return _stage_add_ln_mix(1, False, True, B, T, D, dtype, mask, g)
    if stage == "add_layer_norm_mix6_fwd_only":
        return _stage_add_ln_mix(6, True, True, B, T, D, dtype, mask, g)
    if stage == "add_layer_norm_mix1_fwd_only":   # (one coefficient vector: fused.add_layer_norm_mix takes the one-pass backward either way)
        return _stage_add_ln_mix(1, True, False, B, T, D, dtype, mask, g)
    if stage == "add_layer_norm_mix_lora_nmix3_fwd":
        return _stage_add_ln_mix(3, True, True, B, T, D, dtype, mask, g)
    raise KeyError(stage)


def _check_stage(st, name, dtype, slab_seqs):
    a_h, p_h, c_h = _to_dev(st.acts, dtype, True), _to_dev(st.params, dtype, True), _to_dev(st.consts, dtype, False)
    outs_h = st.hip(a_h, p_h, c_h)
    outs_h = tuple(outs_h) if isinstance(outs_h, (tuple, list)) else (outs_h,)
    n = len(outs_h)
    g = torch.Generator().manual_seed(77)
    douts = [_mk(o.shape, g, 1.0, dtype) for o in outs_h]
    torch.autograd.backward(list(outs_h), [d.to(DEV, dtype) for d in douts])
    torch.cuda.synchronize()
    nprobe = getattr(st, "nprobe", 0)
    outs_r, ag, pg, prg = RF.eval_in_slabs(lambda a, p: st.ref(a, p, dtype), st.acts, st.params, douts + [None] * nprobe,
                                           slab_seqs=slab_seqs, probes=tuple(range(n, n + nprobe)), consts=st.consts)
    po, pgr = st.props(outs_r, prg, st) if (dtype == BF16 and hasattr(st, "props")) else ({}, {})
    print(f"\n  {name} {dtype} rows {outs_h[0].shape[0] * outs_h[0].shape[1]}")
    for i in range(n):
        _compare(outs_h[i], outs_r[i], f"{name} out[{i}]", dtype, 2e-5, prop=po.get(i))
    for k in ag:
        _compare(a_h[k].grad, ag[k], f"{name} d{k}", dtype, 1e-4, prop=pgr.get(k))
    for k in pg:
        _cmp_param(p_h[k].grad, pg[k], f"{name} d{k}", dtype)


# ------------------------------------------------------------------------------------------------------
# 2a. shipped workgroup counts at the shapes training runs
# ------------------------------------------------------------------------------------------------------
TRAIN_SHAPES = [(8, 4096, 1024, BF16), (4, 8192, 2048, BF16), (2, 4096, 1024, F32)]


@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("B,T,D,dtype", TRAIN_SHAPES, ids=["bf16-8x4096x1024", "bf16-4x8192x2048", "fp32-2x4096x1024"])
def test_training_shape_with_shipped_workgroup_counts(stage, B, T, D, dtype):
    """Every backward workgroup walks 32 rows (8 in fp32) or 8 runs, the >= 256 partials go through rwkv7_sum_slabs_bf16, relu^2 at
    [B*T, 4 D] grid-strides; left-padding masks where the stage takes one."""
    rows = B * T
    assert rows > fused._BWD_BLOCKS >= 256 and -(-rows // fused._MIX_BWD_ROWS) > fused._MIX_BWD_BLOCKS
    assert dtype == F32 or -(-rows // fused._ADD_LN_MIX_RUN) > fused._ADD_LN_MIX_BWD_BLOCKS   # (fp32: 2048 runs on 2048 workgroups)
    g = torch.Generator().manual_seed(1000 + D + STAGES.index(stage))
    st = _build(stage, B, T, D, dtype, _mask_left_padding(B, T), g, awkward=False)
    _check_stage(st, stage, dtype, slab_seqs=max(1, 8192 * 1024 // (T * D * (4 if stage == "relu_sq" else 1))))


# ------------------------------------------------------------------------------------------------------
# 2b. a few workgroups walk everything, awkward shapes
# ------------------------------------------------------------------------------------------------------
def _patch_blocks(monkeypatch, blocks, run):
    for name in ("_FWD_BLOCKS", "_MIX_FWD_BLOCKS", "_BWD_BLOCKS", "_MIX_BWD_BLOCKS", "_ADD_LN_MIX_BLOCKS", "_ADD_LN_MIX_BWD_BLOCKS"):
        monkeypatch.setattr(fused, name, blocks)
    monkeypatch.setattr(fused, "_MIX_BWD_ROWS", run)
    monkeypatch.setattr(fused, "_ADD_LN_MIX_RUN", run)


# (B, T, D, workgroups, run length, dtype).  Between them: T not a multiple of the run length (runs straddle two sequences), rows and
# runs not a multiple of the workgroup count (some workgroups get one iteration fewer), rows < workgroups (5 x 1 and 4 x 5 with 300),
# D = 2560 (320 threads: five waves in the LDS reductions), D = 4096 (the maximum), 300 workgroups with more rows / runs than
# workgroups (17 x 77: the device column sum with a slab count that is not a power of two, second iterations for some workgroups only).
AWKWARD = [(3, 45, 1024, 3, 4, BF16), (3, 77, 2560, 7, 3, BF16), (4, 5, 4096, 1, 4, BF16), (5, 1, 128, 300, 4, BF16),
           (4, 5, 2048, 300, 8, BF16), (17, 77, 1024, 300, 4, BF16), (3, 45, 2560, 7, 4, F32), (3, 77, 1024, 3, 5, F32),
           (4, 5, 128, 1, 4, F32), (17, 77, 2048, 300, 4, F32)]
AWKWARD_IDS = [f"{'bf16' if c[5] == BF16 else 'fp32'}-{c[0]}x{c[1]}x{c[2]}-wg{c[3]}-run{c[4]}" for c in AWKWARD]


@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("B,T,D,blocks,run,dtype", AWKWARD, ids=AWKWARD_IDS)
def test_few_workgroups_walk_awkward_shapes(stage, B, T, D, blocks, run, dtype, monkeypatch):
    _patch_blocks(monkeypatch, blocks, run)
    g = torch.Generator().manual_seed(2000 + D + T + STAGES.index(stage))
    st = _build(stage, B, T, D, dtype, _mask_awkward(B, T, run), g, awkward=True)
    _check_stage(st, stage, dtype, slab_seqs=2)   # (slabs of two sequences, the last one shorter when B is odd)


# ------------------------------------------------------------------------------------------------------
# 3. the time-mix backward pair through its C entry points
# ------------------------------------------------------------------------------------------------------
def _pair_hip(dtype, raw, par, cot, mask, H, layer0, compact, nb):
    """fused._TmixCore.backward, stages 1 and 3, with `cot` standing in for the scan's gradients.  Returns (stored k2 / v2, results)."""
    d = lambda t: None if t is None else t.to(DEV, dtype).contiguous()
    R = {k: d(v) for k, v in raw.items()}
    P = {k: d(v.reshape(-1)) for k, v in par.items()}
    C = {k: ([d(t) for t in v] if isinstance(v, list) else d(v)) for k, v in cot.items()}
    m = None if mask is None else d(mask.reshape(-1))
    k = R["k"]
    B, T, D = k.shape
    rows = B * T
    p, call, cl = fused._p, fused._call, ctypes.c_long
    w, k2, v2, a_in, b_in = [torch.empty_like(k) for _ in range(5)]
    call("tmix_prepare_fwd", k, cl(rows), D, p(R["w_pre"]), p(k), p(R["v"]), p(R["a_pre"]), p(R.get("v_pre")), p(R.get("v_first")), p(m),
         p(P["k_k"]), p(P["k_a"]), p(w), p(k2), p(v2), p(a_in), p(b_in), min(rows, fused._FWD_BLOCKS))
    part_post = torch.empty(nb, 3, D, dtype=torch.float32, device=DEV)
    post_args = (cl(rows), D, p(C["dout"]), p(R["y"]), p(R["r"]), p(k2), p(v2), p(R["g"]), p(P["gn_weight"]), p(P["gn_bias"]), p(P["r_k"]),
                 ctypes.c_float(EPS_GN))
    if compact:
        d_y, dt_post, d_g = [torch.empty_like(k) for _ in range(3)]
        hscal = torch.empty(rows, H, 2, dtype=torch.float32, device=DEV)
        d_r_post = d_k2_post = d_v2_post = None
        call("tmix_post_bwd_compact", k, *post_args, p(d_y), p(dt_post), p(d_g), p(hscal), p(part_post), nb)
    else:
        d_y, d_r_post, d_k2_post, d_v2_post, d_g = [torch.empty_like(k) for _ in range(5)]
        call("tmix_post_bwd", k, *post_args, p(d_y), p(d_r_post), p(d_k2_post), p(d_v2_post), p(d_g), p(part_post), nb)
    d_wpre, d_k, d_v, d_apre, d_r = [torch.empty_like(k) for _ in range(5)]
    d_vpre = None if layer0 else torch.empty_like(k)
    d_vf = None if layer0 else torch.empty_like(k)
    part = torch.empty(nb, 5, D, dtype=torch.float32, device=DEV)
    two = lambda name: (C[name] + [None])[:2]
    gsum = [*two("dw"), *two("dk"), d_k2_post, C["dv"][0], d_v2_post, *two("da"), *two("db"), *two("dq"), d_r_post,
            None if layer0 else C.get("d_vf_next")]
    if compact:
        gsum += [dt_post, R["r"], P["r_k"], hscal]
    ptrs = (ctypes.c_void_p * len(gsum))(*[None if t is None else t.data_ptr() for t in gsum])
    call("tmix_prepare_bwd_sum_compact" if compact else "tmix_prepare_bwd_sum", k, cl(rows), D, p(R["w_pre"]), p(k), p(R["v"]), p(R["a_pre"]),
         p(R.get("v_pre")), p(R.get("v_first")), p(m), p(P["k_k"]), p(P["k_a"]), ptrs, p(d_wpre), p(d_k), p(d_v), p(d_apre), p(d_vpre),
         p(d_vf), p(d_r), p(part), nb)
    dp, dpp = fused._colsum(part, dtype), fused._colsum(part_post, dtype)
    torch.cuda.synchronize()
    grads = dict(r=d_r, w_pre=d_wpre, k=d_k, v=d_v, a_pre=d_apre, g=d_g, y=d_y, v_pre=d_vpre, v_first=d_vf)
    pgrads = dict(k_k=dp[0], k_a=dp[1], gn_weight=dpp[0], gn_bias=dpp[1], r_k=dpp[2])
    colsums = dict(w_pre=dp[2], a_pre=dp[3], v_pre=None if layer0 else dp[4])   # what fused._attach_colsums hands to the branches' biases
    return (k2, v2), grads, pgrads, colsums


def _pair_case(dtype, B, T, D, layer0, mask, compact, nsets, with_vf_next, nb, slab_seqs, seed):
    H = D // 64
    g = torch.Generator().manual_seed(seed)
    mk = lambda scale=1.0: _mk((B, T, D), g, scale, dtype)
    raw = dict(r=mk(), w_pre=mk(2.0), k=mk(), v=mk(), a_pre=mk(), g=mk(), y=mk(2.0))
    if not layer0:
        raw.update(v_pre=mk(), v_first=mk())
    par = dict(k_k=(_mk((D,), g, 0.3, dtype) + 0.7).to(dtype).float(), k_a=(_mk((D,), g, 0.1, dtype) + 1.0).to(dtype).float(),
               **_post_params(D, dtype, g))
    cot = dict(dout=mk(), dv=[mk()])
    for name in ("dw", "dq", "dk", "da", "db"):
        cot[name] = [mk() for _ in range(nsets)]
    if with_vf_next and not layer0:
        cot["d_vf_next"] = mk()
    stored, grads, pgrads, colsums = _pair_hip(dtype, raw, par, cot, mask, H, layer0, compact, nb)
    consts = dict(cot, mask=mask, k2_stored=stored[0].float().cpu(), v2_stored=stored[1].float().cpu())

    def loss(a, p):
        return (RF.tmix_pair_loss({k: a[k] for k in raw}, p, {k: a[k] for k in cot}, a.get("mask"), H, EPS_GN, layer0, rt=dtype,
                                  stored=(a["k2_stored"], a["v2_stored"]) if dtype == BF16 else None, round_post_grads=not compact),)

    _, ag, pg, _ = RF.eval_in_slabs(loss, raw, par, None, slab_seqs=slab_seqs, consts=consts)
    name = f"pair {'compact' if compact else 'full'} layer0={layer0} sets={nsets}"
    print(f"\n  {name} {dtype} rows {B * T} workgroups {nb}")
    prop_r = None
    if compact and dtype == BF16:
        # d_r += ds k2 r_k with k2 rebuilt in fp32 where the exact gradient has the stored bf16 k2: half an ulp of k2 (module docstring)
        ds = (cot["dout"].double() * raw["g"].double() * stored[1].double().cpu()).reshape(B, T, H, 64).sum(-1, keepdim=True)
        prop_r = (2.0 ** -8 * (ds * stored[0].double().cpu().reshape(B, T, H, 64) * par["r_k"].double().reshape(1, 1, H, 64)).abs()).reshape(B, T, D)
    props = {"r": prop_r} if prop_r is not None else {}
    if not compact and dtype == BF16:
        # k = 2 through the stored d_r / d_k2 / d_v2 of tmix_post_bwd: their ulp, carried through the prepare backward (which takes
        # d_k2 and d_v2 in channel by channel, so |d k2 / d input| applied to |d_k2| is the exact carry)
        k2s, v2s = consts["k2_stored"], consts["v2_stored"]
        post = lambda a, p: (RF.tmix_post(a["y"], a["r"], a["k2"], a["v2"], a["g"], p["gn_weight"], p["gn_bias"], p["r_k"], H, EPS_GN),)
        _, pa, _, _ = RF.eval_in_slabs(post, dict(y=raw["y"], r=raw["r"], k2=k2s, v2=v2s, g=raw["g"]),
                                       {k_: par[k_] for k_ in ("gn_weight", "gn_bias", "r_k")}, [cot["dout"]], slab_seqs=slab_seqs)
        prep = lambda a, p: RF.tmix_prepare(a["w_pre"], a["k"], a["v"], a["a_pre"], a.get("v_pre"), a.get("v_first"), p["k_k"], p["k_a"],
                                            a.get("mask"), H, layer0)[1:3]
        _, ca, _, _ = RF.eval_in_slabs(prep, {k_: v for k_, v in raw.items() if k_ not in ("r", "g", "y")}, dict(k_k=par["k_k"], k_a=par["k_a"]),
                                       [pa["k2"].abs(), pa["v2"].abs()], slab_seqs=slab_seqs, consts=dict(mask=mask))
        props = {k_: 2.0 ** -7 * ca[k_].abs() for k_ in ("k", "a_pre", "v", "v_pre", "v_first") if k_ in ca}
        props["r"] = 2.0 ** -7 * pa["r"].abs()
    for k_ in ag:
        _compare(grads[k_], ag[k_], f"{name} d{k_}", dtype, 1e-4, prop=props.get(k_))
    for k_ in pg:
        _cmp_param(pgrads[k_], pg[k_], f"{name} d{k_}", dtype)
    for k_, cs in colsums.items():
        if cs is not None:
            _cmp_param(cs, ag[k_].sum((0, 1)), f"{name} column sum of d{k_}", dtype)


def test_compact_backward_pair_at_the_training_shape():
    """What bf16 training launches (rwkv7_tmix_post_bwd_compact -> tmix_prepare_bwd_fast_kernel<.., true>) at 8 x 4096 x 1024 with the
    shipped 1024 workgroups: 32 rows per workgroup, left-padding mask, chained d_vf_next."""
    B, T, D = 8, 4096, 1024
    _pair_case(BF16, B, T, D, False, _mask_left_padding(B, T), True, 1, True, min(B * T, fused._BWD_BLOCKS), 1, seed=31)


@pytest.mark.parametrize("compact,nsets", [(True, 1), (True, 2), (False, 1), (False, 2)],
                         ids=["compact-fast", "compact-two-sets", "full-one-set", "full-two-sets"])
@pytest.mark.parametrize("layer0,masked,with_vf_next", [(True, True, False), (False, False, True), (False, True, False), (True, False, False)],
                         ids=["layer0-mask", "later-vfnext", "later-mask", "layer0"])
@pytest.mark.parametrize("B,T,D,blocks,run,dtype", AWKWARD, ids=AWKWARD_IDS)
def test_backward_pair_few_workgroups(B, T, D, blocks, run, dtype, layer0, masked, with_vf_next, compact, nsets, monkeypatch):
    """compact-fast: tmix_prepare_bwd_fast_kernel; compact-two-sets: the generic kernel's compact branch; full-*: rwkv7_tmix_post_bwd ->
    tmix_prepare_bwd_kernel<T, true> with one and with two gradient sets per tensor (the row-split scalar scan backward's hand-over)."""
    _patch_blocks(monkeypatch, blocks, run)
    mask = _mask_awkward(B, T, run) if masked else None
    _pair_case(dtype, B, T, D, layer0, mask, compact, nsets, with_vf_next, min(B * T, blocks), 2, seed=B * T + D + nsets)
