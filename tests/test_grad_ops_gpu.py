"""GPU (-m gpu): the entries of csrc/grad_ops.hip through ctypes -- sum of squares of a flat bf16 gradient, fp32 micro-batch
accumulate / fold, AdamW with the clip factor read from device memory (rwkvtts_amd/trainer.py's max_grad_norm / accumulate())."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
P = lambda t: ctypes.c_void_p(t.data_ptr())
f = ctypes.c_float


def _lib():
    from rwkvtts_amd import _lib as L
    return L.lib()


def _grad(n, seed, sign_seed=None):
    """bf16 values with magnitudes log-uniform over 1e-4 .. 10 and random signs (drawn from sign_seed if given)."""
    g = torch.Generator().manual_seed(seed)
    mag = torch.exp(torch.empty(n).uniform_(math.log(1e-4), math.log(10.0), generator=g))
    sign = torch.where(torch.rand(n, generator=g if sign_seed is None else torch.Generator().manual_seed(sign_seed)) < 0.5, -1.0, 1.0)
    return (mag * sign).bfloat16().to(DEV)


def _sumsq(lib, x, out, accumulate=0):
    ws = torch.empty(lib.rwkv7_grad_sumsq_workspace_bytes(x.numel()) // 4, dtype=torch.float32, device=DEV)
    assert ws.numel() == -(-x.numel() // 8192)
    rc = lib.rwkv7_grad_sumsq_bf16(ctypes.c_long(x.numel()), P(x), P(ws), P(out), accumulate, None)
    assert rc == 0
    torch.cuda.synchronize()


# 8192 = the tile of stage 1: one short tile, a tile short by one slab, exactly one, one slab over, several with a short last one,
# and more tiles than the 256 threads of stage 2 plus a short one
@pytest.mark.timeout(60)
@pytest.mark.parametrize("n,offset", [(128, 0), (8192 - 128, 0), (8192, 0), (8192 + 128, 0), (3 * 8192 + 384, 0), (2 ** 20 + 128, 0),
                                      (3 * 8192 + 384, 128)])
def test_sumsq_matches_float64_and_is_reproducible(n, offset):
    """Relative error <= 1e-5: every term is non-negative and the fp32 chain per tile is 32 sequential adds plus 8 tree levels
    (about 40 * 2^-24 = 2.4e-6); stage 2 is exact to double.  offset: a slice starting 128 elements (256 bytes) into its allocation."""
    lib = _lib()
    x = _grad(n + offset, n)[offset:]
    want = x.double().pow(2).sum().item()
    out = torch.full((1,), -7.0, device=DEV)
    _sumsq(lib, x, out)
    got = out.item()
    print(f"n={n} offset={offset}: got {got!r} want {want!r} rel {abs(got - want) / want:.3e}")
    assert abs(got - want) <= 1e-5 * want
    again = torch.zeros(1, device=DEV)
    _sumsq(lib, x, again)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32)), "two calls on the same data differ"
    _sumsq(lib, x, again, accumulate=1)
    assert again.item() == (out + out).item()


@pytest.mark.timeout(60)
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
@pytest.mark.parametrize("n,at", [(128, 77), (3 * 8192 + 384, 3 * 8192 + 383), (3 * 8192 + 384, 8192 + 5)])
def test_sumsq_of_a_buffer_with_one_non_finite_value_is_non_finite(bad, n, at):
    lib = _lib()
    x = _grad(n, 5)
    x[at] = bad
    out = torch.zeros(1, device=DEV)
    _sumsq(lib, x, out)
    assert not math.isfinite(out.item())


@pytest.mark.timeout(60)
def test_bad_arguments_return_an_error_without_launching():
    lib = _lib()
    x = _grad(256, 1)
    acc = torch.full((256,), 3.0, device=DEV)
    out = torch.full((1,), 5.0, device=DEV)
    ws = torch.zeros(1, device=DEV)
    n = ctypes.c_long
    assert lib.rwkv7_grad_sumsq_bf16(n(0), P(x), P(ws), P(out), 0, None) == -1
    assert lib.rwkv7_grad_sumsq_bf16(n(192), P(x), P(ws), P(out), 0, None) == -4
    assert lib.rwkv7_grad_sumsq_bf16(n(128), None, P(ws), P(out), 0, None) == -1
    assert lib.rwkv7_grad_sumsq_bf16(n(128), P(x), None, P(out), 0, None) == -1
    assert lib.rwkv7_grad_sumsq_bf16(n(128), P(x), P(ws), None, 0, None) == -1
    assert lib.rwkv7_grad_sumsq_bf16(n(128), P(x[1:]), P(ws), P(out), 0, None) == -4      # not 16-byte aligned
    assert lib.rwkv7_grad_accum_bf16(n(200), P(acc), P(x), 0, None) == -4
    assert lib.rwkv7_grad_accum_bf16(n(128), None, P(x), 0, None) == -1
    assert lib.rwkv7_grad_fold_bf16(n(200), P(acc), P(x), f(0.5), None) == -4
    assert lib.rwkv7_grad_fold_bf16(n(128), P(acc), None, f(0.5), None) == -1
    assert lib.rwkv7_grad_sumsq_workspace_bytes(0) == 0 and lib.rwkv7_grad_sumsq_workspace_bytes(8193) == 8
    torch.cuda.synchronize()
    assert out.item() == 5.0 and ws.item() == 0.0 and (acc == 3.0).all()


def _same_bits(a, b):
    """Bit for bit; where the value is a NaN, both are NaN (which NaN a conversion or an add returns is not a value)."""
    nan = torch.isnan(a)
    iv = torch.int32 if a.dtype == torch.float32 else torch.int16
    return torch.equal(nan, torch.isnan(b)) and torch.equal(a.view(iv)[~nan], b.view(iv)[~nan])


@pytest.mark.timeout(60)
@pytest.mark.parametrize("n", [128, 128 * 1023])
def test_accumulate_and_fold_equal_torch_bit_for_bit(n):
    """Three windows of k = 1, 2, 3 accumulates followed by the fold, against acc += g.float() and ((acc + g.float()) * inv).bfloat16()
    in torch: every step is one fp32 add or one multiply, and one rounding to bf16.  NaN and +-Inf among the gradients."""
    lib = _lib()
    acc = torch.full((n,), float("nan"), device=DEV)          # `first` must not read it
    for k in (1, 2, 3):
        want_acc = torch.zeros(n, device=DEV)
        for j in range(k):
            g = _grad(n, 10 * k + j)
            if j == 1:
                g[3], g[n - 1], g[64] = float("nan"), float("inf"), -float("inf")
            assert lib.rwkv7_grad_accum_bf16(ctypes.c_long(n), P(acc), P(g), int(j == 0), None) == 0
            want_acc += g.float()
            torch.cuda.synchronize()
            assert _same_bits(acc, want_acc), (k, j)
        g = _grad(n, 10 * k + 7)
        if k == 3:
            g[64] = float("inf")                             # -inf + inf in the fold
        inv = 1.0 / (k + 1)
        want = ((want_acc + g.float()) * torch.tensor(inv, dtype=torch.float32, device=DEV)).bfloat16()
        keep = acc.clone()
        assert lib.rwkv7_grad_fold_bf16(ctypes.c_long(n), P(acc), P(g), f(inv), None) == 0
        torch.cuda.synchronize()
        assert _same_bits(g, want), k
        assert _same_bits(acc, keep), "the fold must not write the fp32 sum"
        if k > 1:
            assert torch.isnan(g[3]) and torch.isinf(g[n - 1])


SIZES = [128 * 3, 128 * 1, 128 * 5, 128 * 2]          # four "parameters", slab aligned
GID = [0, 1, 2, 0]                                    # lr_1x, lr_2x, lr_decay, lr_1x
TAB = [[1.0, 0.0], [2.0, 0.0], [1.0, 0.1]]
LRS = [1e-3, 2e-3, 5e-4]


class _State:
    def __init__(self, p0):
        n = p0.numel()
        self.n = n
        self.p32 = p0.clone().to(DEV)
        self.m, self.v = torch.zeros_like(self.p32), torch.zeros_like(self.p32)
        self.p16 = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
        self.slab = torch.cat([torch.full((s // 128,), k, dtype=torch.uint8) for s, k in zip(SIZES, GID)]).to(DEV)
        self.gtab = torch.tensor(TAB, dtype=torch.float32, device=DEV)

    def plain(self, lib, gr, lr, i, flag):
        rc = lib.rwkv7_adamw_groups_bf16(ctypes.c_long(self.n), P(self.p32), P(gr), P(self.m), P(self.v), P(self.p16), P(self.slab),
                                         P(self.gtab), 3, P(flag), f(lr), f(0.9), f(0.95), f(1e-18), i + 1, None)
        assert rc == 0
        torch.cuda.synchronize()

    def clip(self, lib, gr, lr, i, flag, sumsq, max_norm):
        rc = lib.rwkv7_adamw_groups_clip_bf16(ctypes.c_long(self.n), P(self.p32), P(gr), P(self.m), P(self.v), P(self.p16), P(self.slab),
                                              P(self.gtab), 3, P(flag), P(sumsq), f(max_norm), f(lr), f(0.9), f(0.95), f(1e-18), i + 1,
                                              None)
        assert rc == 0
        torch.cuda.synchronize()

    def same(self, o):
        return all(_same_bits(a, b) for a, b in ((self.p32, o.p32), (self.m, o.m), (self.v, o.v), (self.p16, o.p16)))


def _p0():
    return torch.randn(sum(SIZES), generator=torch.Generator().manual_seed(1))


@pytest.mark.timeout(60)
@pytest.mark.parametrize("max_norm", [None, float("inf")], ids=["below-max-norm", "measure-only"])
def test_adamw_clip_with_factor_one_is_bit_identical_to_the_plain_entry(max_norm):
    lib = _lib()
    a, b = _State(_p0()), _State(_p0())
    flag = torch.zeros(1, device=DEV)
    sumsq = torch.zeros(1, device=DEV)
    for i, lr in enumerate(LRS):
        gr = _grad(a.n, 40 + i)
        _sumsq(lib, gr, sumsq)
        mn = max_norm if max_norm is not None else 1.001 * math.sqrt(sumsq.item())      # sumsq below max_norm^2
        a.plain(lib, gr, lr, i, flag)
        b.clip(lib, gr, lr, i, flag, sumsq, mn)
        assert a.same(b), i


@pytest.mark.timeout(60)
def test_adamw_clip_at_half_the_norm_matches_torch_adamw_with_clip_grad_norm():
    """sumsq from the sumsq kernel, max_norm = half the true norm, against torch.optim.AdamW + clip_grad_norm_ on fp32 copies of
    the gradients.  p32 at the bar of the plain entry's test (2e-6 * max(1, |want|max)), p16 == p32.bfloat16(); m and v within 3e-5
    relative: the 1e-5 bar of the norm, doubled for the square, plus fp32 rounding.  An element keeps its sign over the three
    steps, so that exp_avg is a sum of terms of one sign and an element-wise relative bar is meaningful for it."""
    lib = _lib()
    p0 = _p0()
    n = p0.numel()
    offs = [sum(SIZES[:i]) for i in range(len(SIZES))]
    refs = [p0[o:o + s].clone().to(DEV).requires_grad_(True) for o, s in zip(offs, SIZES)]
    opt = torch.optim.AdamW([{"params": [r for r, gi in zip(refs, GID) if gi == k], "weight_decay": TAB[k][1], "scale": TAB[k][0]}
                             for k in range(3)], lr=1e-3, betas=(0.9, 0.95), eps=1e-18)
    st = _State(p0)
    flag = torch.zeros(1, device=DEV)
    sumsq = torch.zeros(1, device=DEV)
    for i, lr in enumerate(LRS):
        gr = _grad(n, 50 + i, sign_seed=50)
        max_norm = 0.5 * gr.double().pow(2).sum().sqrt().item()
        for grp in opt.param_groups:
            grp["lr"] = lr * grp["scale"]
        for r, o, s in zip(refs, offs, SIZES):
            r.grad = gr[o:o + s].float()
        norm = torch.nn.utils.clip_grad_norm_(refs, max_norm)
        assert norm.item() > 1.9 * max_norm
        opt.step()
        _sumsq(lib, gr, sumsq)
        st.clip(lib, gr, lr, i, flag, sumsq, max_norm)
        want = torch.cat([r.detach() for r in refs])
        wm = torch.cat([opt.state[r]["exp_avg"] for r in refs])
        wv = torch.cat([opt.state[r]["exp_avg_sq"] for r in refs])
        print(f"step {i}: p32 {(st.p32 - want).abs().max().item():.3e}  m rel {((st.m - wm).abs() / wm.abs()).max().item():.3e}  "
              f"v rel {((st.v - wv).abs() / wv).max().item():.3e}")
        assert (st.p32 - want).abs().max().item() <= 2e-6 * max(1.0, want.abs().max().item()), i
        assert torch.equal(st.p16, st.p32.bfloat16())
        assert ((st.m - wm).abs() <= 3e-5 * wm.abs()).all() and ((st.v - wv).abs() <= 3e-5 * wv).all(), i


@pytest.mark.timeout(60)
@pytest.mark.parametrize("case", ["sumsq-nan", "sumsq-inf", "flag-and-finite-clip"])
def test_adamw_clip_skips_like_the_plain_entry_with_the_flag_set(case):
    """A non-finite *sumsq with NaN gradients, or the skip flag together with a finite clip: bit-identical to rwkv7_adamw_groups_bf16
    with the skip flag set (the update of a zero gradient), nothing becomes NaN."""
    lib = _lib()
    a, b = _State(_p0()), _State(_p0())
    zero, one = torch.zeros(1, device=DEV), torch.ones(1, device=DEV)
    sumsq = torch.zeros(1, device=DEV)
    gr = _grad(a.n, 60)
    a.plain(lib, gr, 1e-3, 0, zero)                       # non-zero moments first
    b.plain(lib, gr, 1e-3, 0, zero)
    nan_g = torch.full((a.n,), float("nan"), dtype=torch.bfloat16, device=DEV)
    a.plain(lib, nan_g, 1e-3, 1, one)
    if case == "flag-and-finite-clip":
        _sumsq(lib, gr, sumsq)
        b.clip(lib, nan_g, 1e-3, 1, one, sumsq, 0.5 * math.sqrt(sumsq.item()))
    else:
        sumsq.fill_(float("nan") if case == "sumsq-nan" else float("inf"))
        b.clip(lib, nan_g, 1e-3, 1, zero, sumsq, 1.0)
    assert all(torch.isfinite(t.float()).all() for t in (b.p32, b.m, b.v, b.p16))
    assert a.same(b)


@pytest.mark.timeout(60)
def test_adamw_clip_argument_errors_return_before_any_launch():
    lib = _lib()
    s = _State(_p0())
    keep = s.p32.clone()
    gr = _grad(s.n, 70)
    sumsq = torch.ones(1, device=DEV)

    def call(n=s.n, slab=s.slab, gtab=s.gtab, ss=sumsq, max_norm=1.0, step=1):
        return lib.rwkv7_adamw_groups_clip_bf16(ctypes.c_long(n), P(s.p32), P(gr), P(s.m), P(s.v), P(s.p16),
                                                None if slab is None else P(slab), None if gtab is None else P(gtab), 3, None,
                                                None if ss is None else P(ss), f(max_norm), f(1e-3), f(0.9), f(0.95), f(1e-8), step, None)
    assert call(ss=None) == -1
    assert call(max_norm=-1.0) == -1 and call(max_norm=float("nan")) == -1
    assert call(gtab=None) == -1          # table without groups
    assert call(step=0) == -1
    assert call(n=s.n - 4) == -4          # n % 128 != 0 with groups
    torch.cuda.synchronize()
    assert torch.equal(s.p32, keep)
