"""GPU (-m gpu): rwkv7_kl_acc_fwd_bwd_bf16 and what is built on it (losses.fused_linear_kl_accuracy, RWKV7LM(fused_loss=True),
RWKV7CosyConfig(fused_loss=True)) against the fp64 restatement of the row formulas in tests/cosy_head_ref.py ON THE SAME bf16 LOGITS.

Bars (taken from the reference chain and the number formats, nothing tuned on the kernel):
  loss_rows : |hip - exact| <= 2 max_rows|fp32_chain - exact| + V 2^-24 max(|x|, lse) of the row; fp32_chain is label_smoothing_kl's
              per-row arithmetic in fp32 on the same logits
  dlogits   : |hip - exact| <= one bf16 ulp of the exact value + V 2^-24 scale
  correct_rows, ignored rows (0 in all three outputs), columns V .. ld - 1 (bits kept): exact
  gradients of the fused function / model: error(fused) <= 1.1 error(parent's bf16 autograd chain) + V 2^-24 max|exact|, both errors
              against the same fp64 (function) or fp32-model (model) values.  error = RMS of the difference over the tensor.
              Denominators are ordinary ones (200 valid rows, batch 3, 15 valid tokens).  Where the host knows the denominator (batch
              size; n_valid, which RWKV7LM passes) it is inside the kernel's scale and d loss / d logits is rounded from the same fp32
              value as in the parent: ratios of 1.00.  Where only the device knows it (normalize_length without n_valid) d loss /
              d logits is rounded before the division instead of after it -- same places, other VALUES -- and the ratio is not 1:
              emulating both orders on the CPU gives 0.77 .. 0.83 for dh and dw at 200 rows, and up to 1.05 just below a power of two
              (255 rows), where db (51 elements) scatters up to 1.2.
              RWKV7CosyLM(fused_loss) rounds d loss / d logits twice (losses._KLFromLogits): its head gradients get 1.1 sqrt(2).
Every comparison prints `RATIO <case> <observable> <error / bar>`; the record of one run is profiles/cosy_head_parity.txt."""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F

from cosy_head_ref import exact_rows, fp32_chain_rows
from rwkvtts_amd import layouts as L, losses
from rwkvtts_amd.cosy_llm import RWKV7CosyConfig, RWKV7CosyLM, RWKV7LM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN_BITS = 0x7FC1   # a quiet NaN with a payload: padding columns must keep it bit for bit
SHAPES = [(1, 2, 2), (5, 11, 11), (67, 257, 263), (33, 6562, 6562), (33, 6562, 6656), (3, 8193, 8193)]


def _bits(t):
    return t.view(torch.int16)


def _make(rows, V, ld, seed, amp=3.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.full((rows, ld), NAN_BITS, dtype=torch.int16).view(torch.bfloat16)
    x[:, :V] = (torch.randn(rows, V, generator=g) * amp).bfloat16()
    labels = torch.randint(0, V, (rows,), generator=g)
    labels[0] = 0
    if rows > 1:
        labels[1] = V - 1
    labels[2::3] = -1   # a third of the rows ignored
    return x.to(DEV), labels.to(DEV)


def _call(hip_lib, x, labels, V, s, scale, in_place, shift=0):
    """the entry point on a [rows, ld] buffer; returns (dlogits buffer, loss_rows, correct_rows).  shift: dlogits starts that many
    elements into its allocation (logits and dlogits then differ modulo 16 bytes: the kernel's 2-byte route)"""
    rows, ld = x.shape
    src = x.clone()
    dst = src
    if not in_place:   # same padding pattern; the V columns are overwritten by the kernel
        flat = torch.full((rows * ld + shift,), NAN_BITS, dtype=torch.int16, device=DEV).view(torch.bfloat16)
        dst = flat[shift:].view(rows, ld)
        dst.copy_(x)
        dst[:, :V] = 7.0
        assert (dst.data_ptr() - src.data_ptr()) % 16 == (2 * shift) % 16
    loss = torch.full((rows,), -1.0, dtype=torch.float32, device=DEV)
    corr = torch.full((rows,), -1, dtype=torch.int32, device=DEV)
    rc = hip_lib.rwkv7_kl_acc_fwd_bwd_bf16(
        ctypes.c_long(rows), ctypes.c_int(V), ctypes.c_long(ld), ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()),
        ctypes.c_void_p(labels.data_ptr()), ctypes.c_long(-1), ctypes.c_float(s), ctypes.c_float(scale),
        ctypes.c_void_p(loss.data_ptr()), ctypes.c_void_p(corr.data_ptr()),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    if not in_place:
        assert torch.equal(_bits(src), _bits(x)), "out of place: the logits were modified"
        assert shift == 0 or (_bits(flat[:shift]) == NAN_BITS).all(), "elements in front of the dlogits buffer were written"
    return dst, loss, corr


def _bf16_ulp(v):
    """one bf16 ulp at the magnitude of v (fp64), never below the smallest normal's"""
    e = torch.floor(torch.log2(v.abs().clamp(min=2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64, device=v.device), e - 7)


def _check(hip_lib, name, x, labels, V, s, scale, shifted=False):
    rows, ld = x.shape
    xs = x[:, :V]
    e_loss, e_d, e_corr, lse = exact_rows(xs, labels, s)
    chain = fp32_chain_rows(xs, labels, s).double()
    chain_err = (chain - e_loss).abs().max()
    loss_bar = 2 * chain_err + V * 2.0 ** -24 * torch.maximum(xs.double().abs().max(1).values, lse.abs())
    d_bar = _bf16_ulp(e_d * scale) + V * 2.0 ** -24 * scale
    valid = labels != -1
    for in_place, shift in ((True, 0), (False, 0)) + (((False, 1),) if shifted else ()):
        tag = f"{name} s={s} {'in-place' if in_place else 'out-of-place'}" + (" dlogits-off-by-2-bytes" if shift else "")
        d, loss, corr = _call(hip_lib, x, labels, V, s, scale, in_place, shift)
        assert torch.equal(_bits(d[:, V:]), _bits(x[:, V:])), f"{tag}: padding columns changed"
        assert torch.equal(corr.long(), e_corr), f"{tag}: correct_rows"
        assert (loss[~valid] == 0).all() and (corr[~valid] == 0).all() and (_bits(d[:, :V])[~valid] == 0).all(), f"{tag}: ignored rows"
        assert torch.isfinite(loss).all() and torch.isfinite(d[:, :V].float()).all(), tag
        r_loss = ((loss.double() - e_loss).abs() / loss_bar).max().item()
        r_d = ((d[:, :V].double() - e_d * scale).abs() / d_bar).max().item()
        print(f"RATIO {tag} loss_rows {r_loss:.3f} (fp32 chain's own error {chain_err.item():.3e})")
        print(f"RATIO {tag} dlogits {r_d:.3f}")
        assert r_loss <= 1.0, f"{tag}: loss_rows {r_loss} x the bar"
        assert r_d <= 1.0, f"{tag}: dlogits {r_d} x the bar"


@pytest.mark.parametrize("s", [0.0, 0.1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda t: "x".join(map(str, t)))
def test_kernel_against_fp64_rows(hip_lib, shape, s):
    rows, V, ld = shape
    x, labels = _make(rows, V, ld, seed=rows + V)
    # logits and dlogits that differ modulo 16 bytes: once in a register-sized row, once in a two-pass one
    _check(hip_lib, "x".join(map(str, shape)), x, labels, V, s, scale=0.37 if V == 257 else 1.0, shifted=shape in SHAPES[3::2])


def test_kernel_all_rows_ignored(hip_lib):
    x, labels = _make(33, 6562, 6656, seed=1)
    labels[:] = -1
    _check(hip_lib, "all-ignored", x, labels, 6562, 0.1, 1.0)


@pytest.mark.parametrize("shape", [(67, 257, 263), (33, 6562, 6562)], ids=lambda t: "x".join(map(str, t)))
def test_kernel_logits_of_magnitude_80(hip_lib, shape):
    rows, V, ld = shape
    x, labels = _make(rows, V, ld, seed=80, amp=30.0)
    x[:, :V] = x[:, :V].clamp(-80, 80)
    x[0, 1], x[0, 0] = 80.0, -80.0    # label 0 at -80 under a maximum of +80
    x[1, V - 1] = 80.0                # label V - 1 is the maximum
    x[3, :V] = -80.0                  # a whole row at -80
    _check(hip_lib, "pm80-" + "x".join(map(str, shape)), x, labels, V, 0.1, 1.0)


def test_kernel_planted_ties(hip_lib):
    V = 6562
    x, labels = _make(12, V, V, seed=7)
    labels[:] = torch.randint(0, V, (12,))
    top = 40.0
    plant = [((5, 6000), 6000, 0), ((5, 6000), 5, 1),          # first piece against a late piece: two threads, two waves
             ((100, 6561), 6561, 0), ((100, 6561), 100, 1),    # a piece against the last single element
             ((3000, 3001), 3001, 0), ((3000, 3001), 3000, 1),  # neighbours inside one 16-byte piece
             ((0, 1, V - 1), 0, 1), ((0, 1, V - 1), 1, 0)]
    for r, (cols, lab, _) in enumerate(plant):
        for c in cols:
            x[r, c] = top
        labels[r] = lab
    x[8, :] = 1.0
    labels[8] = 0          # the whole row tied: index 0 wins
    x[9, :] = 1.0
    labels[9] = 17
    x[10, labels[10]] = top   # an untied hit
    labels[11] = -1
    want = [w for _, _, w in plant] + [1, 0, 1, 0]
    assert exact_rows(x, labels, 0.1)[2].tolist() == want
    assert (x.cpu().float().argmax(1) == labels.cpu()).long().tolist()[:11] == want[:11]   # torch.argmax on the CPU
    _check(hip_lib, "ties", x, labels, V, 0.1, 1.0)
    # the same rows on 16-byte aligned rows (ld % 8 == 0)
    xa, _ = _make(12, V, 6568, seed=8)
    xa[:, :V] = x
    _check(hip_lib, "ties-aligned", xa, labels, V, 0.1, 1.0)


def _rms(t):
    return t.double().pow(2).mean().sqrt().item()


def _rule(tag, fused, parent, exact, V, factor=1.1):
    ef, ep = _rms(fused.double() - exact.double()), _rms(parent.double() - exact.double())
    floor = V * 2.0 ** -24 * exact.abs().max().item()
    print(f"RATIO {tag} fused-error {ef:.4e} parent-error {ep:.4e} ratio {ef / max(ep, 1e-300):.4f} floor {floor:.2e}")
    assert ef <= factor * ep + floor, f"{tag}: fused error {ef:.4e} > {factor:.3f} x parent's {ep:.4e} + {floor:.2e}"


@pytest.mark.parametrize("s,nl,n_valid", [(0.1, True, None), (0.0, False, None), (0.1, True, 200)])
def test_fused_function_against_the_unfused_pair_and_fp64_gradients(hip_lib, s, nl, n_valid):
    rows, D, V, B = 300, 128, 51, 3
    g = torch.Generator().manual_seed(11)
    h = (torch.randn(rows, D, generator=g)).bfloat16().to(DEV).requires_grad_(True)
    w = (torch.randn(V, D, generator=g) * 0.2).bfloat16().to(DEV).requires_grad_(True)
    b = (torch.randn(V, generator=g) * 0.1).bfloat16().to(DEV).requires_grad_(True)
    labels = torch.randint(0, V, (rows,), generator=g)
    labels[torch.randperm(rows, generator=g)[:100]] = -1   # 200 valid rows
    labels = labels.to(DEV)
    hits = losses.KL_ACC_HITS[0]
    loss, acc = losses.fused_linear_kl_accuracy(h, labels, w, b, B, s, nl, ignore_index=-1, chunk=128,
                                                n_valid=n_valid)   # chunks of 128, 128, 44 rows
    assert losses.KL_ACC_HITS[0] == hits + 3, "the HIP kernel was not launched once per chunk"
    gf = torch.autograd.grad(loss, [h, w, b])
    logits = F.linear(h, w, b)
    p_loss = losses.label_smoothing_kl(logits.unsqueeze(0), labels.unsqueeze(0), V, -1, s, nl)
    p_loss = p_loss if nl else p_loss / B
    assert losses.KL_ACC_HITS[0] == hits + 3
    p_acc = losses.th_accuracy(logits, labels.unsqueeze(0), -1)
    gp = torch.autograd.grad(p_loss, [h, w, b])
    denom = 200 if nl else B
    e_loss, e_d, e_corr, lse = exact_rows(logits.detach(), labels, s)
    assert acc.item() == p_acc.item() == e_corr.sum().item() / 200
    exact = e_loss.sum().item() / denom
    bar = 2 * abs(p_loss.item() - exact) + V * 2.0 ** -24 * max(logits.abs().max().item(), lse.abs().max().item())
    assert int((labels != -1).sum()) == 200
    print(f"RATIO function s={s} nl={nl} n_valid={n_valid} loss {abs(loss.item() - exact) / bar:.3f}")
    assert abs(loss.item() - exact) <= bar
    e_d = e_d / denom
    h64, w64 = h.detach().double(), w.detach().double()
    for name, f_, p_, e_ in (("dh", gf[0], gp[0], e_d @ w64), ("dw", gf[1], gp[1], e_d.t() @ h64), ("db", gf[2], gp[2], e_d.sum(0))):
        assert f_.dtype == torch.bfloat16
        _rule(f"function s={s} nl={nl} n_valid={n_valid} {name}", f_, p_, e_, V)


SMALL = dict(hidden_size=128, num_hidden_layers=2, decay_low_rank_dim=32, a_low_rank_dim=32, v_low_rank_dim=16, gate_low_rank_dim=32)


def _to(batch, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}


def _batch():
    # unequal lengths; 10 + 1 and 3 + 1 valid targets: 15
    return _to(L.cosy_collate([[3, 4, 5, 6], [7, 8]], [list(range(10, 20)), [20, 21, 22]], pad_to_max_length=False), DEV)


def _targets(batch):
    """the flattened training targets of the Cosy layout: -1 over [sos, text, task_id], the speech ids, EOS = 50; shifted by one"""
    rows = [[-1] * (2 + int(nt)) + sp[:int(ns)].tolist() + [50]
            for sp, nt, ns in zip(batch["speech_token"], batch["text_token_len"], batch["speech_token_len"])]
    width = max(map(len, rows))
    return torch.tensor([r + [-1] * (width - len(r)) for r in rows], device=DEV)[:, 1:].reshape(-1)


def _tie_free_parent(batch, lab):
    """RWKV7LM (bf16, default loss) on the tiny Cosy model with the first seed of a fixed list for which no valid row of the batch has an
    argmax tie in its bf16 logits (logits of magnitude 0.5 have a bf16 spacing of 2^-9 .. 2^-8: about one seed in two has a tied row);
    returns (wrapper, seed)."""
    cfg = RWKV7CosyConfig(vocab_size=200, speech_token_size=50, **SMALL)
    for seed in (4, 5, 6, 7, 8, 9, 10, 11):
        llm = RWKV7CosyLM(cfg).init_weights(seed=seed)
        torch.manual_seed(seed)
        m = RWKV7LM(128, 128, 50, llm, lsm_weight=0.1).to(torch.bfloat16).to(DEV).train()
        seen = {}
        hook = llm.lm_head.register_forward_hook(lambda mod, args, out: seen.__setitem__("logits", out.detach()))
        with torch.no_grad():
            m(batch)
        hook.remove()
        top2 = seen["logits"].reshape(-1, 51).float().topk(2, dim=1).values[lab != -1]
        if (top2[:, 0] > top2[:, 1]).all():
            return m, seed
    raise AssertionError("every seed of the list gives an argmax tie")


def test_rwkv7lm_fused_loss_against_the_default_and_the_fp32_model(hip_lib):
    batch = _batch()
    lab = _targets(batch)
    assert int((lab != -1).sum()) == 15
    parent, seed = _tie_free_parent(batch, lab)
    m32 = copy.deepcopy(parent).float().train()   # the bf16 weights' values in an fp32 model
    fused = RWKV7LM(128, 128, 50, parent.llm, lsm_weight=0.1, fused_loss=True).to(torch.bfloat16).to(DEV).train()
    fused.load_state_dict(parent.state_dict())
    names = [n for n, _ in parent.named_parameters()]
    assert names == [n for n, _ in fused.named_parameters()] == [n for n, _ in m32.named_parameters()]

    def run(m):
        r = m(batch)
        gs = torch.autograd.grad(r["loss"], list(m.parameters()), allow_unused=True)
        return r["loss"].detach(), r["acc"], gs

    seen = {}   # the bf16 logits of the parent's forward
    hook = parent.llm.lm_head.register_forward_hook(lambda mod, args, out: seen.__setitem__("logits", out.detach()))
    lp, ap, gp = run(parent)
    hook.remove()
    hits = losses.KL_ACC_HITS[0]
    lf, af, gf = run(fused)
    assert losses.KL_ACC_HITS[0] == hits + 1
    l32, a32, g32 = run(m32)
    x = seen["logits"].reshape(-1, 51)
    top2 = x.float().topk(2, dim=1).values[lab != -1]
    assert (top2[:, 0] > top2[:, 1]).all(), f"argmax tie in the chosen batch (seed {seed})"
    assert af.item() == ap.item() == a32.item()
    e_loss, _, _, lse = exact_rows(x, lab, 0.1)
    exact = e_loss.sum().item() / 15
    bar = 2 * abs(lp.item() - exact) + 51 * 2.0 ** -24 * max(x.abs().max().item(), lse.abs().max().item())
    print(f"RATIO model loss {abs(lf.item() - exact) / bar:.3f} (fused {lf.item():.7f} parent {lp.item():.7f} exact {exact:.7f})")
    assert abs(lf.item() - exact) <= bar
    checked = 0
    for n, a, b, c in zip(names, gf, gp, g32):
        assert (a is None) == (b is None) == (c is None), n
        if a is None:
            continue
        _rule(f"model {n}", a, b, c, 51)
        checked += 1
    assert checked > 20


def test_cosy_lm_fused_loss_keeps_the_logits_bit_for_bit(hip_lib):
    cfg = RWKV7CosyConfig(vocab_size=200, speech_token_size=50, lsm_weight=0.1, **SMALL)
    a = RWKV7CosyLM(cfg).init_weights(seed=4).to(torch.bfloat16).to(DEV).train()
    b = RWKV7CosyLM(RWKV7CosyConfig.from_dict(dict(cfg.to_dict(), fused_loss=True))).to(torch.bfloat16).to(DEV).train()
    b.load_state_dict(a.state_dict())
    assert b.config.fused_loss and not a.config.fused_loss
    batch = _batch()
    hits = losses.KL_ACC_HITS[0]
    oa, ob = a(batch=batch), b(batch=batch)
    assert losses.KL_ACC_HITS[0] == hits + 1
    assert torch.equal(_bits(oa.logits), _bits(ob.logits))
    _, _, labels = a.build_inputs(batch)
    x, lab = oa.logits.detach().reshape(-1, 51), labels.reshape(-1)
    e_loss, e_d, _, lse = exact_rows(x, lab, 0.1)
    exact = e_loss.sum().item() / 15
    bar = 2 * abs(oa.loss.item() - exact) + 51 * 2.0 ** -24 * max(x.abs().max().item(), lse.abs().max().item())
    print(f"RATIO cosy-lm loss {abs(ob.loss.item() - exact) / bar:.3f}")
    assert abs(ob.loss.item() - exact) <= bar
    ga = torch.autograd.grad(oa.loss, [a.lm_head.weight, a.lm_head.bias])
    gb = torch.autograd.grad(ob.loss, [b.lm_head.weight, b.lm_head.bias])
    with torch.no_grad():
        emb, mask, _ = a.build_inputs(batch)
        h = a.model(inputs_embeds=emb, attention_mask=mask)[0].reshape(-1, 128).double()
    e_d = e_d / 15
    _rule("cosy-lm lm_head.weight", gb[0], ga[0], e_d.t() @ h, 51, factor=1.1 * 2 ** 0.5)
    _rule("cosy-lm lm_head.bias", gb[1], ga[1], e_d.sum(0), 51, factor=1.1 * 2 ** 0.5)
    # labels=None: nothing changes
    with torch.no_grad():
        assert torch.equal(_bits(a(inputs_embeds=emb, attention_mask=mask).logits), _bits(b(inputs_embeds=emb, attention_mask=mask).logits))
        assert b(inputs_embeds=emb, attention_mask=mask).loss is None
