"""CPU: the Cosy head's fused loss + accuracy (losses.fused_linear_kl_accuracy, rwkv7_kl_acc_fwd_bwd_bf16).  The closed form the kernel
implements (cosy_head_ref.exact_rows, fp64) against losses.label_smoothing_kl / th_accuracy, the CPU route of the fused function, the
opt-in switches, and the entry point's argument checks."""
import ctypes
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import load_golden
from cosy_head_ref import entropy_constant, exact_rows
from rwkvtts_amd import losses
from rwkvtts_amd.cosy_llm import RWKV7CosyConfig, RWKV7LM


def _closed_form(x, target, s, normalize_length, batch):
    loss_rows, _, correct, _ = exact_rows(x, target, s)
    n = (target != -1).sum()
    return loss_rows.sum() / (n if normalize_length else batch), correct.sum() / n


# fp32 chain against fp64: log_softmax and the V-term row sums carry a few fp32 roundings each; 1e-5 relative is ~100 ulp
REL = 1e-5


@pytest.mark.parametrize("s", [0.0, 0.1])
@pytest.mark.parametrize("nl", [False, True])
def test_closed_form_equals_label_smoothing_kl_on_the_committed_vectors(s, nl):
    g = load_golden("layouts.npz")
    x, t = g["ls.logits"], g["ls.target"]
    loss, acc = _closed_form(x.reshape(-1, 11), t.reshape(-1), s, nl, x.shape[0])
    want = losses.label_smoothing_kl(x, t, 11, -1, s, nl)
    assert abs(loss.item() - want.item()) <= REL * abs(want.item())
    key = f"ls.loss_{s}_{int(nl)}"
    if key in g:   # the reference's own numbers
        assert abs(loss.item() - g[key].item()) <= REL * abs(g[key].item())
    assert acc.item() == losses.th_accuracy(x.view(-1, 11), t, -1).item() == g["ls.acc"].item()


@pytest.mark.parametrize("s", [0.0, 0.1])
@pytest.mark.parametrize("nl", [False, True])
@pytest.mark.parametrize("V", [2, 257])
def test_closed_form_equals_label_smoothing_kl_on_random_rows(s, nl, V):
    gen = torch.Generator().manual_seed(V)
    B, T = 3, 13
    x = (torch.randn(B, T, V, generator=gen) * 3).bfloat16().float()   # bf16-valued: exact ties occur
    t = torch.randint(0, V, (B, T), generator=gen)
    t[0, :5] = -1
    t[1, 0], t[1, 1] = 0, V - 1
    hit = x[2].argmax(-1)
    t[2, :6] = hit[:6]   # some correct rows
    loss, acc = _closed_form(x.reshape(-1, V), t.reshape(-1), s, nl, B)
    want = losses.label_smoothing_kl(x, t, V, -1, s, nl)
    assert abs(loss.item() - want.item()) <= REL * abs(want.item())
    want_acc = losses.th_accuracy(x.view(-1, V), t, -1)
    assert want_acc.item() > 0 and abs(acc.item() - want_acc.item()) < 1e-7


def test_entropy_constant_is_kl_divs_zero_target_convention():
    # s = 0: every off-target class has t = 0 and contributes 0 (F.kl_div's xlogy), the target contributes 1 ln 1 = 0
    assert entropy_constant(11, 0.0) == 0.0
    x = torch.randn(4, 11)
    t = torch.tensor([0, 10, 3, 3])
    assert torch.allclose(exact_rows(x, t, 0.0)[0].float(), F.cross_entropy(x, t, reduction="none"), atol=1e-6)


def test_tie_rule_is_the_lowest_index_among_the_maxima():
    x = torch.zeros(4, 9)
    x[0, 2] = x[0, 5] = 4.0   # label 5 tied with the lower index 2 -> wrong
    x[1, 2] = x[1, 5] = 4.0   # label 2 is the lowest of the tied maxima -> right
    x[2, :] = 1.0             # everything tied: only label 0 is right
    x[3, :] = 1.0
    t = torch.tensor([5, 2, 0, 8])
    assert exact_rows(x, t, 0.1)[2].tolist() == [0, 1, 1, 0]
    assert x.argmax(1).tolist() == [2, 2, 0, 0]   # torch.argmax on the CPU
    assert losses.th_accuracy(x, t.unsqueeze(0), -1).item() == 0.5


@pytest.mark.parametrize("s,nl", [(0.0, True), (0.1, True), (0.1, False)])
def test_fused_function_on_the_cpu_equals_the_unfused_pair_and_autograd(s, nl):
    torch.manual_seed(3)
    B, T, D, V = 2, 9, 16, 23
    h = torch.randn(B, T, D, requires_grad=True)
    lin = nn.Linear(D, V)
    t = torch.randint(0, V, (B, T))
    t[0, :4] = -1
    loss, acc = losses.fused_linear_kl_accuracy(h, t, lin.weight, lin.bias, B, s, nl, ignore_index=-1, chunk=7)
    gh, gw, gb = torch.autograd.grad(loss, [h, lin.weight, lin.bias])
    h2 = h.detach().clone().requires_grad_(True)
    logits = lin(h2)
    want = losses.label_smoothing_kl(logits, t, V, -1, s, nl)
    want_acc = losses.th_accuracy(logits.view(-1, V), t, -1)
    wh, ww, wb = torch.autograd.grad(want, [h2, lin.weight, lin.bias])
    assert not acc.requires_grad
    assert abs(loss.item() - want.item()) <= 1e-6 * abs(want.item()) and acc.item() == want_acc.item()
    for a, b in ((gh, wh), (gw, ww), (gb, wb)):
        assert (a - b).abs().max().item() <= 1e-6 * b.abs().max().item()
    # ... and the closed form's gradient: d loss / d logits = (softmax - true_dist) / denominator
    d = exact_rows(logits.detach().reshape(-1, V), t.reshape(-1), s)[1] / ((t != -1).sum().item() if nl else B)
    assert ((d.t() @ h.detach().reshape(-1, D).double()).float() - gw).abs().max().item() <= 1e-5 * gw.abs().max().item()


def test_fused_function_with_nothing_valid_returns_what_the_pair_returns():
    h, lin = torch.randn(1, 4, 8), nn.Linear(8, 5)
    t = torch.full((1, 4), -1)
    for nl in (False, True):
        loss, acc = losses.fused_linear_kl_accuracy(h, t, lin.weight, lin.bias, 1, 0.1, nl)
        want = losses.label_smoothing_kl(lin(h), t, 5, -1, 0.1, nl)
        assert torch.isnan(acc) and (torch.isnan(loss) if nl else loss.item() == 0.0) and torch.isnan(want) == torch.isnan(loss)


class _StubLLM(nn.Module):
    """What RWKV7LM needs of its llm, on the CPU: .model (hidden states first), .lm_head, get_input_embeddings, .logits of a call."""

    def __init__(self, D, V, text_vocab):
        super().__init__()
        self.text = nn.Embedding(text_vocab, D)
        self.mix = nn.Linear(D, D)
        self.lm_head = nn.Linear(D, V)

    def model(self, inputs_embeds=None, attention_mask=None):
        return (torch.tanh(self.mix(inputs_embeds)).cumsum(1) * attention_mask.unsqueeze(-1),)

    def get_input_embeddings(self):
        return self.text

    def forward(self, inputs_embeds=None, attention_mask=None):
        return types.SimpleNamespace(logits=self.lm_head(self.model(inputs_embeds, attention_mask)[0]))


@pytest.mark.parametrize("nl", [False, True])
def test_rwkv7lm_fused_loss_equals_the_default_on_the_cpu(nl):
    from rwkvtts_amd import layouts as L
    torch.manual_seed(5)
    llm = _StubLLM(16, 21, 40)
    a = RWKV7LM(16, 16, 20, llm, lsm_weight=0.1, length_normalized_loss=nl)
    b = RWKV7LM(16, 16, 20, llm, lsm_weight=0.1, length_normalized_loss=nl, fused_loss=True)
    b.load_state_dict(a.state_dict())
    assert a.fused_loss is False and b.fused_loss is True
    batch = L.cosy_collate([[3, 4, 5, 6], [7, 8]], [[10, 11, 12, 13, 14, 15, 16], [19, 1, 2]], pad_to_max_length=False)
    ra, rb = a(batch), b(batch)
    assert abs(ra["loss"].item() - rb["loss"].item()) <= 1e-6 * abs(ra["loss"].item()) and ra["acc"].item() == rb["acc"].item()
    pa = [p for p in a.parameters()]
    ga = torch.autograd.grad(ra["loss"], pa, allow_unused=True)
    gb = torch.autograd.grad(rb["loss"], [p for p in b.parameters()], allow_unused=True)
    for x, y in zip(ga, gb):
        assert (x is None) == (y is None)
        if x is not None:
            assert (x - y).abs().max().item() <= 1e-6 * max(x.abs().max().item(), 1e-30)
    # an llm without .model / .lm_head keeps today's code
    c = RWKV7LM(16, 16, 20, _Opaque(llm), lsm_weight=0.1, length_normalized_loss=nl, fused_loss=True)
    c.load_state_dict(a.state_dict(), strict=False)
    assert c(batch)["loss"].item() == ra["loss"].item()


class _Opaque(nn.Module):
    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def get_input_embeddings(self):
        return self.inner.text

    def forward(self, inputs_embeds=None, attention_mask=None):
        return self.inner(inputs_embeds=inputs_embeds, attention_mask=attention_mask)


def test_config_switch_defaults_off_and_round_trips():
    small = dict(hidden_size=128, num_hidden_layers=2, vocab_size=200, speech_token_size=50)
    assert RWKV7CosyConfig(**small).fused_loss is False
    assert RWKV7CosyConfig(**small).to_dict()["fused_loss"] is False
    cfg = RWKV7CosyConfig(fused_loss=True, **small)
    back = RWKV7CosyConfig.from_dict(cfg.to_dict())
    assert back.fused_loss is True and back.to_dict() == cfg.to_dict() and "fused_loss" not in back.extra


def test_entry_point_rejects_bad_arguments_before_any_launch(hip_lib):
    one = ctypes.c_void_p(16)   # never dereferenced: the checks fire first
    fn = hip_lib.rwkv7_kl_acc_fwd_bwd_bf16
    assert "rwkv7_kl_acc_fwd_bwd_bf16" in __import__("rwkvtts_amd")._lib.exported_symbols()

    def call(rows=4, V=11, ld=11, logits=one, dlogits=one, labels=one, s=0.1, loss=one, correct=one):
        return fn(ctypes.c_long(rows), ctypes.c_int(V), ctypes.c_long(ld), logits, dlogits, labels, ctypes.c_long(-1), ctypes.c_float(s),
                  ctypes.c_float(1.0), loss, correct, None)

    for name in ("logits", "dlogits", "labels", "loss", "correct"):
        assert call(**{name: None}) == -1, name
    assert call(rows=0) == -1 and call(rows=-3) == -1
    assert call(V=1, ld=1) == -1 and call(V=0) == -1
    assert call(V=11, ld=10) == -1
    for s in (-0.1, 1.0, 1.5, float("nan")):
        assert call(s=s) == -1, s
