"""Training through the recurrent state, host side: the two stateful C entry points (declared, exported, argument checks that
fire before any launch), Cache.zeros(..., differentiable=True) / Cache.detach(), and the identity-step algebra the op pads with."""
import ctypes

import pytest
import torch

from oracle import rwkv7_ref as R
from rwkvtts_amd import _lib, ops
from rwkvtts_amd.backbone import Cache, RWKV7Config
from rwkvtts_amd.synthetic import make_wkv_inputs

NEW = ("rwkv7_wkv_chunk_fwd_state_bf16", "rwkv7_wkv_chunk_bseq_state_bf16")


def test_state_entry_points_declared_and_exported(hip_lib):
    declared = _lib.exported_symbols()
    for n in NEW:
        assert n in declared, f"{n} not declared in include/rwkv7_hip.h"
        assert hasattr(hip_lib, n), f"{n} not exported"


def test_state_entry_points_reject_bad_arguments_without_launching(hip_lib):
    one = ctypes.c_void_p(16)   # never dereferenced: the checks fire first
    fwd, bseq = hip_lib.rwkv7_wkv_chunk_fwd_state_bf16, hip_lib.rwkv7_wkv_chunk_bseq_state_bf16
    # T % 32 != 0 -> RWKV7_ECHUNK
    assert fwd(1, 48, 1, *([one] * 10), None, None, None) == -2
    assert bseq(1, 33, 1, *([one] * 8), None, None, None, None) == -2
    # null operand -> RWKV7_EINVAL
    assert fwd(1, 32, 1, None, *([one] * 9), None, None, None, None, None) == -1
    assert bseq(1, 32, 1, *([one] * 5), None, one, None, None, None, None) == -1      # tinv
    assert bseq(1, 32, 1, *([one] * 6), None, None, None, None, None) == -1           # e_vk
    # sa without hs -> RWKV7_EINVAL ; non-positive sizes -> RWKV7_EINVAL
    assert fwd(1, 32, 1, *([one] * 8), one, None, None, None, None) == -1
    assert fwd(0, 32, 1, *([one] * 8), None, None, None, None, None) == -1
    assert bseq(1, 32, 0, *([one] * 7), None, None, None, None) == -1


def _cfg():
    return RWKV7Config(hidden_size=128, num_hidden_layers=3, vocab_size=16, decay_low_rank_dim=32, a_low_rank_dim=32,
                       v_low_rank_dim=16, gate_low_rank_dim=32)


def test_cache_zeros_differentiable_flag_and_detach():
    cfg = _cfg()
    assert Cache().differentiable is False
    assert Cache.zeros(cfg, 2, "cpu", torch.bfloat16).differentiable is False
    c = Cache.zeros(cfg, 2, "cpu", torch.bfloat16, differentiable=True)
    assert c.differentiable is True and len(c) == 3
    s = c[1]
    assert s.att_x_prev.shape == (2, 128) and s.att_x_prev.dtype == torch.bfloat16
    assert s.att_kv.shape == (2, 2, 64, 64) and s.att_kv.dtype == torch.float32
    # a state with a graph behind it: detach() cuts it, keeps values, seen_tokens and the flag, and shares no storage
    leaf = torch.randn(2, 2, 64, 64, requires_grad=True)
    s.att_kv = leaf * 2.0
    s.ffn_x_prev = torch.randn(2, 128).bfloat16().requires_grad_()
    c.seen_tokens = 40
    d = c.detach()
    assert isinstance(d, Cache) and d is not c and d.seen_tokens == 40 and d.differentiable is True and len(d) == 3
    for a, b in zip(c.states, d.states):
        for ta, tb in ((a.att_x_prev, b.att_x_prev), (a.att_kv, b.att_kv), (a.ffn_x_prev, b.ffn_x_prev)):
            assert not tb.requires_grad and tb.grad_fn is None
            assert torch.equal(ta.detach(), tb) and ta.data_ptr() != tb.data_ptr()
    assert Cache.zeros(cfg, 1, "cpu", torch.float32).detach().differentiable is False
    # the original keeps its graph
    assert c[1].att_kv.grad_fn is not None


def test_decode_step_refuses_a_differentiable_cache():
    from rwkvtts_amd.decode import DecodeStep
    with pytest.raises(ValueError, match="differentiable"):
        DecodeStep(None, None, Cache.zeros(_cfg(), 1, "cpu", torch.bfloat16, differentiable=True))


def test_identity_pad_steps_leave_output_and_state_unchanged_fp64():
    """What ops.wkv7_state_chunked prepends for T % 32 != 0: steps with w = W_PAD (decay exp(-exp(w)) == 1) and q = k = v = a = b = 0.
    On the fp64 oracle scan from a non-zero state they leave y and the state exactly unchanged and output zeros."""
    B, T, H, P = 2, 17, 2, 15
    w, q, k, v, a, b = [t.double() for t in make_wkv_inputs(B, T, H, seed=3, dtype=torch.float32)]
    h0 = torch.randn(B, H, 64, 64, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    assert torch.exp(-torch.exp(torch.tensor(ops.W_PAD, dtype=torch.bfloat16).double())).item() == 1.0
    y, S = R.wkv7_scan(q, w, k, v, a, b, state=h0.clone())
    pad = lambda x, fill: torch.cat([torch.full((B, P, H, 64), fill, dtype=x.dtype), x], 1)
    yp, Sp = R.wkv7_scan(pad(q, 0.0), pad(w, ops.W_PAD), pad(k, 0.0), pad(v, 0.0), pad(a, 0.0), pad(b, 0.0), state=h0.clone())
    assert torch.equal(yp[:, P:], y) and torch.equal(Sp, S)
    assert torch.equal(yp[:, :P], torch.zeros_like(yp[:, :P]))
    # the same steps appended behind the last real one: the final state passes through unchanged
    tail = lambda x, fill: torch.cat([x, torch.full((B, P, H, 64), fill, dtype=x.dtype)], 1)
    yt, St = R.wkv7_scan(tail(q, 0.0), tail(w, ops.W_PAD), tail(k, 0.0), tail(v, 0.0), tail(a, 0.0), tail(b, 0.0), state=h0.clone())
    assert torch.equal(yt[:, :T], y) and torch.equal(St, S)
