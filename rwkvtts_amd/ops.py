"""Host-side mirror of the reference's WKV7 operator interface, backed by librwkv7_hip.so.

Same names, argument order and error behaviour as the reference so that its call sites work unchanged:

    torch.ops.wind_backstepping.forward / .backward      model/llm/cuda/wkv7_op.cpp:21-29
    torch.ops.rwkv7_state_fwd_fp16.forward               model/llm/cuda/rwkv7_state_fwd_fp16.cpp:8-14
    torch.ops.wkv7s.forward                              model/llm/cuda/wkv7s_op.cpp:9-15
    WindBackstepping, RUN_CUDA_RWKV7g                    model/llm/rwkv_s2s_single_ffn.py:15-40
    WKV_7 / RWKV7_OP, WKV_7_batch / RWKV7_BATCH_OP       model/llm/rwkv_asr_cuda_whisper.py:50-81

The ops are registered for the CUDA dispatch key (which is HIP on ROCm) only -- exactly like the
reference (wkv7_op.cpp:26-29) -- so CPU tensors raise NotImplementedError instead of silently
running somewhere else.  PyTorch is plumbing here: it owns the device memory and the stream.

Extension over the reference: fp32 tensors are accepted everywhere bf16 is (routed to the *_f32
C entry points); that is what the fp32 logit-parity tests use.
"""
import torch

from . import _lib, fused

HEAD_SIZE = 64
CHUNK_LEN = 16
DTYPE = torch.bfloat16


# bench.py sets this to a dict to time individual launches with HIP events recorded on the launch stream
# (torch's current stream IS the stream handed to the C ABI): name -> [(start_event, end_event), ...]
KERNEL_TIMERS = None


class _timed:
    def __init__(self, name, ref):
        self.name, self.on = name, KERNEL_TIMERS is not None
        if self.on:
            st = torch.cuda.current_stream(ref.device)
            self.s, self.e, self.st = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), st

    def __enter__(self):
        if self.on:
            self.s.record(self.st)

    def __exit__(self, *a):
        if self.on:
            self.e.record(self.st)
            KERNEL_TIMERS.setdefault(self.name, []).append((self.s, self.e))


def _call(timer, name, ref, *args):
    """_lib.call as the launch that KERNEL_TIMERS lists under `timer`."""
    with _timed(timer, ref):
        _lib.call(name, ref, *args)


def _sfx(ts, what):
    dt = ts[0].dtype
    if dt not in (torch.bfloat16, torch.float32):
        raise TypeError(f"{what}: tensors must be bfloat16 (reference) or float32, got {dt}")
    for t in ts:
        if t.dtype != dt:
            raise TypeError(f"{what}: mixed dtypes {dt} / {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{what}: tensors must be contiguous (rwkv_s2s_single_ffn.py:21)")
        if not t.is_cuda:
            raise NotImplementedError(f"{what}: HIP device tensors only (no CPU path)")
    return "bf16" if dt == torch.bfloat16 else "f32"


# ------------------------------------------------------------------------------------------------
# raw ops (caller allocates everything, ops mutate in place and return None)
# ------------------------------------------------------------------------------------------------
# torch.ops.wind_backstepping.{forward,backward} launch the chunked (MFMA) pair whenever they can -- bf16 tensors, T % 32 == 0 --
# with `s` (a private forward -> backward scratch in the reference, rwkv_s2s_single_ffn.py:22-35) as an opaque arena of the same
# size (include/rwkv7_hip.h, rwkv7_wkv_fwd_fast_bf16); otherwise (fp32, T % 32 == 16) the scalar kernels, whose `s` holds the
# reference's checkpoints.  False = always the scalar kernels (A/B).
REFERENCE_OP_FAST = True


def reference_op_is_fast(dtype, T):
    """Which kernels torch.ops.wind_backstepping.* launch for tensors of this dtype and length."""
    return bool(REFERENCE_OP_FAST and dtype == torch.bfloat16 and T % 32 == 0)


def wkv7_forward_scalar(w, q, k, v, z, a, y, s, sa):
    """The scalar forward kernel (rwkv7_wkv_fwd_*): s = the reference's checkpoints (fp32 [B,H,T/16,64,64], transposed), which
    wkv7_backward_scalar / wkv7_backward_split consume."""
    B, T, H, C = w.shape
    sfx = _sfx([w, q, k, v, z, a, y], "wind_backstepping.forward")
    assert C == HEAD_SIZE and s.dtype == torch.float32 and sa.dtype == torch.float32
    _call("wkv7_fwd", "rwkv7_wkv_fwd_" + sfx, w, B, T, H, w, q, k, v, z, a, y, s, sa)


def wkv7_backward_scalar(w, q, k, v, z, a, dy, s, sa, dw, dq, dk, dv, dz, da):
    B, T, H, C = w.shape
    sfx = _sfx([w, q, k, v, z, a, dy, dw, dq, dk, dv, dz, da], "wind_backstepping.backward")
    _call("wkv7_bwd", "rwkv7_wkv_bwd_" + sfx, w, B, T, H, w, q, k, v, z, a, dy, s, sa, dw, dq, dk, dv, dz, da)


def _check_arena(w, s, what):
    B, T, H, C = w.shape
    if s.dtype != torch.float32 or not s.is_contiguous() or s.numel() < B * H * (T // CHUNK_LEN) * C * C:
        raise ValueError(f"{what}: s must be the reference's contiguous fp32 [B,H,T/16,64,64] scratch (rwkv_s2s_single_ffn.py:23)")


def _wb_forward(w, q, k, v, z, a, y, s, sa):
    B, T, H, C = w.shape
    if not reference_op_is_fast(w.dtype, T):
        return wkv7_forward_scalar(w, q, k, v, z, a, y, s, sa)
    _sfx([w, q, k, v, z, a, y], "wind_backstepping.forward")
    assert C == HEAD_SIZE and sa.dtype == torch.float32
    _check_arena(w, s, "wind_backstepping.forward")
    _call("wkv7c_op_fwd", "rwkv7_wkv_fwd_fast_bf16", w, B, T, H, w, q, k, v, z, a, y, s, sa)


def _wb_backward(w, q, k, v, z, a, dy, s, sa, dw, dq, dk, dv, dz, da):
    B, T, H, C = w.shape
    if not reference_op_is_fast(w.dtype, T):
        return wkv7_backward_scalar(w, q, k, v, z, a, dy, s, sa, dw, dq, dk, dv, dz, da)
    _sfx([w, q, k, v, z, a, dy, dw, dq, dk, dv, dz, da], "wind_backstepping.backward")
    _check_arena(w, s, "wind_backstepping.backward")
    _call("wkv7c_op_bwd", "rwkv7_wkv_bwd_fast_bf16", w, B, T, H, w, q, k, v, z, a, dy, s, sa, dw, dq, dk, dv, dz, da)


def wkv7_backward_split(w, q, k, v, z, a, dy, s, sa, wide=None):
    """WKV7 backward with each head split over two workgroups (rwkv7_wkv_bwd_split_*: all 256 CUs busy at B*H=128); s, sa as
    written by wkv7_forward_scalar.
    Returns (dw2, dq2, dk2, dv, dz2, da2): the *2 tensors are [2, B,T,H,64] partial column sums whose sum over dim 0
    is the gradient wind_backstepping.backward returns; dv is complete.
    wide (bf16 only, measurements/tests): 0 / 1 selects the 256- / 512-thread shape explicitly (rwkv7_wkv_bwd_split_variant_bf16)."""
    B, T, H, C = w.shape
    sfx = _sfx([w, q, k, v, z, a, dy], "wkv7_backward_split")
    dw2, dq2, dk2, dz2, da2 = [torch.empty((2,) + tuple(w.shape), dtype=w.dtype, device=w.device) for _ in range(5)]
    dv = torch.empty_like(v)
    pair = _lib.ptr_array   # a [2, ...] tensor as the two device pointers the entry takes
    args = (B, T, H, w, q, k, v, z, a, dy, s, sa, pair(dw2), pair(dq2), pair(dk2), dv, pair(dz2), pair(da2))
    if wide is None:
        _call("wkv7_bwd", "rwkv7_wkv_bwd_split_" + sfx, w, *args)
    else:
        _call("wkv7_bwd", "rwkv7_wkv_bwd_split_variant_" + sfx, w, *args, int(wide))
    return dw2, dq2, dk2, dv, dz2, da2


def _state_forward(B, T, C, H, state, r, w, k, v, a, b, y):
    sfx = _sfx([r, w, k, v, a, b, y], "rwkv7_state_fwd.forward")
    if state.dtype != torch.float32 or not state.is_contiguous():
        raise TypeError("rwkv7_state_fwd.forward: state must be contiguous float32 [B,H,64,64]")
    _lib.call("rwkv7_wkv_state_fwd_" + sfx, r, int(B), int(T), int(C), int(H), state, r, w, k, v, a, b, y)


def _wkv7s_forward(B, T, C, H, state, r, w, k, v, a, b, y):
    assert B == 1, "wkv7s is the B=1 operator (wkv7s.cu:62)"
    _state_forward(B, T, C, H, state, r, w, k, v, a, b, y)


_registered = []


def _register():
    """Define the three reference op namespaces and bind them to the HIP library."""
    if _registered:
        return
    defs = [
        ("wind_backstepping",
         [("forward(Tensor w, Tensor q, Tensor k, Tensor v, Tensor z, Tensor a, Tensor(a!) y, Tensor(b!) s, "
           "Tensor(c!) sa) -> ()", "forward", _wb_forward),
          ("backward(Tensor w, Tensor q, Tensor k, Tensor v, Tensor z, Tensor a, Tensor dy, Tensor s, Tensor sa, "
           "Tensor(a!) dw, Tensor(b!) dq, Tensor(c!) dk, Tensor(d!) dv, Tensor(e!) dz, Tensor(f!) da) -> ()",
           "backward", _wb_backward)]),
        ("rwkv7_state_fwd_fp16",
         [("forward(int B, int T, int C, int H, Tensor(a!) state, Tensor r, Tensor w, Tensor k, Tensor v, "
           "Tensor a, Tensor b, Tensor(b!) y) -> ()", "forward", _state_forward)]),
        ("wkv7s",
         [("forward(int B, int T, int C, int H, Tensor(a!) state, Tensor r, Tensor w, Tensor k, Tensor v, "
           "Tensor a, Tensor b, Tensor(b!) y) -> ()", "forward", _wkv7s_forward)]),
    ]
    for ns, ops in defs:
        lib = torch.library.Library(ns, "DEF")
        for schema, name, fn in ops:
            lib.define(schema)
            lib.impl(name, fn, "CUDA")
        _registered.append(lib)  # keep alive


_register()


# ------------------------------------------------------------------------------------------------
# autograd wrapper and call-site helpers (reference names)
# ------------------------------------------------------------------------------------------------
class WindBackstepping(torch.autograd.Function):
    """rwkv_s2s_single_ffn.py:15-35.  Argument order (w,q,k,v,z,b) with z == a, b == b."""

    @staticmethod
    def forward(ctx, w, q, k, v, z, b):
        B, T, H, C = w.shape
        assert T % CHUNK_LEN == 0, f"T={T} must be a multiple of {CHUNK_LEN}"
        assert all(i.dtype == w.dtype for i in [w, q, k, v, z, b])
        assert all(i.is_contiguous() for i in [w, q, k, v, z, b])
        y = torch.empty_like(v)
        s = torch.empty(B, H, T // CHUNK_LEN, C, C, dtype=torch.float32, device=w.device)
        sa = torch.empty(B, T, H, C, dtype=torch.float32, device=w.device)
        torch.ops.wind_backstepping.forward(w, q, k, v, z, b, y, s, sa)
        ctx.save_for_backward(w, q, k, v, z, b, s, sa)
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        w, q, k, v, z, b, s, sa = ctx.saved_tensors
        assert dy.dtype == w.dtype
        dw, dq, dk, dv, dz, db = [torch.empty_like(x) for x in [w, q, k, v, z, b]]
        torch.ops.wind_backstepping.backward(w, q, k, v, z, b, dy, s, sa, dw, dq, dk, dv, dz, db)
        return dw, dq, dk, dv, dz, db


def RUN_CUDA_RWKV7g(q, w, k, v, a, b):
    """rwkv_s2s_single_ffn.py:37-40: [B,T,H*64] in, [B,T,H*64] out, differentiable."""
    B, T, HC = q.shape
    q, w, k, v, a, b = [i.view(B, T, HC // HEAD_SIZE, HEAD_SIZE) for i in [q, w, k, v, a, b]]
    return WindBackstepping.apply(w, q, k, v, a, b).view(B, T, HC)


def wkv7_forward_nograd(q, w, k, v, a, b):
    """Inference-only zero-state scan: no checkpoints, no sa (s = sa = NULL in the C ABI)."""
    B, T, HC = q.shape
    H = HC // HEAD_SIZE
    sfx = _sfx([w, q, k, v, a, b], "wkv7_forward_nograd")
    if T % CHUNK_LEN != 0:
        raise ValueError("T must be a multiple of 16; use the state-carrying op for ragged lengths")
    y = torch.empty_like(v)
    _lib.call("rwkv7_wkv_fwd_" + sfx, w, B, T, H, w, q, k, v, a, b, y, None, None)
    return y


def RWKV7_OP(state, r, w, k, v, a, b):
    """rwkv_s2s_single_ffn.py:45-59 (torch.ops.wkv7s): r..b [T,C], state [H,64,64] updated in place."""
    with torch.no_grad():
        T, C = r.shape
        H = C // HEAD_SIZE
        y = torch.empty((T, C), device=k.device, dtype=r.dtype)
        torch.ops.wkv7s.forward(1, T, C, H, state, r, w, k, v, a, b, y)
        return y


def RWKV7_BATCH_OP(state, r, w, k, v, a, b):
    """rwkv_asr_cuda_whisper.py:67-81: r..b [B,T,C], state [B,H,64,64] fp32 updated in place."""
    with torch.no_grad():
        B, T, C = r.shape
        H = C // HEAD_SIZE
        y = torch.empty((B, T, C), device=k.device, dtype=r.dtype)
        torch.ops.rwkv7_state_fwd_fp16.forward(B, T, C, H, state, r, w, k, v, a, b, y)
        return y


# ------------------------------------------------------------------------------------------------
# chunked (MFMA) WKV7: the training fast path (csrc/chunk_common.h, wkv7_chunk_fwd.hip, wkv7_chunk_bwd.hip)
# ------------------------------------------------------------------------------------------------
CHUNK_T = 32
Q15_REC = 64 * 64 + 2 * 256   # int16 units of one 64x64 state checkpoint: 4096 mantissas + 256 fp32 scales
_Q15_IDX = None


def q15_decode(rec):
    """[..., Q15_REC] int16 records (csrc/chunk_common.h: what the chunked forward saves as hs and the adjoint-state kernel as
    e_vk; mantissas in MFMA accumulator order mant[vh][kt][lane][16], one scale per lane) -> fp32 [..., 64 (value), 64 (key)]."""
    global _Q15_IDX
    if _Q15_IDX is None:
        v = torch.arange(64).view(64, 1).expand(64, 64)
        k = torch.arange(64).view(1, 64).expand(64, 64)
        slot = ((v >> 5) * 2 + (k >> 5)) * 64 + (v & 31) + 32 * ((k >> 2) & 1)
        r = (k & 3) + 4 * ((k >> 3) & 3)
        _Q15_IDX = ((slot * 16 + r).reshape(-1), slot.reshape(-1))
    mi, si = (t.to(rec.device) for t in _Q15_IDX)
    q = rec[..., :4096].float().index_select(-1, mi)
    sc = rec[..., 4096:].contiguous().view(torch.float32).index_select(-1, si)
    return (q * sc).reshape(*rec.shape[:-1], 64, 64)


def wkv7_chunk_prep(w, a, b):
    """(I - A_ab)^-1 of every 32-step chunk: fp32 [B,H,T/32,32,32].  w,a,b: [B,T,H,64]."""
    B, T, H, C = w.shape
    sfx = _sfx([w, a, b], "wkv7_chunk_prep")
    tinv = torch.empty(B, H, T // CHUNK_T, CHUNK_T, CHUNK_T, dtype=torch.float32, device=w.device)
    _call("wkv7c_prep", "rwkv7_wkv_chunk_prep_" + sfx, w, B, T, H, w, a, b, tinv)
    return tinv


def _nseq(seq_off):
    """The sequence count of a packed row's seq_off (0 for plain rows, seq_off = None)."""
    if seq_off is None:
        return 0
    if seq_off.dtype != torch.int32 or seq_off.dim() != 1 or seq_off.numel() < 2 or not seq_off.is_contiguous() or not seq_off.is_cuda:
        raise TypeError("seq_off must be a contiguous int32 [nseq + 1] device tensor")
    return seq_off.numel() - 1


def _chunk_fwd(w, q, k, v, a, b, save, seq_off, nseq, h0=None):
    """prep + the sequential chunked forward on [B,T,H,64] rows: (y, tinv, sa, hs, hT), sa = hs = None unless save.
    h0 (fp32 [B or nseq,H,64,64]): start from it on the carried-state entry, which also returns the end states hT (else None)."""
    B, T, H, C = w.shape
    sfx = _sfx([w, q, k, v, a, b], "wkv7_chunk_forward")
    if T % CHUNK_T != 0:
        raise ValueError(f"chunked WKV7 needs T % {CHUNK_T} == 0, got T={T}")
    tinv = wkv7_chunk_prep(w, a, b)
    y = torch.empty_like(v)
    sa = torch.empty(B, T, H, C, dtype=torch.float32, device=w.device) if save else None
    hs = torch.empty(B, H, T // CHUNK_T, Q15_REC, dtype=torch.int16, device=w.device) if save else None
    hT = None if h0 is None else torch.empty(nseq if seq_off is not None else B, H, C, C, dtype=torch.float32, device=w.device)
    args = (B, T, H, w, q, k, v, a, b, tinv, y, sa, hs, seq_off, nseq)
    if h0 is None:
        _call("wkv7c_fwd", "rwkv7_wkv_chunk_fwd_seq_" + sfx, w, *args)
    else:
        _call("wkv7c_fwd_state", "rwkv7_wkv_chunk_fwd_state_seq_bf16", w, *args, h0, hT)
    return y, tinv, sa, hs, hT


def wkv7_chunk_forward(w, q, k, v, a, b, save=True, seq_off=None):
    """Chunked forward.  Returns y, and (tinv, sa, hs) when save (what the chunked backward consumes; hs = the state at the
    start of every chunk as q15 records, see q15_decode).
    seq_off: packed rows -- int32 [nseq + 1] device tensor of cumulative 32-step chunk counts over the [B][T/32] chunk
    space; sequence s owns chunks seq_off[s] .. seq_off[s+1] - 1 and starts from the zero state."""
    y, tinv, sa, hs, _ = _chunk_fwd(w, q, k, v, a, b, save, seq_off, _nseq(seq_off))
    return (y, tinv, sa, hs) if save else y


def _bseq(w, q, a, b, dy, tinv, seq_off, nseq, want_z, state=None):
    """The adjoint-state recurrence on [B,T,H,64] rows: (e_vk, z), z (fp32 [B,T,H,64]) only with want_z.
    state = (dhT, dh0), fp32 [B or nseq,H,64,64], each may be None: the carried-state entry (dh0 is written)."""
    B, T, H, C = w.shape
    if w.dtype != torch.bfloat16:
        raise TypeError("the chunked backward is bf16 only")
    if T % CHUNK_T != 0:
        raise ValueError(f"chunked WKV7 needs T % {CHUNK_T} == 0, got T={T}")
    e_vk = torch.empty(B, H, T // CHUNK_T, Q15_REC, dtype=torch.int16, device=w.device)
    # stateless packed rows may leave positions behind the last sequence untouched: zeros there (the gradient kernel reads every
    # chunk).  The carried-state layouts give every chunk of the row to a sequence.
    zeroed = seq_off is not None and state is None
    z = (torch.zeros if zeroed else torch.empty)(B, T, H, C, dtype=torch.float32, device=w.device) if want_z else None
    args = (B, T, H, w, q, a, b, dy, tinv, e_vk, z, seq_off, nseq)
    if state is None:
        _call("wkv7c_bseq", "rwkv7_wkv_chunk_bseq_bf16", w, *args)
    else:
        _call("wkv7c_bseq_state", "rwkv7_wkv_chunk_bseq_state_seq_bf16", w, *args, *state)
    return e_vk, z


def wkv7_chunk_bwd_seq(w, q, a, b, dy, tinv, seq_off=None, want_z=False):
    """The adjoint-state recurrence of the chunked backward as ONE sequential kernel (csrc/wkv7_chunk_bseq.hip): the factored
    form E_c = E' + A~^T Z + Q~^T dY, Z = (T^T B^) E' + (T^T A_qb^T) dY -- M_c^T / N'_c are not materialised.  Returns e_vk
    (e_vk[b,h,c] = E_{c+1} as q15 records); with want_z also Z (fp32 [B,T,H,64],
    Z_t = dL/du_t) as (e_vk, z)."""
    e_vk, z = _bseq(w, q, a, b, dy, tinv, seq_off, _nseq(seq_off), want_z)
    return (e_vk, z) if want_z else e_vk


def _chunk_bwd(w, q, k, v, a, b, dy, hs, sa, tinv, seq_off, nseq, state=None):
    """bseq (which also writes Z = dL/du) + the per-chunk gradients from Z on [B,T,H,64] rows: [dw, dq, dk, dv, da, db].
    state: as _bseq."""
    B, T, H, C = w.shape
    e_vk, z = _bseq(w, q, a, b, dy, tinv, seq_off, nseq, True, state)
    grads = [torch.empty_like(w) for _ in range(6)]
    _call("wkv7c_bwd_out", "rwkv7_wkv_chunk_bwd_out_z_bf16", w, B, T, H, w, q, k, v, a, b, dy, hs, sa, z, e_vk, *grads)
    return grads


def wkv7_chunk_backward(w, q, k, v, a, b, dy, hs, sa, tinv, seq_off=None):
    """Chunked (MFMA) WKV7 backward, bf16: same gradients as torch.ops.wind_backstepping.backward, T % 32 == 0, from what
    wkv7_chunk_forward saved (hs, sa, tinv).  Two launches: the adjoint-state recurrence (csrc/wkv7_chunk_bseq.hip, which also
    writes Z = dL/du) and the per-chunk gradients from Z (csrc/wkv7_chunk_bwd10.hip, two matrix phases).
    Returns (dw, dq, dk, dv, da, db)."""
    if hs.dtype != torch.int16 or hs.shape[-1] != Q15_REC or sa.dtype != torch.float32 or tinv.dtype != torch.float32:
        raise TypeError("wkv7_chunk_backward takes hs (q15 records), sa and tinv (fp32) as saved by wkv7_chunk_forward")
    return tuple(_chunk_bwd(w, q, k, v, a, b, dy, hs, sa, tinv, seq_off, _nseq(seq_off)))


def debug_mma32(X, Y):
    """GPU unit-test hook: D = X Y^T for X,Y fp32 [32,64] through the bf16-split MFMA primitive; returns (D, DT)."""
    D = torch.empty(32, 32, device=X.device)
    DT = torch.empty(32, 32, device=X.device)
    _lib.call("rwkv7_debug_mma32", X, X.contiguous(), Y.contiguous(), D, DT)
    return D, DT


# ------------------------------------------------------------------------------------------------
# chunked WKV7 through a carried state: training across segments / tuning an initial state
# ------------------------------------------------------------------------------------------------
# Identity steps: w = W_PAD makes exp(w) underflow to 0 in the kernels' fast_exp (v_exp_f32 of -1.4e4), so the step's decay
# exp(-exp(w)) is exactly 1, its log -exp(w) exactly 0; with q = k = v = a = b = 0 the step adds nothing, reads nothing and
# outputs y = 0: S' = S bit for bit.  Every use of w in the chunked kernels goes through -fast_exp(w) (decay logs, their prefix
# sums, g = exp(prefix), 1/g = exp(-prefix), g_{t-1} = exp(prefix - log)) and the decay gradient dw = dlog * log: no 0 * inf.
W_PAD = -1.0e4


def _pad_rows(x, front, tail, fill):
    """[B,T,C] -> contiguous [B, front + T + tail, C] with `fill` in the added rows (x itself when nothing is added)."""
    if front == 0 and tail == 0:
        return x.contiguous()
    B, T, C = x.shape
    out = x.new_full((B, front + T + tail, C), fill)
    out[:, front:front + T] = x
    return out


def _unpad_rows(x, front, tail):
    """[B, front + T + tail, C] -> contiguous [B, T, C] (x itself when nothing was added)."""
    if front == 0 and tail == 0:
        return x
    return x[:, front:x.shape[1] - tail].contiguous()


class _WkvStateChunked(torch.autograd.Function):
    """y, hT = the scans from carried states of a chunk-aligned row [R, front + T + tail, H*64] on the chunked kernels,
    differentiable in h0 and r..b.  r..b come in as [R, T, H*64]: the Function adds `front` / `tail` identity rows (w = W_PAD, the
    rest 0) and drops them again from y and from the input gradients.  seq_off (int32 [nseq + 1] device tensor) / nseq: packed
    rows with one state per sequence, h0 / hT [nseq,H,64,64]; None / 0: one state per row, [R,H,64,64]."""

    @staticmethod
    def forward(ctx, h0, r, w, k, v, a, b, seq_off, nseq, front, tail):
        R, T, HC = r.shape
        H = HC // HEAD_SIZE
        Tp = front + T + tail
        train = any(ctx.needs_input_grad)
        ins = [_pad_rows(x, front, tail, f) for x, f in ((w, W_PAD), (r, 0.0), (k, 0.0), (v, 0.0), (a, 0.0), (b, 0.0))]
        w4, q4, k4, v4, a4, b4 = [x.view(R, Tp, H, HEAD_SIZE) for x in ins]
        y, tinv, sa, hs, hT = _chunk_fwd(w4, q4, k4, v4, a4, b4, train, seq_off, nseq, h0=h0.contiguous())
        if train:
            ctx.save_for_backward(w4, q4, k4, v4, a4, b4, tinv, sa, hs, seq_off)
            ctx.nseq, ctx.n_states, ctx.front, ctx.tail = nseq, hT.shape[0], front, tail
        ctx.set_materialize_grads(False)
        return _unpad_rows(y.view(R, Tp, HC), front, tail), hT

    @staticmethod
    def backward(ctx, dy, dhT):
        w4, q4, k4, v4, a4, b4, tinv, sa, hs, seq_off = ctx.saved_tensors
        R, Tp, H, C = w4.shape
        front, tail = ctx.front, ctx.tail
        dy4 = torch.zeros_like(v4) if dy is None else _pad_rows(dy.to(w4.dtype), front, tail, 0.0).view(R, Tp, H, C)
        dhT = None if dhT is None else dhT.to(torch.float32).contiguous()
        dh0 = torch.empty(ctx.n_states, H, C, C, dtype=torch.float32, device=w4.device) if ctx.needs_input_grad[0] else None
        grads = _chunk_bwd(w4, q4, k4, v4, a4, b4, dy4, hs, sa, tinv, seq_off, ctx.nseq, state=(dhT, dh0))
        dw, dq, dk, dv, da, db = [_unpad_rows(g.view(R, Tp, H * C), front, tail) for g in grads]
        return dh0, dq, dw, dk, dv, da, db, None, None, None, None


def wkv7_state_chunked(h0, r, w, k, v, a, b):
    """The WKV7 scan from a carried state on the chunked (MFMA) kernels, differentiable in all seven inputs: what a stateful
    training forward (truncated BPTT over segments, initial-state tuning) needs.  RWKV7_BATCH_OP computes the same forward
    without a tape (scalar kernel, state updated in place).
      h0: fp32 [B,H,64,64] (row = value, column = key: LayerState.att_kv's layout)
      r, w, k, v, a, b: bf16 [B,T,H*64] as RWKV7_BATCH_OP takes them (w: the pre-activation, decay = exp(-exp(w))); any T >= 1
    Returns (y bf16 [B,T,H*64], hT fp32 [B,H,64,64]); h0 is not modified.  bf16 only (the chunked backward is)."""
    B, T, HC = r.shape
    for t in (w, k, v, a, b):
        if t.shape != r.shape:
            raise ValueError(f"wkv7_state_chunked: r..b must share one shape [B,T,H*64], got {tuple(r.shape)} / {tuple(t.shape)}")
    if HC % HEAD_SIZE != 0 or T < 1:
        raise ValueError(f"wkv7_state_chunked: need T >= 1 and H*64 channels, got {tuple(r.shape)}")
    if any(t.dtype != torch.bfloat16 for t in (r, w, k, v, a, b)):
        raise TypeError("wkv7_state_chunked: r..b must be bfloat16 (the chunked backward is bf16 only)")
    if not all(t.is_cuda for t in (h0, r, w, k, v, a, b)):
        raise NotImplementedError("wkv7_state_chunked: HIP device tensors only (no CPU path)")
    if h0.dtype != torch.float32 or tuple(h0.shape) != (B, HC // HEAD_SIZE, HEAD_SIZE, HEAD_SIZE):
        raise TypeError(f"wkv7_state_chunked: h0 must be float32 [B,H,64,64] = {(B, HC // HEAD_SIZE, 64, 64)}, got "
                        f"{h0.dtype} {tuple(h0.shape)}")
    # T % 32 != 0: identity steps in FRONT (the state reaches the first real step unchanged).  Training (any input requires grad:
    # the Function's needs_input_grad) frames the row with one whole identity chunk at EACH end: the per-chunk gradient kernel
    # (csrc/wkv7_chunk_bwd10.hip, unchanged) treats a row as starting from the zero state and ending with no future -- a workgroup
    # hands the end state of one chunk on as the start state of the next and zeroes it across a row boundary, and the last chunk's
    # rowsum(E * H_C) decay term is dropped.  With the pad chunks every real chunk is an inner one: its start state is the
    # checkpoint of the state after the leading pad (= h0) and its future the adjoint behind the trailing pad (= dhT), both passed
    # through the identity chunks bit for bit.
    train = any(t.requires_grad for t in (h0, r, w, k, v, a, b))
    front = (-T) % CHUNK_T + (CHUNK_T if train else 0)
    return _WkvStateChunked.apply(h0, r, w, k, v, a, b, None, 0, front, CHUNK_T if train else 0)


# ------------------------------------------------------------------------------------------------
# the same on packed rows (fla's cu_seqlens): one carried state per sequence
# ------------------------------------------------------------------------------------------------
class PackedStateLayout:
    """Where a packed row's sequences sit in the chunk-aligned row the stateful packed scan runs on (packed_state_layout).
      t_al     rows of the aligned row (a multiple of CHUNK_T)
      dest     int32 [sum(lens)]: aligned row of every packed position (positions counted from cu_seqlens[0])
      seq_off  int32 [N + 1]: sequence i owns chunks seq_off[i] .. seq_off[i + 1] - 1 (empty range for an empty sequence)
      first, last  int32 [N]: aligned rows of each sequence's first and last token (-1 for an empty sequence)"""
    __slots__ = ("t_al", "dest", "seq_off", "first", "last")

    def __init__(self, t_al, dest, seq_off, first, last):
        self.t_al, self.dest, self.seq_off, self.first, self.last = t_al, dest, seq_off, first, last


def packed_state_layout(lens, train, align=None):
    """The chunk-aligned row for sequences of `lens` tokens that carry a state in and out (host ints; pure, no device work):
      - every sequence ENDS on a chunk boundary and has at least one identity row in front of it (32 - n % 32 of them, 1 .. 32):
        its first chunk is padded in front, so the scan reaches its first token with the carried state untouched, and the model's
        token shift sees a masked predecessor there (RWKV7Model._forward_packed_state adds the carried one);
      - train: one whole identity chunk follows every sequence, inside its chunk range -- the per-chunk gradient kernel reads the
        end state of a sequence's last real chunk from the next chunk's start record, which must be this sequence's own state --
        and one leads the ROW (in the first non-empty sequence's range): that kernel's workgroups run across the head boundaries of
        the [H][chunk] space and start each head's first chunk from zero (include/rwkv7_hip.h, rwkv7_wkv_chunk_fwd_state_seq_bf16;
        the sequences after the first need no leading one);
      - align(rows) -> rows rounds the row up (RWKV7Model: _row_align); the rows it adds are identity chunks of the last non-empty
        sequence, so every chunk of the row belongs to a sequence and none is left to uninitialised memory.
    An empty sequence owns no chunk (first = last = -1).  With no tokens at all t_al = 0."""
    C = CHUNK_T
    lens = [int(n) for n in lens]
    if any(n < 0 for n in lens):
        raise ValueError(f"packed_state_layout: negative sequence length in {lens}")
    dest = torch.empty(sum(lens), dtype=torch.int32)
    seq_off, first, last = [0], [], []
    t, pos, last_ne = (C if train and sum(lens) > 0 else 0), 0, -1
    for i, n in enumerate(lens):
        if n == 0:
            first.append(-1)
            last.append(-1)
            seq_off.append(seq_off[-1])
            continue
        else:
            lo = t + (C - n % C)
            dest[pos:pos + n] = torch.arange(lo, lo + n, dtype=torch.int32)
            first.append(lo)
            last.append(lo + n - 1)
            t = lo + n + (C if train else 0)
            pos += n
            last_ne = i
            seq_off.append(t // C)
    t_al = align(t) if (align is not None and t > 0) else t
    if t_al > t:
        for i in range(last_ne + 1, len(seq_off)):
            seq_off[i] = t_al // C
    return PackedStateLayout(t_al, dest, torch.tensor(seq_off, dtype=torch.int32), torch.tensor(first, dtype=torch.int32),
                             torch.tensor(last, dtype=torch.int32))


def wkv7_state_chunked_seq(h0, r, w, k, v, a, b, seq_off, nseq):
    """The per-sequence scans of a packed row that is ALREADY laid out (packed_state_layout): r..b bf16 [1, T_al, H*64] with
    identity steps (w = W_PAD, the rest 0) at every row outside a sequence, seq_off int32 [nseq + 1] on the device, h0 fp32
    [nseq,H,64,64].  Returns (y [1, T_al, H*64], hT [nseq,H,64,64]); the gradients at the identity rows are not meaningful."""
    return _WkvStateChunked.apply(h0, r, w, k, v, a, b, seq_off, nseq, 0, 0)


class RowMap:
    """A packed row [1, total, D] and the chunk-aligned row [1, t_al, D] its sequences are laid out on, from dest (int32 [total]:
    the aligned row of every packed position, -1 for a position that belongs to no sequence; on the host or the device):
      dest, src_of  int32 [total] / [t_al] on `device`: src_of = the packed position every aligned row holds, -1 for a masked row
      keep          bool [1, t_al, 1]: the aligned rows that hold a token
    Both maps are injective, so both re-layouts and both of their gradients are row gathers (fused.gather_rows)."""

    def __init__(self, dest, t_al, device):
        j = torch.arange(dest.numel(), dtype=torch.int32, device=dest.device)
        src_of = torch.full((t_al + 1,), -1, dtype=torch.int32, device=dest.device)   # slot t_al takes the unowned positions
        src_of = src_of.scatter(0, torch.where(dest >= 0, dest, torch.full_like(dest, t_al)).long(), j)[:t_al]
        self.dest, self.src_of = dest.to(device, non_blocking=True), src_of.to(device, non_blocking=True)
        self.keep = (self.src_of >= 0).view(1, -1, 1)

    def to_aligned(self, x):
        """[1, total, D] -> [1, t_al, D], zeros in the masked rows."""
        return fused.gather_rows(x[0], self.src_of, self.dest).unsqueeze(0)

    def to_packed(self, y):
        """[1, t_al, D] -> [1, total, D], zeros at the positions of no sequence."""
        return fused.gather_rows(y[0], self.dest, self.src_of).unsqueeze(0)


def wkv7_state_chunked_varlen(h0, r, w, k, v, a, b, cu_seqlens):
    """wkv7_state_chunked on a packed row (fla chunk_rwkv7's initial_state / output_final_state with cu_seqlens): sequence i occupies
    [cu_seqlens[i], cu_seqlens[i+1]) of r..b (bf16 [1, total, H*64]) and starts from h0[i] (fp32 [N,H,64,64]).  Returns
    (y [1, total, H*64], hT [N,H,64,64]); differentiable in all seven inputs.  An empty sequence passes its state through
    (hT[i] = h0[i], dh0[i] = dhT[i]); positions outside [cu_seqlens[0], cu_seqlens[-1]) give y = 0.  The op lays the sequences out
    on its own chunk-aligned row (packed_state_layout, identity steps in every pad row, framed for training when any input requires
    grad) and drops the pad rows' gradients.  A device cu_seqlens costs one host read-back."""
    _, total, HC = r.shape
    for t in (w, k, v, a, b):
        if t.shape != r.shape:
            raise ValueError(f"wkv7_state_chunked_varlen: r..b must share one shape [1,total,H*64], got {tuple(r.shape)} / {tuple(t.shape)}")
    if r.shape[0] != 1 or HC % HEAD_SIZE != 0:
        raise ValueError(f"wkv7_state_chunked_varlen: need a packed [1, total, H*64] row, got {tuple(r.shape)}")
    if any(t.dtype != torch.bfloat16 for t in (r, w, k, v, a, b)):
        raise TypeError("wkv7_state_chunked_varlen: r..b must be bfloat16 (the chunked backward is bf16 only)")
    if not all(t.is_cuda for t in (h0, r, w, k, v, a, b)):
        raise NotImplementedError("wkv7_state_chunked_varlen: HIP device tensors only (no CPU path)")
    cu = [int(c) for c in cu_seqlens.tolist()]
    N, H = len(cu) - 1, HC // HEAD_SIZE
    if N < 1 or any(b_ < a_ for a_, b_ in zip(cu[:-1], cu[1:])) or cu[0] < 0 or cu[-1] > total:
        raise ValueError(f"wkv7_state_chunked_varlen: cu_seqlens must be non-decreasing within [0, {total}], got {cu}")
    if h0.dtype != torch.float32 or tuple(h0.shape) != (N, H, HEAD_SIZE, HEAD_SIZE):
        raise TypeError(f"wkv7_state_chunked_varlen: h0 must be float32 [N,H,64,64] = {(N, H, 64, 64)}, got {h0.dtype} {tuple(h0.shape)}")
    train = torch.is_grad_enabled() and any(t.requires_grad for t in (h0, r, w, k, v, a, b))
    lay = packed_state_layout([b_ - a_ for a_, b_ in zip(cu[:-1], cu[1:])], train)
    if lay.t_al == 0:
        return r.new_zeros(r.shape), h0.clone()
    dest = torch.full((total,), -1, dtype=torch.int32)
    dest[cu[0]:cu[-1]] = lay.dest
    rows = RowMap(dest, lay.t_al, r.device)
    r_al, w_al, k_al, v_al, a_al, b_al = [rows.to_aligned(x) for x in (r, w, k, v, a, b)]
    w_al = torch.where(rows.keep, w_al, W_PAD)   # identity steps in every pad row
    y_al, hT = wkv7_state_chunked_seq(h0, r_al, w_al, k_al, v_al, a_al, b_al, lay.seq_off.to(r.device, non_blocking=True), N)
    return rows.to_packed(y_al), hT
