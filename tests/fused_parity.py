"""Comparison helpers shared by tests/test_fused_gpu.py and tests/test_fused_rows_gpu.py (the bars are derived in the header of
tests/test_fused_gpu.py: fp32 kernels relative to max|ref|; bf16 kernels within 1 bf16 ulp, 2^-7 relative with an absolute floor)."""
import torch

DEV = "cuda:0"


def _cmp(got, want, tol, what):
    got = got.detach().float().cpu()
    want = want.detach().float()
    err = (got - want).abs().max().item()
    ref = want.abs().max().item()
    assert err <= tol * max(ref, 1e-3), f"{what}: max|d|={err:.3e} max|ref|={ref:.3e} tol={tol}"


def _cmp_bf16(got, want, what, ulps=1.0):
    got = got.detach().float().cpu()
    want = want.detach().float()
    floor = want.abs().mean().item() * 0.25 + 1e-6
    tol = ulps * 2.0 ** -7 * torch.clamp(want.abs(), min=floor)
    bad = (got - want).abs() > tol
    assert not bad.any(), f"{what}: {bad.sum().item()}/{bad.numel()} beyond {ulps} bf16 ulp"


def _mk(shape, g, scale=1.0, dtype=torch.float32):
    return (torch.randn(*shape, generator=g) * scale).to(dtype).float()  # values exactly representable in dtype


def _run_both(fn_hip, fn_ref, inputs, dtype, grad_names, fwd_tol, bwd_tol):
    """inputs: dict name -> fp32 CPU tensor (already rounded to dtype) or non-tensor."""
    ref_in = {k: (v.clone().requires_grad_(k in grad_names) if torch.is_tensor(v) else v) for k, v in inputs.items()}
    hip_in = {k: (v.to(DEV, dtype).requires_grad_(k in grad_names) if torch.is_tensor(v) else v)
              for k, v in inputs.items()}
    out_r = fn_ref(**ref_in)
    out_h = fn_hip(**hip_in)
    out_r = out_r if isinstance(out_r, (tuple, list)) else (out_r,)
    out_h = out_h if isinstance(out_h, (tuple, list)) else (out_h,)
    g = torch.Generator().manual_seed(77)
    douts = [_mk(o.shape, g, 1.0, dtype) for o in out_r]
    for i, (a, b) in enumerate(zip(out_h, out_r)):
        if dtype == torch.bfloat16:
            _cmp_bf16(a, b, f"out[{i}]")
        else:
            _cmp(a, b, fwd_tol, f"out[{i}]")
    torch.autograd.backward(list(out_r), douts)
    torch.autograd.backward(list(out_h), [d.to(DEV, dtype) for d in douts])
    for n in grad_names:
        gr, gh = ref_in[n].grad, hip_in[n].grad
        assert gh is not None, n
        if dtype == torch.bfloat16:
            # gradients of broadcast parameters are sums over B*T rows rounded once to bf16
            _cmp(gh, gr, 2.0 ** -6, f"d{n}")
        else:
            _cmp(gh, gr, bwd_tol, f"d{n}")
