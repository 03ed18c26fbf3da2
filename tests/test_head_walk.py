"""CPU: what the three gradient nodes of rwkvtts_amd.losses share -- the chunk walk (_chunk_plan), the gradient accumulator
(_HeadGrads) and the torch-route row gradient (_grad_rows_torch).

The reference is the arithmetic the nodes had when each wrote its own loop, restated here (parent_loop, parent_scaled,
parent_ce_rows, parent_seq_rows); every comparison is torch.equal: the shared code issues the same library calls on the same
tensors, so nothing may differ.
The fp32-GEMM flag of the accumulator (the Cosy head: torch.mm(..., out_dtype=torch.float32)) has no CPU implementation in torch;
it is covered by the GPU twin alone (test_head_walk_gpu.py, which runs accumulator_case on the device for both flag values)."""
import pytest
import torch

from rwkvtts_amd import losses

N, D, V, VP = 200, 32, 37, 64
NEEDS = [(True, True, True), (True, False, False), (False, True, False)]


# ---- the walk ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hip", [False, True])
@pytest.mark.parametrize("overlap_last", [False, True])
@pytest.mark.parametrize("align", [1, 64])
def test_walk_covers_every_row_exactly_once(align, overlap_last, hip):
    for n in (1, 15, 64, 65, 127, 128, 129, 200):
        for chunk in (1, 5, 64, 128, 1000):
            per_call, walk = losses._chunk_plan(n, V, 2, hip, chunk, align, overlap_last)
            covered = []
            for s, rows, skip in walk:
                assert 0 <= s and s + rows <= n and 0 <= skip < rows, (n, chunk, s, rows, skip)
                assert skip == 0 or (s, rows, skip) == walk[-1], "only an overlapping last chunk skips rows"
                covered += range(s + skip, s + rows)
            assert covered == list(range(n)), (n, chunk)
            if hip and overlap_last:
                rounded = -(-chunk // align) * align
                assert per_call == min(rounded, n) and all(rows == per_call for _, rows, _ in walk), (n, chunk)
            if align == 1 and not overlap_last:
                assert [s for s, _, _ in walk] == list(range(0, n, min(chunk, n))), (n, chunk)


# ---- the accumulator ---------------------------------------------------------------------------------------------------------------
def parent_loop(walk, pd, h, w, bias, need, fp32, p32=None):
    """dh, dw, db as the three nodes' own loops formed them (done - s was the skip of an overlapping last chunk)."""
    dh = torch.empty_like(h, dtype=torch.float32 if fp32 else h.dtype) if need[0] else None
    dw = torch.zeros_like(w, dtype=torch.float32) if need[1] else None
    db = torch.zeros_like(bias, dtype=torch.float32) if (bias is not None and need[2]) else None
    done = 0
    for s, rows, _ in walk:
        pdc, hc = pd[done:s + rows], h[done:s + rows]
        if need[0]:
            dh[done:s + rows] = torch.mm(pdc, w, out_dtype=torch.float32) if fp32 else pdc @ w
        if need[1]:
            dw += torch.mm(pdc.t(), hc, out_dtype=torch.float32) if fp32 else (pdc.t() @ hc).float()
        if db is not None:
            db += pdc.sum(0, dtype=torch.float32) if p32 is None else p32[done:s + rows].sum(0)
        done = s + rows
    return dh, dw, db


def parent_scaled(dh, dw, db, g, hdtype, wdtype):
    return ((dh.float() * g).to(hdtype) if dh is not None else None, (dw * g).to(wdtype) if dw is not None else None,
            (db * g).to(wdtype) if db is not None else None)


def _same(got, want, what):
    assert len(got) == len(want)
    for name, a, b in zip(("dh", "dw", "db"), got, want):
        assert (a is None) == (b is None), (what, name)
        if a is not None:
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (what, name)


def accumulator_case(device, fp32, need, with_bias, padded=False, from_fp32=False):
    """One accumulation of N rows two ways (chunks of 128 whose last one overlaps by 56 rows; chunks of 64 without overlap) against
    parent_loop, then the scaled triple against parent_scaled.  padded: the weight zero-padded to [VP, D], dw sliced [:V], as the
    padded cross-entropy head does.  from_fp32: the torch routes, which hand the fp32 rows over for db."""
    g = torch.Generator().manual_seed(7)
    cols = VP if padded else V
    p32 = torch.zeros(N, cols)
    p32[:, :V] = torch.randn(N, V, generator=g)
    w = torch.zeros(cols, D)
    w[:V] = torch.randn(V, D, generator=g) * 0.1
    h = torch.randn(N, D, generator=g).bfloat16().to(device)
    bias = (torch.randn(cols, generator=g) * 0.1).bfloat16().to(device) if with_bias else None
    p32, pd, w = p32.to(device), p32.bfloat16().to(device), w.bfloat16().to(device)
    p32 = p32 if from_fp32 else None
    overlapping = losses._chunk_plan(N, V, 2, True, 128, 64, True)[1]
    assert overlapping == [(0, 128, 0), (72, 128, 56)]
    for walk in (overlapping, losses._chunk_plan(N, V, 2, True, 64)[1]):
        grads = losses._HeadGrads(need, h, w, bias, fp32=fp32)
        for s, rows, skip in walk:
            lo, hi = s + skip, s + rows
            grads.add(pd[lo:hi], h[lo:hi], lo, hi, None if p32 is None else p32[lo:hi])
        want = parent_loop(walk, pd, h, w, bias, need, fp32, p32)
        _same((grads.dh, grads.dw, grads.db), want, ("sums", len(walk)))
        if padded and need[1]:
            assert torch.equal(grads.dw[:V], want[1][:V]) and not grads.dw[V:].any()
        scale = torch.tensor(0.37, device=device)
        _same(losses._HeadGrads.scaled(grads.dh, grads.dw, grads.db, scale, torch.bfloat16, torch.bfloat16),
              parent_scaled(*want, scale, torch.bfloat16, torch.bfloat16), ("scaled", len(walk)))


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("need", NEEDS)
def test_accumulator_equals_the_nodes_own_loops(need, with_bias):
    accumulator_case("cpu", False, need, with_bias)


def test_accumulator_on_a_zero_padded_weight():
    accumulator_case("cpu", False, (True, True, True), False, padded=True)


def test_accumulator_takes_db_from_the_fp32_rows_of_a_torch_route():
    accumulator_case("cpu", False, (True, True, True), True, from_fp32=True)


# ---- the torch-route row gradient --------------------------------------------------------------------------------------------------
def parent_ce_rows(logits, lab, ignore_index, label_smoothing, inv):
    vmask = lab != ignore_index
    safe = lab.clamp(min=0)
    tgt = logits.gather(1, safe.unsqueeze(1)).squeeze(1)
    p = torch.softmax(logits, dim=-1)
    if label_smoothing > 0:
        p = p - label_smoothing / logits.shape[-1]
        p.scatter_add_(1, safe.unsqueeze(1), torch.full_like(tgt, -(1 - label_smoothing)).unsqueeze(1))
    else:
        p.scatter_add_(1, safe.unsqueeze(1), torch.full_like(tgt, -1.0).unsqueeze(1))
    return p * (vmask.unsqueeze(1) * inv)


def parent_seq_rows(x, lb, ignore_index, scales):
    p = torch.softmax(x, dim=1)
    p.scatter_add_(1, lb.clamp(min=0).unsqueeze(1), torch.full_like(p[:, :1], -1.0))
    return p * (scales * (lb != ignore_index)).unsqueeze(1)


def _rows():
    g = torch.Generator().manual_seed(11)
    logits = torch.randn(9, 11, generator=g) * 3
    lab = torch.randint(0, 11, (9,), generator=g)
    lab[[1, 6]] = -100
    scales = torch.randn(9, generator=g)
    scales[2], scales[3] = 0.0, -1.5
    return logits, lab, scales


@pytest.mark.parametrize("inv", [1 / 7, -0.25])
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
def test_grad_rows_torch_equals_the_cross_entropy_nodes_expression(smoothing, inv):
    logits, lab, _ = _rows()
    inv = torch.tensor(inv)
    got = losses._grad_rows_torch(logits, lab, smoothing, (lab != -100) * inv)
    assert got.dtype == torch.float32 and torch.equal(got, parent_ce_rows(logits, lab, -100, smoothing, inv))
    assert not got[[1, 6]].any() and got[0].any()


def test_grad_rows_torch_equals_the_sequence_nodes_expression():
    logits, lab, scales = _rows()
    got = losses._grad_rows_torch(logits, lab, 0.0, scales * (lab != -100))
    assert got.dtype == torch.float32 and torch.equal(got, parent_seq_rows(logits, lab, -100, scales))
    assert not got[[1, 2, 6]].any() and got[3].any()
