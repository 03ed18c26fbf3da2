"""GPU (-m gpu): the z-loss / max-logit regularisers on the HIP route -- rwkv7_ce_reg_fwd_bwd_bf16 alone,
losses.fused_linear_cross_entropy(z_loss, max_logit, stats) on the padded head, the Spark / XY models and DataParallelTrainer.

The kernel is held against an fp64 restatement from the SAME bf16 logits.  No tolerance is fixed in advance for its gradient and its
lse: each case first measures the EXISTING kernel (rwkv7_ce_fwd_bwd_ld_bf16) against fp64 on the same logits -- per valid row the
largest element error relative to the row's largest gradient magnitude, the maximum over the rows: E -- and the regularised kernel must
stay within 2 E by the same measure (the margin is for the one more multiply, by k = 1 + 2 z lse, in front of the one bf16 rounding).
An ABSOLUTE error d of lse is a RELATIVE error d of every softmax value of the row, so lse_rows is held to |lse_rows - lse| <= 2 E too.
max_rows is exact, and so is the place of the max-logit bump.
Both errors are, in the end, the one bf16 rounding of the row's largest elements: at most 2^-8 of the value, and anywhere below that by
the luck of the value.  The maximum over the 4 valid rows of a 5-row launch is therefore noise, and so is the ratio of two such maxima
(the first run of this file, with one draw of logits per case, gave at V = 7, rows = 5: regularised 3.519e-03 against plain 1.426e-03
-- each EXACTLY the error of the correctly rounded fp64 value, the best any kernel can write).  So a case draws its logits as often
as it takes to see 64 rows (13 draws of 5 rows, one of 64), both kernels on the same draws, and E and the regularised error are the
maxima over all of them; the bar stays 2 E.  Every comparison prints `PARITY <case> <observable> <error> <yardstick>`;
the record of one run is profiles/logit_reg_parity.txt."""
import pytest
import torch
import torch.nn.functional as F

from rwkvtts_amd import _lib, losses, trainer
from rwkvtts_amd.xy_llm import RWKV7XYConfig, RWKV7XYLM
from test_preference_gpu import KW, SENTINEL, _bits, _pairs, _rel_l2, _spark

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IGN = -100
NAME = "rwkv7_ce_reg_fwd_bwd_bf16"
PLAIN = "rwkv7_ce_fwd_bwd_ld_bf16"
Z, C, LS, SCALE = 1e-2, 5e-2, 0.1, 0.37
# V, ld, rows: singles only; odd unaligned rows (head and tail singles); padded aligned rows; the XY head
CASES = [(7, 8, 5), (7, 8, 64), (8193, 8193, 5), (8193, 8193, 64), (8193, 8448, 5), (8193, 8448, 64), (66661, 66664, 5), (66661, 66664, 8)]


def _inputs(V, ld, rows, draw=0):
    """bf16 logits [rows, ld] (columns V .. a sentinel) and labels: row 1 ignored, row 3 with label 0; rows 0 and 7 with their maximum
    TWICE; the maximum of row 2 at index 0 (the head singles of an unaligned row), of row 5 inside a 16-byte piece, of row 6 in the tail
    singles, of row 4 at V - 1; every other row as drawn -- 3 sigma bf16 values, where ties among the largest are common."""
    g = torch.Generator().manual_seed(V + ld + rows + 1000 * draw)
    x = torch.zeros(rows, ld, dtype=torch.bfloat16)
    x[:, :V] = (torch.randn(rows, V, generator=g) * 3).bfloat16()
    _bits(x)[:, V:] = SENTINEL
    lab = torch.randint(0, V, (rows,), generator=g)
    places = {0: [1, V // 2], 2: [0], 4: [V - 1], 5: [min(20, V - 1)], 6: [max(V - 3, 0)], 7: [min(3, V - 1), V - 2]}
    for r, cols in places.items():
        if r < rows:
            x[r, cols] = 24.0 + r   # exact in bf16, above every drawn value
    lab[1] = IGN
    lab[3] = 0
    if rows > 40:
        lab[[23, 40]] = IGN
    return x.to(DEV), lab.to(DEV), places


def _launch(name, x, lab, V, ls, *reg):
    """The entry on a copy of x: (gradient buffer, loss_rows[, lse_rows, max_rows])."""
    rows, ld = x.shape
    out = x.clone()
    loss = torch.full((rows,), -7.0, device=DEV)
    if name == PLAIN:
        _lib.call(name, out, rows, V, ld, out, lab, IGN, SCALE, loss, ls)
        return out, loss
    lse, mx = torch.full((rows,), -7.0, device=DEV), torch.full((rows,), -7.0, device=DEV)
    _lib.call(name, out, rows, V, ld, out, lab, IGN, SCALE, loss, ls, *reg, lse, mx)
    return out, loss, lse, mx


def _fp64(x, lab, V, ls, z, c):
    """The header's formulas in fp64 from the bf16 logits: (gradient [rows, V], lse, m, a), zero on ignored rows."""
    x64 = x[:, :V].double()
    valid = lab != IGN
    lse = torch.logsumexp(x64, 1)
    m = x64.max(1).values
    a = (x64 == m[:, None]).int().argmax(1)   # the first of equal values: the lowest index
    t = torch.full_like(x64, ls / V)
    t.scatter_add_(1, lab.clamp(min=0)[:, None], torch.full_like(t[:, :1], 1 - ls))
    d = torch.exp(x64 - lse[:, None]) * (1 + 2 * z * lse)[:, None] - t
    d.scatter_add_(1, a[:, None], (c * m)[:, None])
    return d * SCALE * valid[:, None], lse * valid, m * valid, a


def _row_err(got, want):
    """max over the rows of (largest element error / largest |reference| of the row); rows whose reference is zero are skipped."""
    top = want.abs().max(1).values
    err = (got.double() - want).abs().max(1).values
    keep = top > 0
    return (err[keep] / top[keep]).max().item()


# ---- 1: off is the plain kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,ld,rows", CASES)
@pytest.mark.parametrize("ls", [0.0, LS])
def test_coefficients_zero_give_the_plain_kernels_bits(hip_lib, V, ld, rows, ls):
    x, lab, _ = _inputs(V, ld, rows)
    want, want_loss = _launch(PLAIN, x, lab, V, ls)
    got, loss, lse, mx = _launch(NAME, x, lab, V, ls, 0.0, 0.0)
    assert torch.equal(_bits(got), _bits(want)) and torch.equal(loss, want_loss)
    assert not torch.equal(_bits(got), _bits(x))
    x2, loss2 = x.clone(), torch.empty_like(loss)
    _lib.call(NAME, x2, rows, V, ld, x2, lab, IGN, SCALE, loss2, ls, 0.0, 0.0, None, None)
    assert torch.equal(_bits(x2), _bits(want)) and torch.equal(loss2, want_loss), "lse_rows / max_rows may be NULL"


# ---- 2: parity ---------------------------------------------------------------------------------------------------------------------
def _parity(V, ld, rows):
    """Both kernels and the fp64 restatement on every draw of the case; the tensors of draw 0, the errors over all draws."""
    first = None
    for draw in range(max(1, -(-64 // rows))):
        x, lab, places = _inputs(V, ld, rows, draw)
        valid = lab != IGN
        plain, plain_loss = _launch(PLAIN, x, lab, V, LS)
        got, loss, lse, mx = _launch(NAME, x, lab, V, LS, Z, C)
        d0, lse64, m64, a64 = _fp64(x, lab, V, LS, 0.0, 0.0)
        d1 = _fp64(x, lab, V, LS, Z, C)[0]
        E, err = _row_err(plain[:, :V], d0), _row_err(got[:, :V], d1)
        lse_err = (lse.double() - lse64).abs().max().item()
        assert torch.equal(loss, plain_loss), "loss_rows stays the plain cross-entropy, bit for bit"
        assert torch.equal(mx.double(), m64), "max_rows is exact"
        if first is None:
            first = dict(x=x, lab=lab, valid=valid, places=places, plain_loss=plain_loss, got=got, loss=loss, lse=lse, mx=mx, m64=m64,
                         a64=a64, E=E, err=err, lse_err=lse_err)
        else:
            first.update(E=max(first["E"], E), err=max(first["err"], err), lse_err=max(first["lse_err"], lse_err))
    return first


@pytest.mark.parametrize("V,ld,rows", CASES)
def test_kernel_against_the_fp64_restatement(hip_lib, V, ld, rows):
    p = _parity(V, ld, rows)
    case = f"kernel rows={rows} V={V} ld={ld}"
    print(f"PARITY {case} grad {p['err']:.3e} plain {p['E']:.3e}")
    print(f"PARITY {case} lse {p['lse_err']:.3e} plain-grad {p['E']:.3e}")
    valid, got, x = p["valid"], p["got"], p["x"]
    assert torch.equal(p["loss"], p["plain_loss"]), "loss_rows stays the plain cross-entropy, bit for bit"
    assert torch.equal(p["mx"].double(), p["m64"]), "max_rows is exact"
    assert (p["lse"][~valid] == 0).all() and (p["mx"][~valid] == 0).all() and (p["loss"][~valid] == 0).all()
    assert (got[~valid][:, :V] == 0).all(), "ignored rows stay all-zero"
    assert torch.equal(_bits(got)[:, V:], _bits(x)[:, V:]), "columns V .. ld - 1 are not written"
    # the bump of c m sc sits on the LOWEST index among the maxima and nowhere else: against the same launch with c = 0 only element
    # a moves, by c m sc up to the two bf16 roundings (each at most 2^-8 of its value); a bump above 2^-6 is far above them
    no_bump = _launch(NAME, x, p["lab"], V, LS, Z, 0.0)[0]
    moved = (got[:, :V].double() - no_bump[:, :V].double()).abs()
    want_bump = (C * p["m64"] * SCALE).abs()
    rows_v = valid.nonzero()[:, 0]
    a_v = p["a64"][rows_v]
    clear = want_bump[rows_v] > 2 ** -6
    assert clear.sum().item() >= min(4, len(rows_v)) and torch.equal(moved[rows_v].argmax(1)[clear], a_v[clear])
    roundings = 2 ** -8 * (got[rows_v, a_v].double().abs() + no_bump[rows_v, a_v].double().abs())
    assert ((moved[rows_v, a_v] - want_bump[rows_v]).abs() <= roundings + 1e-6).all()
    moved[rows_v, a_v] = 0
    assert moved.max().item() == 0.0, "no other element sees the max-logit coefficient"
    for r, cols in p["places"].items():
        if r < rows and bool(valid[r]):
            assert p["a64"][r].item() == min(cols), (r, cols)
    assert p["err"] <= 2 * p["E"], (p["err"], p["E"])
    assert p["lse_err"] <= 2 * p["E"], (p["lse_err"], p["E"])


@pytest.fixture(scope="module")
def yardstick(hip_lib):
    """E and the lse error of the padded Spark shape, measured once: the bar of the trainer's statistics."""
    p = _parity(8193, 8448, 64)
    return p["E"]


# ---- 3: independence ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,ld", [(7, 8), (8193, 8193), (8193, 8448), (66661, 66664)])
def test_a_rows_outputs_do_not_depend_on_its_neighbours_or_its_place(hip_lib, V, ld):
    """How a row is split into singles and 16-byte pieces follows from its ADDRESS modulo 16 bytes (and the sums from the split), so a
    row is moved by multiples of 8 rows, which keep that for every ld: the launch of 13 rows against launches that start 8 rows later
    (the row changes its wave, its workgroup and its neighbours), against a chunked walk, and against other rows around it."""
    rows = 13
    x, lab, _ = _inputs(V, ld, rows)
    full = _launch(NAME, x, lab, V, LS, Z, C)

    def same(part, lo, hi, at=0):
        for a, b in zip(part, full):
            assert torch.equal(_bits(a[at:at + hi - lo]) if a.dtype == torch.bfloat16 else a[at:at + hi - lo],
                               _bits(b[lo:hi]) if b.dtype == torch.bfloat16 else b[lo:hi])

    same(_launch(NAME, x[8:], lab[8:], V, LS, Z, C), 8, 13)          # rows 8 .. 12 as rows 0 .. 4 of their own launch
    same(_launch(NAME, x[:8], lab[:8], V, LS, Z, C), 0, 8)           # the chunk split 8 + 5
    other = x.clone()
    other[:8, :V] = (other[:8, :V].float() * -0.5).bfloat16()        # other neighbours, other labels around rows 8 .. 12
    lab2 = lab.clone()
    lab2[:8] = IGN
    same(tuple(t[8:] for t in _launch(NAME, other, lab2, V, LS, Z, C)), 8, 13)


# ---- 4: the padded route -------------------------------------------------------------------------------------------------------------
def _head_case(N, D, V, seed, bias=False):
    g = torch.Generator().manual_seed(seed)
    h = (torch.randn(N, D, generator=g) * 0.5).to(DEV, torch.bfloat16)
    w = (torch.randn(V, D, generator=g) * D ** -0.5).to(DEV, torch.bfloat16)
    b = (torch.randn(V, generator=g) * 0.1).to(DEV, torch.bfloat16) if bias else None
    lab = torch.randint(0, V, (N,), generator=g).to(DEV)
    lab[::7] = IGN
    lab[1] = V - 1
    return h, w, b, lab


def _both_routes(monkeypatch, fn, reg=True):
    """fn() on the HIP route and on the torch route (the A/B switch RWKV7_HIP_CE=0).  reg: the call has a regulariser on."""
    out = []
    for hip in (True, False):
        monkeypatch.setattr(losses, "HIP_CE", hip)
        hits = losses.LOGIT_REG_HITS[0]
        out.append(fn())
        assert (losses.LOGIT_REG_HITS[0] > hits) == (hip and reg)
    return out


def test_padded_route_against_the_torch_route(hip_lib, monkeypatch):
    """hidden [256, 1024], V = 8193.  Bars: the loss within 1e-4 (test_heads_gpu.py's bar for a head's training loss), dh and dW within
    4e-3 relative L2 (the bar of the padded head's own test for two routes that each round d loss / d logits to bf16 once)."""
    h, w, _, lab = _head_case(256, 1024, 8193, 5)

    def run():
        hi, wi = h.clone().requires_grad_(), w.clone().requires_grad_()
        stats = torch.zeros(4, device=DEV)
        loss = losses.fused_linear_cross_entropy(hi, lab, wi, None, IGN, z_loss=Z, max_logit=C, stats=stats)
        loss.backward()
        return loss.item(), hi.grad, wi.grad, stats

    pads = losses.PADDED_HEAD_HITS[0]
    (l1, dh1, dw1, s1), (l0, dh0, dw0, s0) = _both_routes(monkeypatch, run)
    assert losses.PADDED_HEAD_HITS[0] == pads + 1, "the HIP call took the padded route"
    print(f"PARITY padded loss {abs(l1 - l0):.3e} dh {_rel_l2(dh1, dh0):.3e} dW {_rel_l2(dw1, dw0):.3e}")
    assert abs(l1 - l0) < 1e-4
    assert _rel_l2(dh1, dh0) < 4e-3 and _rel_l2(dw1, dw0) < 4e-3
    assert s1[0].item() == s0[0].item() == (lab != IGN).sum().item()
    assert ((s1 - s0).abs() <= 1e-4 * s0.abs()).all()
    # the regularisers are in the gradient: the plain head's differs by far more than the two routes do
    hi = h.clone().requires_grad_()
    losses.fused_linear_cross_entropy(hi, lab, w, None, IGN).backward()
    assert _rel_l2(hi.grad, dh1) > 10 * 4e-3


# ---- 5: models and trainer ----------------------------------------------------------------------------------------------------------
def _no_dropout(m):
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m


def _head_grads(m):
    return {k: p.grad.clone() for k, p in m.named_parameters() if ("head" in k) and p.grad is not None}


def test_spark_model_forward_backward_against_the_torch_route(hip_lib, monkeypatch):
    m = _no_dropout(_spark().train())
    m.config.z_loss, m.config.max_logit = Z, C
    batch = _pairs(m, 4, 64, seed=31)

    def run():
        m.zero_grad(set_to_none=True)
        loss = m(**batch).loss
        loss.backward()
        return loss.item(), _head_grads(m)

    (l1, g1), (l0, g0) = _both_routes(monkeypatch, run)
    print(f"PARITY spark model loss {abs(l1 - l0):.3e} " + " ".join(f"{k} {_rel_l2(g1[k], g0[k]):.3e}" for k in g0))
    assert abs(l1 - l0) < 1e-4 and g0 and all(_rel_l2(g1[k], g0[k]) < 4e-3 for k in g0)


def _head_grads_fp64(h, lab, W, b, hip, ls, z, c):
    """(dW, db) of one head in fp64 from the logits its ROUTE forms out of the recorded hidden states: the HIP route F.linear's bf16
    logits (the bias inside the GEMM's epilogue), the torch route the bf16 product in fp32 plus the fp32 bias.  The objective is the
    mean over the valid rows of CE (label smoothing ls) + z lse^2 + 0.5 c m^2, its gradient by the logits as _fp64 states it."""
    x = F.linear(h, W, b) if hip else (h @ W.t()).float() + b.float()
    d = _fp64(x, lab, x.shape[1], ls, z, c)[0] / SCALE / (lab != IGN).sum()
    return d.t() @ h.double(), d.sum(0)


def test_xy_model_forward_backward_against_the_torch_route(hip_lib, monkeypatch):
    """Bias and label smoothing on; the coefficients reach each of the four channels' heads.  The loss of the two routes agrees within
    1e-4 (test_heads_gpu.py's bar for a head's training loss).
    The head gradients are NOT compared route against route: with a bias the routes see different logits (one bf16 rounding of
    product + bias on the HIP route; the rounded product plus an fp32 bias on the torch route), and the max-logit bump is discontinuous
    in them.  Measured on this model and batch: the arg-max differs in 7 of 1015 valid rows of channel 0, and that alone moves the
    fp64 gradient of the objective by 3.5e-3 (dW) and 2.8e-3 (db) relative L2 between the two sets of logits, against 6e-5 with c = 0
    -- as much as all roundings of a route together (a first form of this test compared the routes and saw 4.3e-3 .. 4.9e-3 on
    channel 0 against 1.7e-3 .. 3.0e-3 with the coefficients off).  So each route's dW and db are held against fp64 from ITS OWN
    logits (the heads' inputs are recorded on the way in), and, as for the kernel, the bar is measured, not fixed: twice the error
    of the same route with both coefficients 0 against fp64 by the same measure (relative L2), per tensor."""
    small = dict(hidden_size=128, num_hidden_layers=2, decay_low_rank_dim=32, a_low_rank_dim=32, v_low_rank_dim=16, gate_low_rank_dim=32)
    cfg = RWKV7XYConfig(vocab_size=120, speech_vocab_size=16, num_channels=4, text_shift_size=100, lsm_weight=LS, z_loss=Z, max_logit=C,
                        **small)
    m = RWKV7XYLM(cfg).init_weights(seed=2)
    with torch.no_grad():
        for head in m.heads:
            head.bias.normal_(0, 0.1)
    m = m.to(DEV).to(torch.bfloat16).train()
    g = torch.Generator().manual_seed(8)
    B, T = 8, 128
    ids = torch.cat([torch.randint(0, 119, (B, T, 1), generator=g), torch.randint(0, 15, (B, T, 3), generator=g)], 2).to(DEV)
    labels = torch.cat([torch.randint(0, 120, (B, T, 1), generator=g), torch.randint(0, 16, (B, T, 3), generator=g)], 2)
    labels[0, :9, :] = IGN
    labels[3, 40:, 2] = IGN
    labels = labels.to(DEV)
    seen = []
    real = losses.fused_linear_cross_entropy

    def spy(hidden, lab, weight, bias=None, ignore_index=-100, **kw):
        seen.append((hidden.detach().reshape(-1, hidden.shape[-1]).clone(), lab.reshape(-1).clone(), weight.detach().clone(),
                     bias.detach().clone()))
        return real(hidden, lab, weight, bias, ignore_index, **kw)

    import rwkvtts_amd.xy_llm as xy_llm
    monkeypatch.setattr(xy_llm, "fused_linear_cross_entropy", spy)

    def run():
        m.zero_grad(set_to_none=True)
        del seen[:]
        launches = losses.LOGIT_REG_HITS[0]
        loss = m(input_ids=ids, labels=labels).loss
        loss.backward()
        return loss.item(), _head_grads(m), losses.LOGIT_REG_HITS[0] - launches, list(seen)

    def errors(res, z, c):
        """{(route, tensor): relative L2 error against fp64 from the route's own logits}"""
        out = {}
        for hip, (_, grads, _, calls) in zip((True, False), res):
            assert len(calls) == 4
            for i, (h, lab, W, b) in enumerate(calls):
                dW, db = _head_grads_fp64(h, lab, W, b, hip, LS, z, c)
                out["hip" if hip else "torch", f"heads.{i}.weight"] = _rel_l2(grads[f"heads.{i}.weight"], dW)
                out["hip" if hip else "torch", f"heads.{i}.bias"] = _rel_l2(grads[f"heads.{i}.bias"], db)
        return out

    on = _both_routes(monkeypatch, run)
    got = errors(on, Z, C)
    m.config.z_loss = m.config.max_logit = 0.0
    plain = errors(_both_routes(monkeypatch, run, reg=False), 0.0, 0.0)
    (l1, _, n1, _), (l0, _, _, _) = on
    print(f"PARITY xy model loss {abs(l1 - l0):.3e} 1.000e-04")
    for k in got:
        print(f"PARITY xy model {k[0]} {k[1]} {got[k]:.3e} plain {plain[k]:.3e}")
    assert n1 == 4, "one launch per channel"
    assert abs(l1 - l0) < 1e-4 and len(got) == 16
    for k in got:
        assert got[k] <= 2 * plain[k], (k, got[k], plain[k])


def test_trainer_statistics_leave_the_digest_alone_and_equal_the_fp64_values(hip_lib, yardstick, monkeypatch):
    """logit_stats=True with both coefficients 0: the same parameters, moments and digest as without it, and last_logit_stats against
    fp64 from the logits the head saw (its hidden states and labels are recorded on the way in; F.linear gives the head's own bf16
    logits).  Bars from the kernel's measured bar 2 E on lse (absolute): mean_lse within 2 E, mean_lse_sq within 2 max|lse| 2 E
    + (2 E)^2; the row maxima are exact, so mean_max carries the fp32 sums alone: 16 ulp."""
    seen = []
    real = losses.fused_linear_cross_entropy

    def spy(hidden, labels, weight, bias=None, ignore_index=-100, **kw):
        seen.append((hidden.detach().clone(), labels.clone(), weight.detach().clone(), kw.get("stats") is not None))
        return real(hidden, labels, weight, bias, ignore_index, **kw)

    import rwkvtts_amd.spark_llm as spark_llm
    monkeypatch.setattr(spark_llm, "fused_linear_cross_entropy", spy)

    def run(**kw):
        torch.manual_seed(12)
        m = _no_dropout(_spark(vocab=8193).train())
        tr = trainer.DataParallelTrainer(m, **KW, **kw)
        for s_ in (41, 42):
            tr.step(**_pairs(m, 2, 64, seed=s_))
        return tr

    a, b = run(), run(logit_stats=True)
    torch.cuda.synchronize()
    assert a.last_logit_stats is None and [s_[3] for s_ in seen] == [False, False, True, True]
    assert a.digest() == b.digest() and torch.equal(a.flat.flat_param, b.flat.flat_param) and torch.equal(a.exp_avg, b.exp_avg)
    hidden, labels, weight, _ = seen[-1]   # the statistics are the last optimizer step's
    x = F.linear(hidden.reshape(-1, hidden.shape[-1]), weight).double()
    valid = labels.reshape(-1) != IGN
    lse, mx = torch.logsumexp(x, 1)[valid], x.max(1).values[valid]
    got = {k: v.item() for k, v in b.last_logit_stats.items()}
    E2 = 2 * yardstick
    want = dict(tokens=valid.sum().item(), mean_lse=lse.mean().item(), mean_lse_sq=(lse * lse).mean().item(), mean_max=mx.mean().item())
    bars = dict(tokens=0.0, mean_lse=E2, mean_lse_sq=2 * lse.abs().max().item() * E2 + E2 * E2, mean_max=2 ** -20 * abs(want["mean_max"]))
    for k in want:
        print(f"PARITY trainer stats {k} {abs(got[k] - want[k]):.3e} {bars[k]:.3e}")
    for k in want:
        assert abs(got[k] - want[k]) <= bars[k], (k, got[k], want[k])
