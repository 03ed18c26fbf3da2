"""GPU (-m gpu): policy-gradient (GRPO / PPO-clip) training on the HIP route -- rwkv7_ce_policy_fwd_bwd_bf16
alone, losses.fused_linear_policy, the heads' policy_loss / token_logprobs on the real backbone, DataParallelTrainer.policy_step.

Kernel, rho = 1: NO tolerance -- with old_lp = the kernel's own lp_rows and no reference, every row equals bit for bit what
rwkv7_ce_seq_bwd_bf16 writes with seq_scale = the fp32 product seq_w * adv.
Kernel, general: MEASURED against yardsticks on the same bf16 logits, the reference being plain autograd in fp64 (minimum, clamp, k3).
  per-row lp / l_t / kl : max |error| <= 2 x the max |error| of rwkv7_head_eval_bf16's loss_rows against ITS fp64 restatement.  lp is that
      value negated, bit for bit; l_t and kl follow from lp in double with |d l_t / d lp| = |rho A| <= 1.3 and |d kl / d lp| < 0.5 for the
      inputs used here (|A| <= 0.8, |log rho| <= 0.42, |d| <= 0.35), plus one fp32 rounding of the result.
  gradient rows         : relative L2 error <= 2 x that of rwkv7_ce_seq_bwd_bf16 (seq_scale = seq_w * adv) against ITS restatement.
  clip_rows             : equal to the fp64 decision on every row whose fp64 rho is further than 1e-4 (relative) from both bounds.
fused_linear_policy: dh / dW / db against fp64 autograd on the same bf16 inputs, the bar 2 x fused_linear_cross_entropy's own error.
Every comparison prints `PARITY <case> <observable> <error> <yardstick>`; the record of one run is profiles/policy_head_parity.txt."""
import pytest
import torch
import torch.nn.functional as F

from rwkvtts_amd import _lib, losses, trainer
from test_policy import BETA, CLIP, N, ce_yardstick, policy_case, policy_fp64
from test_preference_gpu import HEADS, KW, SENTINEL, _bits, _grad_names, _pairs, _rel_l2, _spark

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IGN = -100
NAME = "rwkv7_ce_policy_fwd_bwd_bf16"
EPS = (0.2, 0.2)
KBETA = 0.3
SHAPES = [(5, 8), (1025, 1032), (6562, 6568), (8193, 8193), (8193, 8448)]
# rows = 70: rows 0-4 in front; one row; an empty sequence; 22 falls inside the workgroup of rows 20-23; rows 60-69 behind
# rows = 9 : row 0 in front; one row; an empty sequence; two sequences of three rows; row 8 behind
LAYOUT = {70: ([5, 6, 6, 22, 41, 60], [2, 7, 23, 40, 59, 63], 25), 9: ([1, 2, 2, 5, 8], [3], 4)}
ADV = [0.8, 0.5, -0.6, 0.7, -0.8]
# weights of one size: a relative L2 error over rows of which ONE carries all the weight is the rounding luck of its few largest elements
SEQ_W = [0.07, 0.3, 1.0 / 16, 1.0 / 19, 1.0 / 19]
LOG_RHO = [-0.40, 0.40, 0.30, -0.30, 0.35, -0.05]   # by row, cyclically: both sides of both bounds whatever the advantage's sign
REF_D = [0.30, -0.20, 0.10, -0.35, 0.0]


def kernel_case(rows, V, ld, row0):
    """CPU tensors of one kernel case: logits [rows, ld] (sentinel bits behind column V), labels, seq_start, adv, seq_w, the sequence of
    every row (-1: none), and old / ref of every BATCH row (row0 + rows entries) placed around the fp64 log-probability of the bf16
    logits at chosen distances."""
    g = torch.Generator().manual_seed(V + ld + row0 + rows)
    offsets, ignored, last_col = LAYOUT[rows]
    x = torch.zeros(rows, ld, dtype=torch.bfloat16)
    x[:, :V] = (torch.randn(rows, V, generator=g) * 3).bfloat16()
    _bits(x)[:, V:] = SENTINEL
    lab = torch.randint(0, V, (rows,), generator=g)
    lab[ignored] = IGN
    lab[last_col] = V - 1
    n_seq = len(offsets) - 1
    seq_of = torch.full((rows,), -1)
    for s in range(n_seq):
        seq_of[offsets[s]:offsets[s + 1]] = s
    lp = F.log_softmax(x[:, :V].double(), dim=1).gather(1, lab.clamp(min=0).unsqueeze(1)).squeeze(1)
    t = torch.arange(rows)
    jitter = (torch.rand(rows, generator=g, dtype=torch.float64) - 0.5) * 0.04
    old, ref = torch.zeros(row0 + rows), torch.zeros(row0 + rows)
    old[row0:] = (lp - torch.tensor(LOG_RHO, dtype=torch.float64)[t % 6] - jitter).float()
    ref[row0:] = (lp + torch.tensor(REF_D, dtype=torch.float64)[t % 5]).float()
    return dict(x=x, lab=lab, st=torch.tensor(offsets) + row0, adv=torch.tensor(ADV[:n_seq]), w=torch.tensor(SEQ_W[:n_seq]),
                seq_of=seq_of, on=(seq_of >= 0) & (lab != IGN), old=old, ref=ref, V=V, ld=ld, rows=rows, row0=row0)


def kernel_fp64(c, with_ref):
    """The fp64 restatement on the case's bf16 logits: (d loss / d logits [rows, V], lp, l_t, kl, clipped, rho), masked to the rows
    that count."""
    x = c["x"][:, :c["V"]].double().requires_grad_()
    lp = F.log_softmax(x, dim=1).gather(1, c["lab"].clamp(min=0).unsqueeze(1)).squeeze(1)
    s, on, r0 = c["seq_of"].clamp(min=0), c["on"], c["row0"]
    A, rho = c["adv"].double()[s], torch.exp(lp - c["old"][r0:].double())
    s1, s2 = rho * A, rho.clamp(1 - EPS[0], 1 + EPS[1]) * A
    per, kl = -torch.minimum(s1, s2), torch.zeros_like(lp)
    if with_ref:
        d = c["ref"][r0:].double() - lp
        kl = torch.exp(d) - d - 1
        per = per + KBETA * kl
    (per * c["w"].double()[s] * on).sum().backward()
    return x.grad, lp.detach() * on, per.detach() * on, kl.detach() * on, (s1 > s2) & on, rho.detach()


def run_kernel(c, old, ref, adv=None, w=None, rows=None, first=0, st=None):
    """The entry on a fresh device copy of rows first .. first + rows - 1 of the case: (the rewritten logits, stats fp32 [4, rows])."""
    rows = c["rows"] - first if rows is None else rows
    whole = c["x"].to(DEV).clone()
    x = whole[first:first + rows]   # a view: every row keeps its address modulo 16 bytes, as in a chunk walk over one buffer
    st = (c["st"] if st is None else st).to(DEV)
    adv, w = (c["adv"] if adv is None else adv).to(DEV), (c["w"] if w is None else w).to(DEV)
    stats = torch.full((4, rows + 2), -77.0, device=DEV)
    _lib.call(NAME, x, rows, c["V"], c["ld"], x, c["lab"].to(DEV)[first:first + rows].contiguous(), IGN, c["row0"] + first, st.numel() - 1,
              st, adv, w, old.to(DEV), None if ref is None else ref.to(DEV), EPS[0], EPS[1], KBETA, stats[0, 1:], stats[1, 1:],
              stats[2, 1:], stats[3, 1:])
    torch.cuda.synchronize()
    assert bool((stats[:, 0] == -77).all()) and bool((stats[:, -1] == -77).all()), "per-row outputs written outside [0, rows)"
    assert torch.equal(_bits(x)[:, c["V"]:].cpu(), _bits(c["x"])[first:first + rows, c["V"]:]), "columns V .. ld - 1 must stay untouched"
    return x, stats[:, 1:-1]


CASES = [(rows, V, ld, row0) for rows in (9, 70) for V, ld in SHAPES for row0 in (0, 1000)]


@pytest.mark.parametrize("rows,V,ld,row0", CASES)
def test_at_rho_one_the_rows_are_the_sequence_scale_kernels_bit_for_bit(hip_lib, rows, V, ld, row0):
    c = kernel_case(rows, V, ld, row0)
    _, first = run_kernel(c, torch.zeros(row0 + rows), None)
    old = torch.zeros(row0 + rows, device=DEV)
    old[row0:] = first[0]
    got, stats = run_kernel(c, old, None)
    want = c["x"].to(DEV).clone()
    assert want.data_ptr() % 16 == got.data_ptr() % 16
    scale = (c["w"] * c["adv"]).to(DEV)   # the fp32 product
    _lib.call("rwkv7_ce_seq_bwd_bf16", want, rows, V, ld, want, c["lab"].to(DEV), IGN, row0, scale.numel(), c["st"].to(DEV), scale, None)
    assert torch.equal(_bits(got), _bits(want))
    on = c["on"].to(DEV)
    assert bool((got[~on][:, :V] == 0).all()) and bool((got[on][:, :V] != 0).any(dim=1).all())
    assert torch.equal(stats[0], first[0]) and bool((stats[0][~on] == 0).all()) and bool((stats[0][on] < 0).all())
    assert torch.equal(stats[1], torch.where(on, -c["adv"].to(DEV)[c["seq_of"].clamp(min=0).to(DEV)], torch.zeros_like(stats[1])))
    assert bool((stats[2] == 0).all()) and bool((stats[3] == 0).all())


@pytest.mark.parametrize("with_ref", [True, False])
@pytest.mark.parametrize("rows,V,ld,row0", CASES)
def test_against_the_fp64_restatement(hip_lib, rows, V, ld, row0, with_ref):
    c = kernel_case(rows, V, ld, row0)
    grad, lp, per, kl, clipped, rho = kernel_fp64(c, with_ref)
    on, n_on = c["on"], int(c["on"].sum())
    near = on & (((rho / (1 - EPS[0]) - 1).abs() <= 1e-4) | ((rho / (1 + EPS[1]) - 1).abs() <= 1e-4))
    assert 4 * int(clipped.sum()) >= n_on and 4 * int((on & ~clipped).sum()) >= n_on, (n_on, int(clipped.sum()))
    assert 50 * int(near.sum()) <= n_on and bool((c["adv"] > 0).any()) and bool((c["adv"] < 0).any())
    got, stats = run_kernel(c, c["old"], c["ref"] if with_ref else None)
    got, stats = got[:, :V].cpu(), stats.cpu()
    # the yardsticks on the same logits: the evaluation kernel's row loss, the sequence-scale kernel's gradient
    x, lab = c["x"].to(DEV), c["lab"].to(DEV)
    ev, ok = torch.empty(rows, device=DEV), torch.empty(rows, dtype=torch.int32, device=DEV)
    _lib.call("rwkv7_head_eval_bf16", x, rows, V, ld, x, lab, IGN, 0, 0.0, ev, ok, None)
    nll = -F.log_softmax(c["x"][:, :V].double(), dim=1).gather(1, c["lab"].clamp(min=0).unsqueeze(1)).squeeze(1) * (c["lab"] != IGN)
    yard_row = (ev.cpu().double() - nll).abs().max().item()
    seq = x.clone()
    scale = (c["w"] * c["adv"]).to(DEV)
    _lib.call("rwkv7_ce_seq_bwd_bf16", seq, rows, V, ld, seq, lab, IGN, row0, scale.numel(), c["st"].to(DEV), scale, None)
    p = torch.softmax(c["x"][:, :V].double(), dim=1)
    p.scatter_add_(1, c["lab"].clamp(min=0).unsqueeze(1), torch.full_like(p[:, :1], -1.0))
    want_seq = p * (scale.cpu().double()[c["seq_of"].clamp(min=0)] * on).unsqueeze(1)
    keep = on & ~near
    yard_grad = _rel_l2(seq[:, :V].cpu()[keep], want_seq[keep])
    case = f"rows={rows} V={V} ld={ld} row0={row0} ref={int(with_ref)}"
    errs = {k: (stats[i].double() - v).abs().max().item() for i, (k, v) in enumerate((("lp", lp), ("l_t", per), ("kl", kl)))}
    err_grad = _rel_l2(got[keep], grad[keep])
    for k, e in errs.items():
        print(f"PARITY kernel {case} {k} {e:.3e} {yard_row:.3e}")
    print(f"PARITY kernel {case} grad {err_grad:.3e} {yard_grad:.3e}")
    assert torch.equal(stats[3][keep] != 0, clipped[keep]) and bool((stats[3][~on] == 0).all())
    assert bool((stats[:3, ~on] == 0).all()) and bool((got[~on] == 0).all())
    assert (bool((stats[2] != 0).any())) == with_ref
    for k, e in errs.items():
        assert e <= 2 * yard_row, (k, e, yard_row)
    assert err_grad <= 2 * yard_grad, (err_grad, yard_grad)


@pytest.mark.parametrize("V,ld", SHAPES)
@pytest.mark.parametrize("row0", [0, 1000])
def test_rows_depend_on_neither_the_other_sequences_nor_the_split_of_the_launch(hip_lib, V, ld, row0):
    rows = 70
    c = kernel_case(rows, V, ld, row0)
    whole, stats = run_kernel(c, c["old"], c["ref"])
    # sequence 3 alone in the launch, under another index: its rows keep every bit, all others are zeros
    alone, alone_stats = run_kernel(c, c["old"], c["ref"], adv=c["adv"][3:4], w=c["w"][3:4], st=c["st"][3:5])
    mine = (c["seq_of"] == 3).to(DEV)
    assert torch.equal(_bits(alone)[mine], _bits(whole)[mine]) and torch.equal(alone_stats[:, mine], stats[:, mine])
    assert bool((alone[~mine][:, :V] == 0).all()) and bool((alone_stats[:, ~mine] == 0).all())
    # the other sequences' advantages and weights changed: the same
    other, other_stats = run_kernel(c, c["old"], c["ref"], adv=torch.where(torch.arange(5) == 3, c["adv"], c["adv"] * -3.0),
                                    w=torch.where(torch.arange(5) == 3, c["w"], c["w"] * 0.37))
    assert torch.equal(_bits(other)[mine], _bits(whole)[mine]) and torch.equal(other_stats[:, mine], stats[:, mine])
    # one launch over 70 rows against two over rows 0-29 and 30-69 (a split inside sequence 3, off the workgroups' four-row grid)
    a, a_stats = run_kernel(c, c["old"], c["ref"], rows=30)
    b, b_stats = run_kernel(c, c["old"], c["ref"], first=30)
    assert torch.equal(_bits(torch.cat((a, b))), _bits(whole)) and torch.equal(torch.cat((a_stats, b_stats), 1), stats)


# ---- fused_linear_policy on the HIP route ----------------------------------------------------------------------------------------------
def _policy_grads(case, ref, chunk):
    h, w, b, lab, st, adv, seq_w, old, _ = case
    leaves = [t.detach().clone().requires_grad_() for t in (h, w, b)]
    loss, rows = losses.fused_linear_policy(leaves[0], lab, leaves[1], leaves[2], IGN, seq_start=st, adv=adv, seq_w=seq_w, old_logp=old,
                                            ref_logp=ref, clip=CLIP, kl_beta=BETA, chunk=chunk)
    loss.backward()
    return loss.detach(), rows, [t.grad for t in leaves]


@pytest.fixture(scope="module")
def parity(hip_lib):
    case = policy_case(dtype=torch.bfloat16, device=DEV)
    h, w, b, lab, st, adv, seq_w, old, ref = case
    refs = [t.double().requires_grad_() for t in (h, w, b)]
    want = policy_fp64(*refs, lab, st, adv, seq_w, old, ref, CLIP, BETA)
    want[0].backward()
    got = {}
    for chunk, launches in ((64, 4), (128, 2), (N, 1)):   # 64: 0, 64, 128 and the last 64 rows; 128: 0 and the last 128 rows
        hits = losses.POLICY_HITS[0]
        got[chunk] = _policy_grads(case, ref, chunk)
        assert losses.POLICY_HITS[0] == hits + launches, "the HIP route: one rwkv7_ce_policy_fwd_bwd_bf16 launch per chunk"
    return dict(case=case, want=want, want_grads=[t.grad for t in refs], yard=ce_yardstick(h, w, b, lab, N), got=got)


def test_fused_gradients_within_twice_the_cross_entropy_paths_own_error(parity):
    want, lp, kl, clipped, rho = parity["want"]
    scale = (parity["case"][6].double()[losses._row_sequences(parity["case"][4], 0, N)[0]] * (lp != 0)).sum().item()
    for chunk, (loss, rows, grads) in parity["got"].items():
        err = abs(loss.item() - want.item()) / scale
        print(f"PARITY fused chunk={chunk} loss {err:.3e} (of the sum of the row weights) lp {(rows['logp'] - lp).abs().max().item():.3e}")
        # bf16 logits: a row's lp is off by a few bf16 roundings of logits of size <= 4 (2^-8 each); the loss is a weighted mean of
        # terms with |d l / d lp| <= 3
        assert err <= 3 * 2 ** -6 and bool(((rows["logp"] - lp).abs() <= 2 ** -5).all())
        assert grads[0].dtype == grads[1].dtype == torch.bfloat16
        for name, g_, r, yard in zip(("dh", "dW", "db"), grads, parity["want_grads"], parity["yard"]):
            e = _rel_l2(g_, r)
            print(f"PARITY fused chunk={chunk} {name} {e:.3e} {yard:.3e}")
            assert 0 < e <= 2 * yard, (chunk, name, e, yard)


def test_an_overlapping_last_chunk_is_not_counted_twice(parity):
    """N = 200, chunk = 128: the last chunk is rows 72 .. 199 and overlaps 56 rows of the first."""
    h, w, b, lab, st, adv, seq_w, old, ref = parity["case"]
    one, two = parity["got"][N][2], parity["got"][128][2]
    rows = slice(72, 128)
    x = F.linear(h[rows], w, b).double()   # the overlapped rows' contribution, restated in torch from the bf16 logits
    sq, inside = losses._row_sequences(st, 72, 56)
    sc = losses._policy_rows_torch(x, lab[rows], IGN, sq, inside, adv, seq_w, old[rows], ref[rows], 1 - CLIP[0], 1 + CLIP[1], BETA)[4]
    pd = losses._grad_rows_torch(x, lab[rows], 0.0, sc).bfloat16()
    extra = dict(dW=(pd.t() @ h[rows]).float(), db=pd.float().sum(0))
    assert bool((sc != 0).any())
    for name, i in (("dW", 1), ("db", 2)):
        bar = 2 * parity["yard"][i]
        same, doubled = _rel_l2(two[i], one[i]), _rel_l2(two[i], one[i].float() + extra[name])
        print(f"PARITY fused overlap {name} {same:.3e} {parity['yard'][i]:.3e} double-counted {doubled:.3e}")
        assert same <= bar, (name, same, bar)
        assert doubled > 10 * bar, (name, doubled, bar)
    assert _rel_l2(two[0], one[0]) <= 2 * parity["yard"][0]   # dh: every row written once, by the chunk that owns it
    assert torch.equal(parity["got"][128][1]["clipped"], parity["got"][N][1]["clipped"])


def test_peak_memory_stays_below_the_materialised_fp32_route(hip_lib):
    """N = 4096 rows, V = 8193: the peak of loss + backward against fp32 logits -> log_softmax -> the same objective in torch."""
    rows, D_, V_ = 4096, 256, 8193
    g = torch.Generator().manual_seed(3)
    h = torch.randn(rows, D_, generator=g).bfloat16().to(DEV).requires_grad_()
    w = (torch.randn(V_, D_, generator=g) * 0.1).bfloat16().to(DEV).requires_grad_()
    lab = torch.randint(0, V_, (rows,), generator=g).to(DEV)
    st = torch.arange(9, device=DEV) * 512
    adv, seq_w = torch.linspace(-1, 1, 8, device=DEV), torch.full((8,), 1 / 4096, device=DEV)
    old = torch.full((rows,), -9.0, device=DEV)

    def fused():
        losses.fused_linear_policy(h, lab, w, None, IGN, seq_start=st, adv=adv, seq_w=seq_w, old_logp=old, clip=CLIP)[0].backward()

    def materialised():
        lp = F.log_softmax(F.linear(h, w).float(), dim=-1).gather(1, lab.unsqueeze(1)).squeeze(1)
        rho, A = torch.exp(lp - old), adv.repeat_interleave(512)
        (-torch.minimum(rho * A, rho.clamp(1 - CLIP[0], 1 + CLIP[1]) * A) / 4096).sum().backward()

    peaks = []
    for fn in (fused, materialised):
        fn()   # warm-up: workspaces and caches exist before the measured call
        h.grad = w.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - base)
        h.grad = w.grad = None
    print(f"PARITY fused memory {peaks[0] / 2 ** 20:.1f} MiB materialised {peaks[1] / 2 ** 20:.1f} MiB")
    assert peaks[0] < peaks[1], peaks


# ---- the heads on the real backbone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", list(HEADS))
def test_reduction_on_the_heads_of_the_real_backbone(hip_lib, head):
    """old_logps = token_logprobs, advantages = 1, no KL, normalize = "token": the loss is -1 and no row is clipped, up to what the
    backbone's training nodes (autograd on) and its inference nodes (token_logprobs) differ by in bf16.  (The gradients of the
    reduction: test_reduction_policy_step_has_steps_gradient, through the trainer.)"""
    m, batch, tokens = HEADS[head]()
    n = len(tokens)
    old = m.token_logprobs(**batch())
    assert old.dtype == torch.float32 and int((old != 0).sum()) == sum(tokens) and not m.training
    hits = losses.POLICY_HITS[0]
    out = m.policy_loss(advantages=torch.ones(n), old_logps=old, normalize="token", **batch())
    assert losses.POLICY_HITS[0] == hits + 1 and int(out["valid"].sum()) == sum(tokens)
    rho = torch.exp(out["logp"] - old)[out["valid"]]
    print(f"PARITY {head} reduction loss+1 {abs(out['loss'].item() + 1):.3e} max|rho-1| {(rho - 1).abs().max().item():.3e}")
    # one bf16 rounding of a logit of size <= 8 is 2^-6: a token's ratio may be off by a few of those, their mean by far less
    assert abs(out["loss"].item() + 1) <= 2 ** -7 and bool(((rho - 1).abs() <= 2 ** -3).all()) and not bool(out["clipped"].any())
    got = _grad_names(m, out["loss"])
    trained = _grad_names(m, m(**batch()).loss)
    assert got == trained and any("lm_head" in k for k in got) and len(got) > 20


LENS = [24, 20, 12, 8]   # four utterances: the rows of one packed [1, 64] batch, or of a right-padded [4, 64] one


def _two_layouts(seed=31):
    """The same four utterances packed (cu_seqlens) and padded (right-padded rows: the backbone is causal, so what follows an utterance
    in its row does not reach it).  Every utterance's first label is -100: after the shift by one no row of the packed batch predicts
    across a boundary, and row cu[i] + t of the packed batch is row (i, t) of the padded one.  Returns the two batches and the index of
    each utterance's rows in the two flattened layouts."""
    g = torch.Generator().manual_seed(seed)
    total, T = sum(LENS), 64
    cu = torch.tensor([0] + LENS).cumsum(0)
    emb = (torch.randn(1, total, 256, generator=g) * 0.5).bfloat16()
    labels = torch.randint(0, 256, (1, total), generator=g)
    labels[0, cu[:-1]] = -100
    pe, pl = torch.zeros(4, T, 256, dtype=torch.bfloat16), torch.full((4, T), -100)
    for i, (s, n) in enumerate(zip(cu.tolist(), LENS)):
        pe[i, :n], pl[i, :n] = emb[0, s:s + n], labels[0, s:s + n]
    packed = dict(inputs_embeds=emb.to(DEV), labels=labels.to(DEV), cu_seqlens=cu.to(DEV))
    padded = dict(inputs_embeds=pe.to(DEV), labels=pl.to(DEV))
    rows_packed = torch.arange(total, device=DEV)
    rows_padded = torch.cat([i * T + torch.arange(n) for i, n in enumerate(LENS)]).to(DEV)
    return packed, padded, rows_packed, rows_padded


def _named_grads(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None and bool((p.grad != 0).any())}


def _compare_grads(case, got, want, other):
    """got against want, tensor by tensor and as one flat vector; the yardstick is want against `other`, a second route to the same
    gradient.  The bar is 2 x the yardstick; a tensor on which the two routes happen to agree better than they do overall is held to
    the overall figure."""
    assert set(got) == set(want) == set(other) and len(want) > 20 and any("lm_head" in k for k in want), set(got) ^ set(want)
    flat = lambda d: torch.cat([d[k].reshape(-1).double() for k in sorted(want)])   # noqa: E731
    err, yard = _rel_l2(flat(got), flat(want)), _rel_l2(flat(other), flat(want))
    print(f"PARITY {case} flat gradient {err:.3e} {yard:.3e}")
    worst = max(((_rel_l2(got[k], want[k]), _rel_l2(other[k], want[k]), k) for k in want), key=lambda t: t[0] / max(t[1], yard))
    print(f"PARITY {case} worst tensor {worst[2]} {worst[0]:.3e} {worst[1]:.3e}")
    assert 0 < yard and err <= 2 * yard, (err, yard)
    for k in want:
        e, y = _rel_l2(got[k], want[k]), _rel_l2(other[k], want[k])
        assert e <= 2 * max(y, yard), (k, e, y, yard)


def _no_dropout(m):
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m


def test_packed_cu_seqlens_and_padded_batches_of_the_same_utterances_agree(hip_lib, parity):
    """policy_loss on the packed and on the padded layout of the same utterances: the loss, every utterance's rows of logp / kl /
    clipped, and the gradients of every parameter.  Row values: the two layouts run different backbone nodes, whose bf16 hidden states
    and so the bf16 logits differ in their last bits -- a few roundings of 2^-8 relative on logits of size <= 4: |d logp| <= 2^-5,
    |d kl| <= |1 - exp(d)| |d logp| <= 2^-5, clipped equal wherever rho is further than 2^-5 (relative) from both bounds, and the loss,
    a weighted mean of terms with |d l / d lp| <= 3, within 3 x 2^-5.  Gradients, every parameter, per tensor and flat: the bf16 bar of
    test_preference_gpu -- 2 x the relative L2 error of the fused cross-entropy HIP path against its fp64 restatement.  (How far the
    model's own training loss is apart between the two layouts is printed beside it but is no yardstick: on MI355X the two layouts'
    forward passes agree bit for bit, and what is left in either gradient is a handful of bf16 roundings that fall the other way
    because the gradient GEMMs sum over 64 rows in one layout and over 256, most of them zeros, in the other -- 2.5e-5 against 4.1e-6,
    two counts of flipped roundings.)"""
    m = _no_dropout(_spark().train())
    packed, padded, rp, rq = _two_layouts()
    adv = torch.tensor([0.7, -0.5, 0.9, -0.6])
    g = torch.Generator().manual_seed(32)
    base = m.token_logprobs(**padded)[rq]
    old, ref = torch.zeros(2, 4 * 64, device=DEV), torch.zeros(2, 4 * 64, device=DEV)
    noise = ((torch.rand(2, sum(LENS), generator=g) - 0.5) * torch.tensor([[0.9], [0.5]])).to(DEV)
    old[1][rq], ref[1][rq] = base + noise[0], base + noise[1]
    old[0][:sum(LENS)], ref[0][:sum(LENS)] = old[1][rq], ref[1][rq]
    outs, grads, ce = [], [], []
    for i, batch in enumerate((packed, padded)):
        n = batch["labels"].numel()
        out = m.policy_loss(advantages=adv, old_logps=old[i][:n], ref_logps=ref[i][:n], clip=CLIP, kl_beta=BETA, **batch)
        _grad_names(m, out["loss"])
        outs.append(out)
        grads.append(_named_grads(m))
        _grad_names(m, m(**batch).loss)
        ce.append(_named_grads(m))
    a, b = outs
    assert int(a["valid"].sum()) == int(b["valid"].sum()) == sum(LENS) - 4 and torch.equal(a["valid"][rp], b["valid"][rq])
    assert not bool(b["valid"].clone().index_fill_(0, rq, False).any()), "the padding rows of the padded batch do not count"
    d_lp, d_kl = (a["logp"][rp] - b["logp"][rq]).abs().max().item(), (a["kl"][rp] - b["kl"][rq]).abs().max().item()
    d_loss = abs(a["loss"].item() - b["loss"].item())
    rho = torch.exp(b["logp"][rq] - old[1][rq])
    far = ((rho / (1 - CLIP[0]) - 1).abs() > 2 ** -5) & ((rho / (1 + CLIP[1]) - 1).abs() > 2 ** -5)
    print(f"PARITY packed/padded loss {d_loss:.3e} logp {d_lp:.3e} kl {d_kl:.3e} rows outside the band {int(far.sum())} of {far.numel()}")
    assert d_lp <= 2 ** -5 and d_kl <= 2 ** -5 and d_loss <= 3 * 2 ** -5
    assert torch.equal(a["clipped"][rp][far], b["clipped"][rq][far]) and 0 < b["clipped"].sum() < b["valid"].sum()
    assert 3 * int((far & b["valid"][rq]).sum()) >= 2 * int(b["valid"].sum()), "the inputs: most rows' decision must be comparable"
    # the bar: 2 x the smallest of the cross-entropy path's own errors against fp64 (dh, dW, db of the `parity` case), per tensor and flat
    assert set(grads[0]) == set(grads[1]) == set(ce[0]) == set(ce[1]) and len(ce[0]) > 20 and any("lm_head" in k for k in ce[0])
    flat = lambda d: torch.cat([d[k].reshape(-1).double() for k in sorted(ce[0])])   # noqa: E731
    yard = min(parity["yard"])
    err, layouts = _rel_l2(flat(grads[0]), flat(grads[1])), _rel_l2(flat(ce[0]), flat(ce[1]))
    worst = max((_rel_l2(grads[0][k], grads[1][k]), k) for k in ce[0])
    print(f"PARITY packed/padded flat gradient {err:.3e} {yard:.3e} (the training loss's own gradient, packed against padded: "
          f"{layouts:.3e}) worst tensor {worst[1]} {worst[0]:.3e}")
    assert err <= 2 * yard and worst[0] <= 2 * yard, (err, worst, yard)


# ---- DataParallelTrainer.policy_step on the HIP AdamW path ---------------------------------------------------------------------------
def _spark_trainer_case():
    m = _no_dropout(_spark().train())
    batch = _pairs(m, 2, 64, seed=24)

    def other_route(model):
        model.config.fuse_cross_entropy = not model.config.fuse_cross_entropy
    return m, batch, 4, other_route


def _cosy_trainer_case():
    llm, batch, tokens = HEADS["cosy"]()

    def other_route(model):
        model.config.fused_loss = not model.config.fused_loss
    return llm.train(), batch(), len(tokens), other_route


@pytest.mark.parametrize("case", ["spark", "cosy"])
def test_reduction_policy_step_has_steps_gradient(hip_lib, case):
    """old_logps = token_logprobs, advantages = 1, no KL, normalize = "token", training mode without dropout: policy_step's loss is -1
    and the gradient it leaves in the flat buffer is step's at the same batch (the token-mean cross-entropy; Cosy without label
    smoothing, length-normalised) -- every parameter, tensor by tensor and flat.  The yardstick is step against step with the head's
    other route to the same loss (Spark: fuse_cross_entropy off, i.e. materialised logits; Cosy: fused_loss switched); bar 2 x."""
    import copy
    m, batch, n, other_route = dict(spark=_spark_trainer_case, cosy=_cosy_trainer_case)[case]()
    twins = [copy.deepcopy(m) for _ in range(2)]
    other_route(twins[1])
    trs = [trainer.DataParallelTrainer(x, **KW) for x in [m] + twins]
    assert all(t.hip_adamw for t in trs)
    old = trs[0].token_logprobs([batch])[0]
    hits = losses.POLICY_HITS[0]
    out = trs[0].policy_step(advantages=torch.ones(n), old_logps=old, normalize="token", **batch)
    loss_step = trs[1].step(**batch)
    trs[2].step(**batch)
    torch.cuda.synchronize()
    assert losses.POLICY_HITS[0] == hits + 1 and all(t.step_idx == 1 and t.nan_flag.item() == 0 for t in trs)
    print(f"PARITY {case} trainer reduction loss+1 {abs(out['loss'].item() + 1):.3e} clip_frac {out['clip_frac'].item():.3e} "
          f"ratio_mean-1 {abs(out['ratio_mean'].item() - 1):.3e}")
    assert abs(out["loss"].item() + 1) <= 2 ** -7 and out["clip_frac"].item() == 0 and out["kl"].item() == 0
    assert abs(out["ratio_mean"].item() - 1) <= 2 ** -7 and bool(torch.isfinite(loss_step))
    got, want, other = (_named_grads(t.model) for t in trs)
    _compare_grads(f"{case} trainer reduction", got, want, other)


def test_a_step_after_a_policy_step_equals_a_step_after_loading_that_state(hip_lib, tmp_path):
    torch.manual_seed(5)
    a = trainer.DataParallelTrainer(_spark().train(), **KW)   # training mode: dropout draws, the checkpoint carries the random streams
    batches = [_pairs(a.model, 2, 64, seed=s) for s in (70, 72, 73)]
    a.step(**batches[0])
    old = a.token_logprobs([batches[1]])[0]
    a.policy_step(advantages=torch.tensor([1.0, -1.0, 0.5, -0.5]), old_logps=old, ref_logps=old, kl_beta=BETA, **batches[1])
    a.save_checkpoint(str(tmp_path))
    a.step(**batches[2])
    torch.manual_seed(6)
    b = trainer.DataParallelTrainer(_spark(seed=4).train(), **KW)
    b.load_checkpoint(str(tmp_path))
    b.step(**batches[2])
    torch.cuda.synchronize()
    assert a.step_idx == b.step_idx == 3
    for name in ("master", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a.flat.flat_param, b.flat.flat_param) and torch.equal(a.flat.flat_grad, b.flat.flat_grad)


@pytest.mark.timeout(120)
def test_policy_step_on_the_hip_path(hip_lib):
    torch.manual_seed(11)
    m = _spark(vocab=8193).train()
    tr = trainer.DataParallelTrainer(m, max_grad_norm=1.0, **KW)
    assert tr.hip_adamw
    batch = _pairs(m, 4, 512, seed=21)   # 8 candidates, N = 8 x 512 = 4096 rows, V = 8193
    old = tr.token_logprobs([batch])[0]
    assert old.is_cuda and old.shape == (4096,) and m.training
    adv = losses.group_advantages(torch.tensor([0.1, 0.9, 0.4, 0.2, 0.8, 0.3, 0.5, 0.7]), 4)
    hits = losses.POLICY_HITS[0]
    outs = [tr.policy_step(advantages=adv, old_logps=old, ref_logps=old, kl_beta=0.05, **batch) for _ in range(4)]
    assert losses.POLICY_HITS[0] == hits + 4 and tr.step_idx == 4 and tr.nan_flag.item() == 0
    assert all(v.is_cuda and v.shape == () and bool(torch.isfinite(v)) for o in outs for v in o.values())
    assert abs(outs[0]["ratio_mean"].item() - 1) <= 0.05 and outs[0]["kl"].item() < 1e-2, "on policy up to dropout and bf16"
    assert all(0 <= o["clip_frac"].item() <= 1 and o["kl"].item() >= 0 for o in outs)
    # a NaN among old_logps on a row that counts: step()'s zero-gradient step -- the state a step() on a NaN loss leaves behind
    twin = trainer.DataParallelTrainer(_spark(vocab=8193).train(), max_grad_norm=1.0, **KW)
    for name in ("master", "exp_avg", "exp_avg_sq"):
        getattr(twin, name).copy_(getattr(tr, name))
    twin.flat.flat_param.copy_(tr.flat.flat_param)
    twin.step_idx = tr.step_idx
    bad = old.clone()
    bad[(old != 0).nonzero()[3]] = float("nan")
    tr.policy_step(advantages=adv, old_logps=bad, **batch)
    poisoned = dict(batch, inputs_embeds=batch["inputs_embeds"].clone())
    poisoned["inputs_embeds"][0, 5, 7] = float("nan")
    twin.step(**poisoned)
    torch.cuda.synchronize()
    assert tr.nan_flag.item() == 1 and tr.step_idx == 5
    for name in ("master", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(tr, name), getattr(twin, name)), name
    assert torch.equal(tr.flat.flat_param, twin.flat.flat_param) and bool(torch.isfinite(tr.master).all())
