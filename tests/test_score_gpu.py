"""GPU (-m gpu): rwkv7_seq_scores_f32 and what is built on it (losses.fused_linear_score on the HIP route, the heads' score,
DataParallelTrainer.score).

Kernel alone, on score_fixture's sequences (33 copies of the set, 264 sequences, 49 995 rows) with random inputs: loss_rows
log-uniform in [1e-6, 30] with planted exact duplicates (of ordinary values and of a sequence's maximum), random correct_rows, a tenth
of the labels ignored -- ignored rows carry a large loss and correct = 1, which must not count.  Against score_fixture.reference:
counts, worst_loss (bits) and worst_row exact, loss_sum within n 2^-52 sum|loss_rows| of the row-order fp64 sum (the bound between
any two fp64 summation orders).  The FIXED order is tested as bit-identity of a sequence's outputs when it is scored alone
(n_seq = 1), in the 264-sequence launch, and in a launch whose sequences are laid out in another order (another workgroup each).
Head: on the HIP route the full-length loss_rows equals, bit for bit, the concatenated outputs of rwkv7_head_eval_bf16 run chunk by
chunk on the same GEMM calls, and the five outputs do not depend on the chunk size (7, 64, 200, N).  The gate rounds a chunk up to
64 rows and lets a short last chunk overlap its predecessor: the library GEMM rounds a few logits differently in calls of fewer than
16 rows (measured: 392 of 9.9 M logits at chunk 7 or 8, none in calls of 16 to 1515 rows), so without that rule chunk 7 moved
loss_sum by 3.5e-7 relative.  Heads and trainer: as on the CPU, with the real backbone."""
import pytest
import torch

import score_fixture as SF
from rwkvtts_amd import _lib, layouts as L, losses, trainer
from rwkvtts_amd.cosy_llm import RWKV7CosyConfig, RWKV7CosyLM
from rwkvtts_amd.spark_llm import RWKV7ForSpeech, RWKV7SpeechConfig
from rwkvtts_amd.xy_llm import RWKV7XYConfig, RWKV7XYLM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IGN = -100
SMALL = dict(hidden_size=128, num_hidden_layers=2, decay_low_rank_dim=32, a_low_rank_dim=32, v_low_rank_dim=16, gate_low_rank_dim=32)


# ---- the kernel alone ----------------------------------------------------------------------------------------------------------------
def _launch(st, loss, corr, lab, ignore=IGN):
    """rwkv7_seq_scores_f32 on device inputs -> dict of the five outputs; a sentinel in front of and behind each must survive."""
    n = st.numel() - 1
    types = dict(loss_sum=torch.float64, tokens=torch.int64, correct=torch.int64, worst_loss=torch.float32, worst_row=torch.int64)
    raw = {k: torch.full((n + 2,), -77, dtype=t, device=DEV) for k, t in types.items()}
    _lib.call("rwkv7_seq_scores_f32", loss, n, st, loss, corr, lab, ignore, *[raw[k][1:] for k in losses.SCORE_KEYS])
    torch.cuda.synchronize()
    for k, v in raw.items():
        assert v[0] == -77 and v[-1] == -77, f"{k}: written outside [0, n_seq)"
    return {k: v[1:-1].clone() for k, v in raw.items()}


@pytest.fixture(scope="module")
def rows(hip_lib):
    """CPU inputs of 33 copies of the set, the reference, and the device copies with the 264-sequence launch's outputs."""
    g = torch.Generator().manual_seed(2024)
    n = SF.COPIES * SF.SET_ROWS
    st = SF.seq_start(SF.COPIES)
    lab = SF.labels_for(1000, IGN, g, SF.COPIES)
    loss = torch.exp(torch.empty(n).uniform_(-13.8155, 3.4012, generator=g)).clamp(1e-6, 30.0)   # log-uniform in [1e-6, 30]
    src = torch.randint(0, n, (n // 4,), generator=g)
    loss[torch.randint(0, n, (n // 4,), generator=g)] = loss[src]   # exact duplicates all over
    loss[0], loss[1] = 1e-6, 30.0
    valid = lab != IGN
    for s in range(st.numel() - 1):   # every sequence with three valid rows or more: its maximum at two places
        idx = valid[st[s]:st[s + 1]].nonzero().squeeze(1) + st[s]
        if idx.numel() >= 3:
            a, b = sorted(idx[torch.randperm(idx.numel(), generator=g)[:2]].tolist())
            loss[a] = loss[b] = loss[idx].max()
    corr = torch.randint(0, 2, (n,), generator=g, dtype=torch.int32)
    loss[~valid], corr[~valid] = 1e9, 1   # must not count
    ref = SF.reference(st, loss, corr, lab, IGN)
    dev = tuple(t.to(DEV) for t in (st, loss, corr, lab))
    return dict(cpu=(st, loss, corr, lab), dev=dev, ref=ref, got=_launch(*dev))


def test_kernel_against_the_reference(rows):
    SF.assert_scores(rows["got"], rows["ref"], "264 sequences")
    got = {k: v.cpu() for k, v in rows["got"].items()}
    for i in (2, SF.ALL_IGNORED, 8 + 2, 32 * 8 + SF.ALL_IGNORED):   # the empty range and the all-ignored sequence
        assert [got[k][i].item() for k in losses.SCORE_KEYS] == [0.0, 0, 0, 0.0, -1], i
    assert (got["worst_loss"][got["tokens"] > 0] <= 30.0).all() and got["tokens"].sum() > 40000


def test_a_sequence_scored_alone_has_the_same_bits(rows):
    st, loss, corr, lab = rows["dev"]
    for i in list(range(8)) + list(range(20 * 8, 21 * 8)):   # n_seq = 1: the set's eight sequences, in copy 0 and in copy 20
        alone = _launch(st[i:i + 2].contiguous(), loss, corr, lab)
        SF.assert_bit_identical(alone, {k: v[i:i + 1] for k, v in rows["got"].items()}, f"sequence {i} alone")
    one_set = _launch(st[:9].contiguous(), loss, corr, lab)
    SF.assert_bit_identical(one_set, {k: v[:8] for k, v in rows["got"].items()}, "n_seq = 8")


def test_another_order_of_the_sequences_changes_no_bit(rows):
    st, loss, corr, lab = rows["cpu"]
    g = torch.Generator().manual_seed(5)
    n_seq = st.numel() - 1
    perm = torch.randperm(n_seq, generator=g)
    lens = (st[1:] - st[:-1])[perm]
    gather = torch.cat([torch.arange(st[p], st[p + 1]) for p in perm.tolist()])
    st2 = torch.cat((torch.zeros(1, dtype=torch.int64), lens.cumsum(0)))
    got = _launch(*(t.to(DEV) for t in (st2, loss[gather], corr[gather], lab[gather])))
    SF.assert_bit_identical(got, {k: v[perm.to(DEV)] for k, v in rows["got"].items()}, "permuted")


def test_one_row_next_to_100003_rows_and_a_nan(hip_lib):
    g = torch.Generator().manual_seed(9)
    n = 1 + 100003 + 300
    st = torch.tensor([0, 1, 100004, n])
    loss = torch.rand(n, generator=g) * 12
    lab = torch.randint(0, 50, (n,), generator=g)
    lab[torch.rand(n, generator=g) < 0.2] = IGN
    lab[0], lab[100004 + 200], lab[100004 + 250] = 3, 3, 3
    loss[100004 + 200] = loss[100004 + 250] = float("nan")   # a NaN is the worst row (torch.max / torch.argmax take it so): the first one
    corr = torch.randint(0, 2, (n,), generator=g, dtype=torch.int32)
    ref = SF.reference(st[:3], loss, corr, lab, IGN)
    got = _launch(*(t.to(DEV) for t in (st, loss, corr, lab)))
    SF.assert_scores({k: v[:2] for k, v in got.items()}, ref, "1 and 100003 rows")
    assert got["tokens"][1] > 70000
    assert got["worst_row"][2] == 200 and torch.isnan(got["worst_loss"][2]) and torch.isnan(got["loss_sum"][2])
    assert got["tokens"][2].item() == (lab[100004:] != IGN).sum().item()


# ---- fused_linear_score on the HIP route -----------------------------------------------------------------------------------------------
def _head(V, copies=1, bias=True, seed=0):
    g = torch.Generator().manual_seed(V + seed)
    n = SF.SET_ROWS * copies
    h = torch.randn(n, 128, generator=g).bfloat16().to(DEV)
    w = (torch.randn(V, 128, generator=g) * 0.2).bfloat16().to(DEV)
    b = (torch.randn(V, generator=g) * 0.1).bfloat16().to(DEV) if bias else None
    return h, w, b, SF.labels_for(V, -1, g, copies).to(DEV)


def _score(h, lab, w, b, kind, s, st, **kw):
    return dict(zip(losses.SCORE_KEYS, losses.fused_linear_score(h, lab, w, b, -1, kind, smoothing=s, seq_start=st.to(DEV), **kw)))


def _own_reference(h, lab, w, b, kind, s, st):
    loss_rows, correct_rows, lab_c, hip = losses._score_rows(h, lab, w, b, -1, kind, s, None)
    assert hip
    return SF.reference(st, loss_rows.cpu(), correct_rows.cpu(), lab_c.cpu(), -1)


@pytest.mark.parametrize("kind,s", [(losses.EVAL_CE, 0.1), (losses.EVAL_KL, 0.1)])
def test_loss_rows_are_the_eval_kernels_and_chunking_changes_no_bit(hip_lib, kind, s):
    V = SF.V_PADDED
    h, w, b, lab = _head(V)
    N, ld, st = SF.SET_ROWS, -(-V // 8) * 8, SF.seq_start()
    assert ld != V
    outs = {}
    for chunk in (7, 64, 200, N):
        # the gate's walk, restated: the chunk rounded up to 64 rows (7 -> 64, 200 -> 256), the last chunk the LAST `c` rows
        c = min(-(-chunk // 64) * 64, N)
        starts = list(range(0, N - c, c)) + [N - c]
        hits = losses.EVAL_HITS[0], losses.SCORE_HITS[0]
        outs[chunk] = _score(h, lab, w, b, kind, s, st, chunk=chunk)
        assert (losses.EVAL_HITS[0], losses.SCORE_HITS[0]) == (hits[0] + len(starts), hits[1] + 1), "one launch per chunk, then one"
        loss_rows, correct_rows, _, hip = losses._score_rows(h, lab, w, b, -1, kind, s, chunk)
        assert hip
        buf = torch.empty(c, ld, dtype=torch.bfloat16, device=DEV)
        for c0 in starts:   # the same GEMM call and the kernel on the chunk alone
            torch.addmm(b, h[c0:c0 + c], w.t(), out=buf[:, :V])
            lo = torch.empty(c, dtype=torch.float32, device=DEV)
            co = torch.empty(c, dtype=torch.int32, device=DEV)
            _lib.call("rwkv7_head_eval_bf16", buf, c, V, ld, buf, lab[c0:c0 + c].contiguous(), -1, kind, s, lo, co, None)
            assert torch.equal(loss_rows[c0:c0 + c].view(torch.int32), lo.view(torch.int32)), (chunk, c0)
            assert torch.equal(correct_rows[c0:c0 + c], co), (chunk, c0)
    SF.assert_scores(outs[N], _own_reference(h, lab, w, b, kind, s, st), "one chunk")
    for chunk in (7, 64, 200):
        SF.assert_bit_identical(outs[chunk], outs[N], f"chunk {chunk} against N")
    # 197 rows in chunks of 64: the last chunk would be 5 rows, the size at which the library GEMM rounds differently
    st = torch.tensor([0, 1, 64, 130, 197])
    SF.assert_bit_identical(_score(h[:197], lab[:197], w, b, kind, s, st, chunk=64), _score(h[:197], lab[:197], w, b, kind, s, st),
                            "a 5-row tail")


def test_the_fixture_calls_on_the_hip_route(hip_lib):
    kind, s = losses.EVAL_CE, 0.1
    h, w, b, lab = _head(SF.V_PADDED)
    st = SF.seq_start()
    whole = _score(h, lab, w, b, kind, s, st)
    for i in range(len(SF.LENS)):   # n_seq = 1
        SF.assert_bit_identical(_score(h, lab, w, b, kind, s, st[i:i + 2]), {k: v[i:i + 1] for k, v in whole.items()}, f"sequence {i} alone")
    h, w, b, lab = _head(SF.V_PADDED, copies=SF.COPIES, seed=1)   # 33 copies of the lengths, every row its own
    st = SF.seq_start(SF.COPIES)
    SF.assert_scores(_score(h, lab, w, b, kind, s, st), _own_reference(h, lab, w, b, kind, s, st), "33 copies")
    h, w, b, lab = _head(SF.V_ODD, bias=False)   # the Spark head's width, no bias
    st = SF.seq_start()
    SF.assert_scores(_score(h, lab, w, None, kind, 0.0, st), _own_reference(h, lab, w, None, kind, 0.0, st), "V = 8193")


# ---- one head per layout, the real backbone ----------------------------------------------------------------------------------------------
def _to(batch, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}


def _sums_match(score, metrics):
    """as in test_score.py: exact counts, loss_sum within n 2^-52 |loss_sum| (positive row losses: |loss_sum| is sum|rows|)"""
    assert torch.equal(score["tokens"].sum(-1).reshape(-1), metrics["tokens"])
    assert torch.equal(score["correct"].sum(-1).reshape(-1), metrics["correct"])
    bar = metrics["tokens"] * 2.0 ** -52 * metrics["loss_sum"].abs()
    assert bool(((score["loss_sum"].sum(-1).reshape(-1) - metrics["loss_sum"]).abs() <= bar).all())
    assert bool(((score["worst_row"] >= 0) == (score["tokens"] > 0)).all())


def _spark(seed=3):
    cfg = RWKV7SpeechConfig(vocab_size=257, text_vocab_size=300, audio_global_vocab_size=64, **SMALL)
    return RWKV7ForSpeech(cfg).init_weights(seed=seed).to(DEV).to(torch.bfloat16)


def test_spark_score_padded(hip_lib):
    m = _spark().train()
    batch = L.synthetic_spark_batch(m, 3, 256, seed=5, n_text=31, n_global=8)
    hits = losses.SCORE_HITS[0]
    got = m.score(**batch)
    assert losses.SCORE_HITS[0] == hits + 1 and m.training
    assert all(v.shape == (3,) and v.is_cuda for v in got.values())
    _sums_match(got, m.eval_metrics(**batch))
    assert got["tokens"].tolist() == [256 - 3 - 31 - 8] * 3


def test_spark_score_packed_cu_seqlens(hip_lib):
    m = _spark().train()
    g = torch.Generator().manual_seed(6)
    cu = torch.tensor([0, 70, 103, 103, 231, 236])   # five utterances, one empty
    labels = torch.randint(0, 256, (1, 236), generator=g)
    labels[0, cu[1:] - 1] = -100
    batch = dict(inputs_embeds=(torch.randn(1, 236, 128, generator=g) * 0.5).bfloat16().to(DEV), labels=labels.to(DEV), cu_seqlens=cu.to(DEV))
    hits = losses.SCORE_HITS[0]
    got = m.score(**batch)
    assert losses.SCORE_HITS[0] == hits + 1 and all(v.shape == (5,) for v in got.values())
    _sums_match(got, m.eval_metrics(**batch))
    shifted = torch.cat((labels[0, 1:], torch.tensor([-100])))
    assert got["tokens"].tolist() == [int((shifted[a:b] != -100).sum()) for a, b in zip(cu[:-1].tolist(), cu[1:].tolist())]
    assert got["worst_row"][2] == -1


def test_xy_score(hip_lib):
    cfg = RWKV7XYConfig(vocab_size=120, speech_vocab_size=16, num_channels=4, text_shift_size=100, lsm_weight=0.1, **SMALL)
    m = RWKV7XYLM(cfg).init_weights(seed=2)
    with torch.no_grad():
        for h in m.heads:
            h.bias.normal_(0, 0.1)
    m = m.to(DEV).to(torch.bfloat16).train()
    g = torch.Generator().manual_seed(0)
    text = [[101 + i for i in range(5)], [90, 91, 92]]
    audio = [torch.randint(0, 15, (4, n), generator=g).tolist() for n in (9, 5)]
    batch = _to(L.XYDataProcessor(120, 4, 100, 16).process_batch(text, audio), DEV)
    hits = losses.SCORE_HITS[0]
    got = m.score(**batch)
    assert losses.SCORE_HITS[0] == hits + 4 and m.training and all(v.shape == (4, 2) for v in got.values())
    _sums_match(got, m.eval_metrics(**batch))


def test_cosy_score(hip_lib):
    cfg = RWKV7CosyConfig(vocab_size=200, speech_token_size=50, lsm_weight=0.1, length_normalized_loss=True, **SMALL)
    llm = RWKV7CosyLM(cfg).init_weights(seed=4).to(torch.bfloat16).to(DEV).train()
    batch = _to(L.cosy_collate([[3, 4, 5, 6], [7, 8]], [list(range(10, 20)), [20, 21, 22]], pad_to_max_length=False), DEV)
    hits = losses.SCORE_HITS[0]
    got = llm.score(batch=batch)
    assert losses.SCORE_HITS[0] == hits + 1 and llm.training and got["tokens"].tolist() == [11, 4]
    _sums_match(got, llm.eval_metrics(batch=batch))


# ---- DataParallelTrainer.score on the HIP AdamW path -------------------------------------------------------------------------------------
KW = dict(lr=1e-3, warmup_steps=0, total_steps=10)


def _advance(tr, steps):
    for step in steps:
        tr.step(**L.synthetic_spark_batch(tr.model, 2, 256, seed=100 * step, n_text=31, n_global=8))


def _state(tr):
    torch.cuda.synchronize()
    return dict(param=tr.flat.flat_param.clone(), master=tr.master.clone(), exp_avg=tr.exp_avg.clone(), exp_avg_sq=tr.exp_avg_sq.clone(),
                grad=tr.flat.flat_grad.clone(), nan_flag=tr.nan_flag.clone(), step_idx=tr.step_idx, last_lr=tr.last_lr, lr=tr.current_lr(),
                rng=torch.get_rng_state(), cuda_rng=torch.cuda.get_rng_state(DEV), training=tr.model.training)


def _same(a, b):
    for k, v in a.items():
        assert torch.equal(v, b[k]) if torch.is_tensor(v) else v == b[k], k


@pytest.mark.timeout(120)
def test_three_steps_score_two_steps_equals_five_steps_on_the_hip_path(hip_lib):
    def run(score):
        torch.manual_seed(11)
        m = _spark().train()
        assert m.dropout.p == 0.02
        tr = trainer.DataParallelTrainer(m, **KW)
        assert tr.hip_adamw
        _advance(tr, range(3))
        res = None
        if score:
            shard = [L.synthetic_spark_batch(m, 2, 256, seed=900 + i, n_text=31, n_global=8) for i in range(2)]
            before, digest = _state(tr), tr.digest()
            hits = losses.SCORE_HITS[0]
            res = tr.score(shard)
            assert losses.SCORE_HITS[0] == hits + 2
            _same(before, _state(tr))
            assert tr.digest() == digest and tr.model.training
        _advance(tr, range(3, 5))
        return _state(tr), res

    (a, _), (b, res) = run(False), run(True)
    _same(a, b)
    assert res["tokens"].tolist() == [256 - 3 - 31 - 8] * 4   # two batches of two utterances, every semantic position once
    assert (res["mean_loss"] > 0).all() and (res["worst_loss"] >= res["mean_loss"] * (1 - 1e-6)).all() and (res["worst_row"] >= 0).all()
