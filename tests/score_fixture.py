"""The sequences that test_score.py and test_score_gpu.py both score, and the per-sequence reference they compare against.

One SET is eight sequences laid back to back: lengths 1, 63, 64, 65, 257, 1025 (one row; one short of, exactly, and one past a wave;
one past the 256-thread workgroup; four strides and one row), one EMPTY range, and one sequence whose labels are all ignore_index.
A set is scored with n_seq = 1 (every sequence on its own, seq_start = [lo, hi] into the same rows) and as COPIES = 33 sets in one
call (264 sequences).

The reference is written from the definitions in include/rwkv7_hip.h, sequence by sequence on the CPU: counts, maximum and first
argmax are exact; the fp64 sum is taken in row order.  Any two fp64 summation orders of the same n terms differ by at most
(n - 1) 2^-52 sum|x| (each is within (n - 1) 2^-53 sum|x| of the exact sum), hence the bar n 2^-52 sum|x| -- derived, not tuned."""
import torch

LENS = (1, 63, 0, 64, 65, 40, 257, 1025)   # 0: the empty range
ALL_IGNORED = 5                            # the 40-row sequence: every label is ignore_index
SET_ROWS = sum(LENS)
COPIES = 33
V_PADDED, V_ODD = 6562, 8193               # 6562 % 8 = 2: the rows of logits are padded to ld = 6568


def seq_start(copies=1):
    lens = torch.tensor(LENS * copies, dtype=torch.int64)
    return torch.cat((torch.zeros(1, dtype=torch.int64), lens.cumsum(0)))


def labels_for(V, ignore, g, copies=1):
    """int64 [copies * SET_ROWS]: random classes, about a tenth ignored, the ALL_IGNORED sequence of every copy ignored entirely;
    the one-row sequence and the last row of every sequence stay valid."""
    n = SET_ROWS * copies
    lab = torch.randint(0, V, (n,), generator=g)
    lab[torch.rand(n, generator=g) < 0.1] = ignore
    st = seq_start(copies).tolist()
    for s in range(len(st) - 1):
        if st[s + 1] > st[s]:
            lab[st[s + 1] - 1] = int(torch.randint(0, V, (1,), generator=g))
        if s % len(LENS) == ALL_IGNORED:
            lab[st[s]:st[s + 1]] = ignore
    return lab


def reference(st, loss_rows, correct_rows, labels, ignore):
    """CPU tensors in -> dict of per-sequence CPU tensors: loss_sum (fp64, row order), tokens, correct, worst_loss (the maximum of the
    fp32 row losses, bits kept), worst_row (its first index relative to the sequence's start) and bar (tokens 2^-52 sum|loss_rows|)."""
    st, lab = st.tolist(), labels.tolist()
    n_seq = len(st) - 1
    out = dict(loss_sum=torch.zeros(n_seq, dtype=torch.float64), tokens=torch.zeros(n_seq, dtype=torch.int64),
               correct=torch.zeros(n_seq, dtype=torch.int64), worst_loss=torch.zeros(n_seq, dtype=torch.float32),
               worst_row=torch.full((n_seq,), -1, dtype=torch.int64), bar=torch.zeros(n_seq, dtype=torch.float64))
    for s in range(n_seq):
        lo, hi = st[s], st[s + 1]
        rows = [r for r in range(lo, hi) if lab[r] != ignore]
        if not rows:
            continue
        x = loss_rows[rows]
        assert x.dtype == torch.float32
        out["loss_sum"][s] = x.double().cumsum(0)[-1]
        out["tokens"][s] = len(rows)
        out["correct"][s] = int(correct_rows[rows].sum())
        out["worst_loss"][s] = x.max()
        out["worst_row"][s] = rows[int((x == x.max()).nonzero()[0])] - lo
        out["bar"][s] = len(rows) * 2.0 ** -52 * x.double().abs().sum()
    return out


def assert_scores(got, want, tag=""):
    """got: the five tensors (any device) as a dict; want: reference().  Counts, worst_loss (bit for bit) and worst_row exact, loss_sum
    within the bar."""
    got = {k: v.cpu() for k, v in got.items()}
    assert got["loss_sum"].dtype == torch.float64 and got["worst_loss"].dtype == torch.float32, tag
    assert got["tokens"].dtype == got["correct"].dtype == got["worst_row"].dtype == torch.int64, tag
    for k in ("tokens", "correct", "worst_row"):
        assert torch.equal(got[k], want[k]), f"{tag}: {k}"
    assert torch.equal(got["worst_loss"].view(torch.int32), want["worst_loss"].view(torch.int32)), f"{tag}: worst_loss bits"
    err = (got["loss_sum"] - want["loss_sum"]).abs()
    assert bool((err <= want["bar"]).all()), f"{tag}: loss_sum off by {err.max().item()} (bar {want['bar'].max().item()})"


def assert_bit_identical(a, b, tag=""):
    for k in a:
        x, y = a[k].cpu(), b[k].cpu()
        assert x.dtype == y.dtype and torch.equal(x.view(torch.int64 if x.element_size() == 8 else torch.int32),
                                                  y.view(torch.int64 if y.element_size() == 8 else torch.int32)), f"{tag}: {k}"
