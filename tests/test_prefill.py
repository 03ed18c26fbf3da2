"""CPU: the graph-replayed packed prefill's device-free parts -- the two entries are declared, exported and reject bad arguments
before they launch, and prefill.plan (layout, index block, split into replays) on seeded random packs and its edge cases."""
import ctypes
import random

import pytest
import torch

from rwkvtts_amd import _lib, ops
from rwkvtts_amd.prefill import ROW_ZERO, plan

NEW = ("rwkv7_add_ln_mix_rows_fwd_bf16", "rwkv7_wkv_chunk_fwd_state_rows_bf16")
BUCKETS = (256, 512, 1024, 2048, 4096)
C = 32


def test_entries_are_declared_and_exported(hip_lib):
    for name in NEW:
        assert name in _lib.exported_symbols()
        assert hasattr(hip_lib, name)


def test_row_entry_argument_errors_do_not_launch(hip_lib):
    one = ctypes.c_void_p(16)   # never dereferenced: the checks fire first
    f = hip_lib.rwkv7_add_ln_mix_rows_fwd_bf16

    def call(T=64, D=128, nmix=6, x=one, branch=None, gamma=one, params=one, prev_src=one, last_dst=one, x_prev=one, x_out=None, out=one,
             nblocks=4, run_len=4):
        return f(T, D, nmix, x, branch, gamma, None, ctypes.c_float(1e-5), None, params, prev_src, last_dst, None, x_prev, x_out, out,
                 nblocks, run_len, None)

    for kw in (dict(x=None), dict(gamma=None), dict(params=None), dict(prev_src=None), dict(last_dst=None), dict(x_prev=None), dict(out=None),
               dict(T=0), dict(nblocks=0), dict(run_len=0), dict(branch=one)):   # branch without x_out
        assert call(**kw) == -1, kw
    for kw in (dict(nmix=3), dict(nmix=0), dict(nmix=7), dict(T=48), dict(D=100), dict(D=0), dict(D=4160)):
        assert call(**kw) == -4, kw


def test_scan_entry_argument_errors_do_not_launch(hip_lib):
    one = ctypes.c_void_p(16)
    f = hip_lib.rwkv7_wkv_chunk_fwd_state_rows_bf16
    names = ("w", "q", "k", "v", "a", "b", "tinv", "y", "seq_off", "state", "state_row")

    def call(T=64, H=2, nseq=2, **null):
        p = {n: (None if n in null else one) for n in names}
        return f(T, H, p["w"], p["q"], p["k"], p["v"], p["a"], p["b"], p["tinv"], p["y"], p["seq_off"], nseq, p["state"], p["state_row"], None)

    for n in names:
        assert call(**{n: True}) == -1, n
    assert call(T=0) == -1 and call(H=0) == -1 and call(nseq=0) == -1 and call(nseq=-2) == -1
    assert call(T=48) == -4 and call(T=16) == -4


# ------------------------------------------------------------------------------------------------------------------------ plan
def _check(lens, rows, fresh, n_rows=64, max_seqs=8, buckets=BUCKETS):
    reps = plan(lens, rows, fresh, n_rows, max_seqs, buckets)
    seen = [torch.zeros(n, dtype=torch.int32) for n in lens]          # how often every token is placed
    cursor = [0] * len(lens)                                          # pieces of a prompt come in order and concatenate to it
    ended = []
    for rp in reps:
        assert rp.t_al in buckets and rp.keep.shape == (rp.t_al,) and len(rp.pieces) <= max_seqs
        assert rp.seq_off.shape == (max_seqs + 1,) and rp.state_row.shape == (max_seqs,)
        covered = torch.zeros(rp.t_al, dtype=torch.int32)
        so = rp.seq_off.tolist()
        assert so[0] == 0 and so == sorted(so) and so[-1] == rp.t_al // C
        assert so[len(rp.pieces)] == rp.t_al // C                     # the rounding's chunks belong to the last piece: none unowned
        for j, (i, lo, hi, at) in enumerate(rp.pieces):
            n = hi - lo
            assert n >= 1 and lo == cursor[i]
            cursor[i] = hi
            seen[i][lo:hi] += 1
            covered[at:at + n] += 1
            assert (at + n) % C == 0                                  # ends on a chunk boundary
            assert at >= 1 and not bool(rp.keep[at - 1])              # a masked row in front
            assert so[j] * C <= at - 1 and at + n <= so[j + 1] * C    # inside its own chunk range, masked row included
            if hi < lens[i]:
                assert n % C == 0                                     # a split prompt is cut on multiples of 32 tokens
            zero = fresh and lo == 0                                  # only the first piece of a fresh prompt carries the zero marks
            assert int(rp.state_row[j]) == (rows[i] | (ROW_ZERO if zero else 0))
            assert int(rp.prev_src[at]) == (-2 if zero else rows[i])
            assert int(rp.last_dst[at + n - 1]) == rows[i] and int(rp.last_row[j]) == at + n - 1
        assert [s for s in rp.state_row.tolist()[len(rp.pieces):]] == [-1] * (max_seqs - len(rp.pieces))   # unused entries inactive
        assert all(a == b for a, b in zip(so[len(rp.pieces):], so[len(rp.pieces) + 1:]))                     # ... with empty ranges
        assert torch.equal(covered, rp.keep.to(torch.int32)) and int(covered.max()) == 1
        firsts = {at for _, _, _, at in rp.pieces}
        lasts = {at + hi - lo - 1 for _, lo, hi, at in rp.pieces}
        assert set((rp.prev_src != -1).nonzero().flatten().tolist()) == firsts
        assert set((rp.last_dst != -1).nonzero().flatten().tolist()) == lasts
        for m in (rp.prev_src, rp.last_dst):                          # each cache row at most once per field per replay
            named = [r for r in m.tolist() if r >= 0]
            assert len(named) == len(set(named))
        active = [r & ~ROW_ZERO for r in rp.state_row.tolist() if r >= 0]
        assert len(active) == len(set(active))
        ended += [i for i, _ in rp.ends]
        for i, j in rp.ends:
            assert rp.pieces[j][0] == i and rp.pieces[j][2] == lens[i]
        blk = rp.index_block()
        assert blk.dtype == torch.int32 and blk.numel() == 3 * max_seqs + 1 + 3 * rp.t_al
    assert all(int(s.min()) == 1 and int(s.max()) == 1 for s in seen) and cursor == list(lens)   # every token on exactly one row
    assert sorted(ended) == list(range(len(lens)))
    return reps


def _fits_one(lens, max_seqs=8, buckets=BUCKETS):
    return len(lens) <= max_seqs and sum((n // C + 1) * C for n in lens) <= buckets[-1]


def test_plan_random_packs():
    rng = random.Random(0)
    one = 0
    for trial in range(200):
        n = rng.randint(1, 12)
        lens = [rng.choice([1, 2, 31, 32, 33, 64, rng.randint(1, 300), rng.randint(1, 1500)]) for _ in range(n)]
        rows = rng.sample(range(64), n)
        fresh = bool(trial % 2)
        reps = _check(lens, rows, fresh)
        if _fits_one(lens):
            one += 1
            assert len(reps) == 1
            rp = reps[0]
            need = sum((k // C + 1) * C for k in lens)
            assert rp.t_al == min(b for b in BUCKETS if b >= need)    # the smallest bucket that fits
            lay = ops.packed_state_layout(lens, False, align=lambda t: rp.t_al)
            assert lay.t_al == rp.t_al
            assert torch.equal(rp.seq_off[:n + 1], lay.seq_off)
            assert [p[3] for p in rp.pieces] == lay.first.tolist() and rp.last_row[:n].tolist() == lay.last.tolist()
            dest = torch.cat([torch.arange(at, at + hi - lo, dtype=torch.int32) for _, lo, hi, at in rp.pieces])
            assert torch.equal(dest, lay.dest)
        else:
            assert len(reps) > 1
    assert one > 50


@pytest.mark.parametrize("lens", [[1], [32], [64, 1, 96], [255], [4095], [1, 4095 - 32 - 1]])
def test_plan_edges_in_one_replay(lens):
    # a one-token prompt; n % 32 == 0; n = a bucket's capacity exactly (bucket - 1 tokens: one masked row in front)
    for fresh in (True, False):
        reps = _check(lens, list(range(3, 3 + len(lens))), fresh)
        assert len(reps) == 1
    if lens == [255]:
        assert reps[0].t_al == 256
    if lens == [4095]:
        assert reps[0].t_al == 4096
    if lens == [1]:
        rp = reps[0]
        at = rp.pieces[0][3]
        assert at == 31 and int(rp.prev_src[at]) == 3 and int(rp.last_dst[at]) == 3   # reads and writes the same row (fresh=False)


def test_plan_more_prompts_than_max_seqs():
    lens = [5, 40, 7, 100, 1, 64, 33, 9, 12, 77, 3]
    reps = _check(lens, list(range(11)), True, max_seqs=4)
    assert [len(r.pieces) for r in reps] == [4, 4, 3]
    assert [[p[0] for p in r.pieces] for r in reps] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10]]


def test_plan_splits_a_prompt_longer_than_the_largest_bucket():
    n = int(2.5 * 4096)
    for fresh in (True, False):
        reps = _check([n], [9], fresh)
        assert len(reps) == 3 and all(len(r.pieces) == 1 for r in reps)
        cuts = [(p[1], p[2]) for r in reps for p in r.pieces]
        assert cuts[0][0] == 0 and cuts[-1][1] == n and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
        marks = [int(r.state_row[0]) & ROW_ZERO for r in reps]
        assert marks == ([ROW_ZERO, 0, 0] if fresh else [0, 0, 0])
        assert [int(r.prev_src[r.pieces[0][3]]) for r in reps] == ([-2, 9, 9] if fresh else [9, 9, 9])
        assert [len(r.ends) for r in reps] == [0, 0, 1]
    # beside other prompts: its pieces never share a replay
    reps = _check([100, n, 50], [0, 1, 2], True)
    for r in reps:
        assert len({p[0] for p in r.pieces}) == len(r.pieces)


def test_plan_rejects_bad_rows():
    for lens, rows in (([5, 6], [1]), ([5, 6], [1, 1]), ([5, 6], [1, 64]), ([5, 6], [-1, 2]), ([5, 0], [1, 2]), ([], [3])):
        with pytest.raises(ValueError):
            plan(lens, rows, True, 64)
    with pytest.raises(ValueError, match="distinct rows"):
        plan([5, 6], [2, 2], True, 64)
    with pytest.raises(ValueError, match="names 1 rows for 2 sequences"):
        plan([5, 6], [2], True, 64)
