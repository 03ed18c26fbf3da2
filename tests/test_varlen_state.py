"""Packed rows that carry one recurrent state per sequence, host side: the two C entry points (declared, exported, argument checks
that fire before any launch) and the invariants of the chunk-aligned layout (ops.packed_state_layout) the op and the model build."""
import ctypes
import random

import pytest

from rwkvtts_amd import _lib, ops
from rwkvtts_amd.backbone import _row_align

NEW = ("rwkv7_wkv_chunk_fwd_state_seq_bf16", "rwkv7_wkv_chunk_bseq_state_seq_bf16")


def test_state_seq_entry_points_declared_and_exported(hip_lib):
    declared = _lib.exported_symbols()
    for n in NEW:
        assert n in declared, f"{n} not declared in include/rwkv7_hip.h"
        assert hasattr(hip_lib, n), f"{n} not exported"


def test_state_seq_entry_points_reject_bad_arguments_without_launching(hip_lib):
    one = ctypes.c_void_p(16)   # never dereferenced: the checks fire first
    fwd, bseq = hip_lib.rwkv7_wkv_chunk_fwd_state_seq_bf16, hip_lib.rwkv7_wkv_chunk_bseq_state_seq_bf16
    # fwd: B T H, w q k v a b tinv y, sa hs, seq_chunk_off nseq, h0 hT, stream
    # bseq: B T H, w q a b dy tinv e_vk, z, seq_chunk_off nseq, dhT dh0, stream
    # NULL seq_chunk_off with nseq > 0, and a seq_chunk_off with nseq <= 0 -> RWKV7_EINVAL
    assert fwd(1, 32, 1, *([one] * 8), None, None, None, 2, None, None, None) == -1
    assert fwd(1, 32, 1, *([one] * 8), None, None, one, 0, None, None, None) == -1
    assert bseq(1, 32, 1, *([one] * 7), None, None, 3, None, None, None) == -1
    assert bseq(1, 32, 1, *([one] * 7), None, one, -1, None, None, None) == -1
    # T % 32 != 0 -> RWKV7_ECHUNK
    assert fwd(1, 48, 1, *([one] * 8), None, None, one, 2, one, one, None) == -2
    assert bseq(1, 33, 1, *([one] * 7), None, one, 2, one, one, None) == -2
    # null operands -> RWKV7_EINVAL
    assert fwd(1, 32, 1, None, *([one] * 7), None, None, one, 2, None, None, None) == -1
    assert bseq(1, 32, 1, *([one] * 5), None, one, None, one, 2, None, None, None) == -1      # tinv
    assert bseq(1, 32, 1, *([one] * 6), None, None, one, 2, None, None, None) == -1           # e_vk
    # sa without hs ; non-positive sizes -> RWKV7_EINVAL
    assert fwd(1, 32, 1, *([one] * 8), one, None, one, 2, None, None, None) == -1
    for B, T, H in ((0, 32, 1), (1, 0, 1), (1, 32, 0), (-1, 32, 1)):
        assert fwd(B, T, H, *([one] * 8), None, None, one, 2, one, one, None) == -1
        assert bseq(B, T, H, *([one] * 7), None, one, 2, one, one, None) == -1


def _check_layout(lens, train, align):
    C = ops.CHUNK_T
    lay = ops.packed_state_layout(lens, train, align=align)
    N = len(lens)
    dest, seq_off, first, last = lay.dest.tolist(), lay.seq_off.tolist(), lay.first.tolist(), lay.last.tolist()
    assert len(dest) == sum(lens) and len(seq_off) == N + 1 and len(first) == N and len(last) == N
    if sum(lens) == 0:
        assert lay.t_al == 0 and all(f == -1 for f in first) and all(s == 0 for s in seq_off)
        return lay
    assert lay.t_al % C == 0 and seq_off[0] == 0 and seq_off[-1] * C == lay.t_al
    if align is not None:
        assert align(lay.t_al) == lay.t_al
    assert all(a <= b for a, b in zip(seq_off[:-1], seq_off[1:]))
    assert len(set(dest)) == len(dest) and all(0 <= d < lay.t_al for d in dest)   # injective, inside the row
    owned = set(dest)
    pos = 0
    raw = 0
    for i, n in enumerate(lens):
        lo, hi = seq_off[i] * C, seq_off[i + 1] * C
        if n == 0:
            assert first[i] == last[i] == -1 and lo == hi, (i, lens)
            continue
        rows = dest[pos:pos + n]
        pos += n
        assert rows == list(range(first[i], first[i] + n)) and last[i] == first[i] + n - 1   # contiguous, in order
        assert (last[i] + 1) % C == 0, "a sequence ends on a chunk boundary"
        assert first[i] - 1 >= lo and first[i] - 1 not in owned, "a masked row in front of every sequence, inside its range"
        lead = C if (train and i == next(j for j, m in enumerate(lens) if m)) else 0   # training: one identity chunk leads the row
        assert first[i] - lo <= C + lead, "at most one chunk of front padding"
        tail = last[i] + 1 + (C if train else 0)
        assert tail <= hi, "the trailing identity chunk (training) lies inside the sequence's range"
        assert not owned.intersection(range(last[i] + 1, hi)), "nothing but identity rows behind the last token"
        raw = max(raw, tail)
    # the rows the rounding added belong to the last non-empty sequence; no more than one chunk of padding per sequence otherwise
    assert raw <= sum(lens) + sum((C if n else 0) + (C if (train and n) else 0) for n in lens) + (C if train else 0)
    assert lay.t_al == (align(raw) if align is not None else raw)
    return lay


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("align", [None, _row_align])
def test_packed_state_layout_invariants_for_random_lengths(train, align):
    rng = random.Random(5 + train)
    cases = [[0], [1], [32], [33], [0, 0, 0], [31, 32, 33, 0, 64], [1, 17, 32, 33, 100, 0, 256], [0, 5, 0], [2047, 1, 0]]
    for _ in range(60):
        n = rng.randint(1, 12)
        cases.append([rng.choice([0, 0, 32, 64, rng.randint(1, 300), rng.randint(1, 3000)]) for _ in range(n)])
    for lens in cases:
        _check_layout(lens, train, align)


def test_packed_state_layout_known_rows():
    lay = ops.packed_state_layout([1, 0, 32, 33], train=False)
    assert lay.first.tolist() == [31, -1, 64, 127] and lay.last.tolist() == [31, -1, 95, 159]
    assert lay.seq_off.tolist() == [0, 1, 1, 3, 5] and lay.t_al == 160
    lay = ops.packed_state_layout([1, 0, 32, 33], train=True)
    assert lay.first.tolist() == [63, -1, 128, 223] and lay.seq_off.tolist() == [0, 3, 3, 6, 9] and lay.t_al == 288
    lay = ops.packed_state_layout([0, 0, 5], train=True)   # empty sequences in front own empty ranges at chunk 0
    assert lay.first.tolist() == [-1, -1, 59] and lay.seq_off.tolist() == [0, 0, 0, 3]
    # rounding: the added chunks go to the last non-empty sequence; the empty sequence behind it keeps an empty range at the end
    lay = ops.packed_state_layout([40, 2000, 0], train=False, align=_row_align)
    assert lay.t_al == 2304 and lay.seq_off.tolist() == [0, 2, 72, 72]
    with pytest.raises(ValueError):
        ops.packed_state_layout([3, -1], train=False)
