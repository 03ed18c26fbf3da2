"""Graph-replayed stateful prompt prefill straight into chosen rows of a cache.

RWKV7Model(inputs_embeds, cu_seqlens, past_key_values, cache_rows) computes the same thing eagerly: it reads cu_seqlens and cache_rows
on the host, builds the layout there, runs the unfused stages of the differentiable path one torch op at a time, patches every
sequence's first row and stores its last row with gathers and scatters, and gathers / scatters the named cache rows around the call.
That is host and launch time (23.9 ms per admission at 0.4B in profiles/continuous_bench.txt) for well under a millisecond of
arithmetic.  PackedPrefill is the inference path in its own right:

  * two kernels address the cache rows themselves and take their whole layout from device memory: rwkv7_add_ln_mix_rows_fwd_bf16
    (residual add + LayerNorm + token-shift lerps with carried predecessors in and out of x_prev rows, csrc/prefill_rows.hip) and
    rwkv7_wkv_chunk_fwd_state_rows_bf16 (the chunked scan on indexed state rows, in place, csrc/wkv7_chunk_fwd9.hip);
  * so the 24 layers are captured ONCE per size class (bucket = rows of the aligned packed row) as a torch.cuda.CUDAGraph, and a
    prefill is: copy the prompts into the bucket's static input row, one pinned host-to-device copy of the index block, one replay;
  * plan() -- the layout, the index block, the split of an oversized pack into several replays -- is a pure host function.

Nothing on the run() path reads the device back (.tolist() / .item() / .cpu() / synchronize).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib, fused, ops
from .backbone import Cache

C = ops.CHUNK_T
ROW_ZERO = 1 << 30   # RWKV7_STATE_ROW_ZERO (include/rwkv7_hip.h)


@dataclass
class Replay:
    """One replay of one bucket's graph (PackedPrefill.plan).  Sequence entry j of the replay is piece j.
      t_al       the bucket: rows of the aligned packed row
      seq_off    int32 [max_seqs + 1]  chunk ranges; entries past the pieces are empty
      state_row  int32 [max_seqs]      cache row of each piece (| ROW_ZERO: start from zero); -1 = inactive entry
      prev_src / last_dst  int32 [t_al]  the row kernel's maps (include/rwkv7_hip.h)
      keep       bool [t_al]           rows that hold a token
      last_row   int32 [max_seqs]      aligned row of each piece's last token (0 for inactive entries)
      pieces     [(sequence, token lo, token hi, aligned lo)]: tokens [lo, hi) of that prompt sit at aligned rows lo .. lo + hi - lo
      ends       [(sequence, entry j)]: the sequences whose LAST token is in this replay"""
    t_al: int
    seq_off: torch.Tensor
    state_row: torch.Tensor
    prev_src: torch.Tensor
    last_dst: torch.Tensor
    keep: torch.Tensor
    last_row: torch.Tensor
    pieces: List[Tuple[int, int, int, int]] = field(default_factory=list)
    ends: List[Tuple[int, int]] = field(default_factory=list)

    def index_block(self):
        """The replay's device-side indices as ONE int32 row: seq_off | state_row | last_row | prev_src | last_dst | keep."""
        return torch.cat([self.seq_off, self.state_row, self.last_row, self.prev_src, self.last_dst, self.keep.to(torch.int32)])


def plan(lens: Sequence[int], rows: Sequence[int], fresh, n_rows: int, max_seqs: int = 8,
         buckets: Sequence[int] = (256, 512, 1024, 2048, 4096)) -> List[Replay]:
    """The replays that prefill prompts of `lens` tokens into cache rows `rows` (of a cache with n_rows rows).  Pure host function.

    Layout: ops.packed_state_layout(train=False) -- every piece ends on a chunk boundary with 1 .. 32 masked rows in front --
    rounded up to the smallest bucket that fits; the rows the rounding adds are identity chunks of the last piece, the sequence
    entries past the pieces are inactive (state_row = -1, empty chunk range), so no chunk reads uninitialised memory.  Pieces are
    packed first-fit in order; a pack that does not fit the largest bucket or max_seqs becomes several replays.  A prompt longer than
    a bucket holds (largest bucket - 1 tokens) is cut on multiples of 32 tokens into pieces that go to consecutive replays: the later
    pieces continue from the row (prev_src = the row, no zero mark).  fresh=False: the first pieces continue from what the rows hold
    too (a prompt that arrives in parts).  fresh may also be a sequence of bools, one per prompt: sequence i gets the zero mark on its
    first piece only if fresh[i] (a pack that mixes fresh prompts with suffixes of a stored state)."""
    lens, rows = [int(n) for n in lens], [int(r) for r in rows]
    buckets = sorted(int(b) for b in buckets)
    N = len(lens)
    fresh = [bool(fresh)] * N if isinstance(fresh, (bool, int)) else [bool(f) for f in fresh]
    if len(fresh) != N:
        raise ValueError(f"fresh names {len(fresh)} sequences, there are {N}")
    if not buckets or any(b < 2 * C or b % C for b in buckets) or max_seqs < 1:
        raise ValueError(f"buckets must be multiples of {C} >= {2 * C} and max_seqs >= 1, got {buckets}, {max_seqs}")
    if len(rows) != N:
        raise ValueError(f"cache_rows names {len(rows)} rows for {N} sequences")
    if len(set(rows)) != N or any(not 0 <= r < n_rows for r in rows):
        raise ValueError(f"cache_rows must be {N} distinct rows in [0, {n_rows}), got {rows}")
    if any(n < 1 for n in lens):
        raise ValueError(f"every prompt needs at least one token, got lengths {lens}")
    big = buckets[-1]
    alen = lambda n: (n // C + 1) * C
    # pieces in order: (sequence, token lo, token hi)
    todo = []
    for i, n in enumerate(lens):
        lo = 0
        while n - lo > big - 1:          # a piece of big - 32 tokens fills the largest bucket (32 masked rows in front)
            todo.append((i, lo, lo + big - C))
            lo += big - C
        todo.append((i, lo, n))
    groups, cur, used = [], [], 0
    for p in todo:
        a = alen(p[2] - p[1])
        if cur and (used + a > big or len(cur) == max_seqs or any(q[0] == p[0] for q in cur)):
            groups.append(cur)
            cur, used = [], 0
        cur.append(p)
        used += a
    if cur:
        groups.append(cur)
    out = []
    for g in groups:
        need = sum(alen(hi - lo) for _, lo, hi in g)
        t_al = next(b for b in buckets if b >= need)
        lay = ops.packed_state_layout([hi - lo for _, lo, hi in g], False, align=lambda t: t_al)
        seq_off = torch.full((max_seqs + 1,), t_al // C, dtype=torch.int32)
        seq_off[:len(g) + 1] = lay.seq_off
        state_row = torch.full((max_seqs,), -1, dtype=torch.int32)
        last_row = torch.zeros(max_seqs, dtype=torch.int32)
        prev_src = torch.full((t_al,), -1, dtype=torch.int32)
        last_dst = torch.full((t_al,), -1, dtype=torch.int32)
        keep = torch.zeros(t_al, dtype=torch.bool)
        rp = Replay(t_al, seq_off, state_row, prev_src, last_dst, keep, last_row)
        first, last = lay.first.tolist(), lay.last.tolist()
        for j, (i, lo, hi) in enumerate(g):
            zero = fresh[i] and lo == 0
            state_row[j] = rows[i] | (ROW_ZERO if zero else 0)
            prev_src[first[j]] = -2 if zero else rows[i]
            last_dst[last[j]] = rows[i]
            last_row[j] = last[j]
            keep[first[j]:last[j] + 1] = True
            rp.pieces.append((i, lo, hi, first[j]))
            if hi == lens[i]:
                rp.ends.append((i, j))
        out.append(rp)
    return out


def add_ln_mix_rows(x, branch, norm, mask, params, prev_src, last_dst, x_prev_rd, x_prev):
    """rwkv7_add_ln_mix_rows_fwd_bf16 on the current stream: x, branch [T, D] bf16 (branch may be None), mask [T] bf16 or None,
    params [nmix, D], prev_src / last_dst int32 [T] on the device, x_prev (and x_prev_rd, the snapshot carried predecessors are read
    from; None: x_prev itself) [S, D].  Returns (x + branch, out [nmix, T, D])."""
    T, D = x.shape
    nmix = params.shape[0]
    out = torch.empty(nmix, T, D, dtype=x.dtype, device=x.device)
    x1 = torch.empty_like(x) if branch is not None else None
    run = fused._ADD_LN_MIX_RUN   # the row kernel walks runs of rows on the grid of the training-side add + LayerNorm + lerp kernels
    _lib.call("rwkv7_add_ln_mix_rows_fwd_bf16", x, T, D, nmix, x, branch, norm.weight, norm.bias, norm.eps, mask, params, prev_src,
              last_dst, x_prev_rd, x_prev, x1, out, fused._grid(T, run, fused._ADD_LN_MIX_BLOCKS), run)
    return (x if branch is None else x1), out


def wkv_state_rows(state, r, w, k, v, a, b, seq_off, state_row):
    """rwkv7_wkv_chunk_fwd_state_rows_bf16 (after rwkv7_wkv_chunk_prep) on the current stream: r..b bf16 [1, T, H*64] with identity
    steps outside the pieces, seq_off int32 [nseq + 1] and state_row int32 [nseq] on the device, state fp32 [S,H,64,64] updated in
    place.  The caller guarantees distinct active rows in [0, S).  Returns y [1, T, H*64]."""
    _, T, HC = r.shape
    H = HC // 64
    w4, a4, b4 = (t.view(1, T, H, 64) for t in (w, a, b))
    tinv = ops.wkv7_chunk_prep(w4, a4, b4)
    y = torch.empty_like(v)
    _lib.call("rwkv7_wkv_chunk_fwd_state_rows_bf16", r, T, H, w, r, k, v, a, b, tinv, y, seq_off, state_row.numel(), state, state_row)
    return y


def cache_field_table(cache: Cache) -> torch.Tensor:
    """The device table rwkv7_cache_rows_commit_bf16 takes for `cache`: int64 [3 L], per layer the addresses of att_x_prev, att_kv,
    ffn_x_prev.  The cache's tensors must outlive the table; ValueError for fields the entry does not cover."""
    if cache is None or len(cache) == 0:
        raise ValueError("rwkv7_cache_rows_commit_bf16: no per-layer cache")
    S, D = cache[0].att_x_prev.shape
    H = cache[0].att_kv.shape[1]
    ptrs = []
    for st in cache.states:
        for t, dt, shape in ((st.att_x_prev, torch.bfloat16, (S, D)), (st.att_kv, torch.float32, (S, H, 64, 64)), (st.ffn_x_prev, torch.bfloat16, (S, D))):
            if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda or t.data_ptr() % 16:
                raise ValueError(f"rwkv7_cache_rows_commit_bf16: cache field {tuple(t.shape)} / {t.dtype}: expected a contiguous, 16-byte "
                                 f"aligned {dt} {shape} on the HIP device")
            ptrs.append(t.data_ptr())
    return torch.tensor(ptrs, dtype=torch.int64).to(cache[0].att_kv.device)


def check_commit_rows(src_row: Sequence[int], dst_row: Sequence[int], src_rows: int, dst_rows: int):
    """Host check of the row lists before they go to the device (the kernel does not check them): as many sources as destinations,
    active sources in [0, src_rows), active destinations distinct and in [0, dst_rows); a negative destination marks a skipped entry."""
    src_row, dst_row = [int(r) for r in src_row], [int(r) for r in dst_row]
    if len(src_row) != len(dst_row):
        raise ValueError(f"{len(src_row)} source rows for {len(dst_row)} destination rows")
    act = [(s, d) for s, d in zip(src_row, dst_row) if d >= 0]
    if any(not 0 <= s < src_rows for s, _ in act) or any(d >= dst_rows for _, d in act) or len({d for _, d in act}) != len(act):
        raise ValueError(f"rows {src_row} -> {dst_row}: sources must lie in [0, {src_rows}), destinations distinct in [0, {dst_rows})")
    return src_row, dst_row


def cache_rows_commit(src_tbl, dst_tbl, src_row, dst_row, n: int, layers: int, D: int, H: int):
    """rwkv7_cache_rows_commit_bf16 on the current stream: src_tbl / dst_tbl from cache_field_table, src_row / dst_row int32 device
    tensors of at least n entries whose values the caller has checked (check_commit_rows)."""
    for t in (src_row, dst_row):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.is_cuda and t.numel() >= n
    assert src_tbl.dtype == torch.int64 and dst_tbl.dtype == torch.int64 and src_tbl.numel() == dst_tbl.numel() == 3 * layers
    _lib.call("rwkv7_cache_rows_commit_bf16", dst_tbl, int(layers), int(n), src_tbl, dst_tbl, src_row, dst_row, int(D), int(H))


SEED_ZERO = -1   # RWKV7_SEED_ZERO (include/rwkv7_hip.h)


def check_seed_rows(src_row: Sequence[int], dst_row: Sequence[int], src_rows: int, dst_rows: int):
    """check_commit_rows for rwkv7_cache_rows_seed_bf16: an entry is active with a destination >= 0 and a source >= SEED_ZERO (a
    source below it skips the entry, as a negative destination does); an active source is SEED_ZERO or a row in [0, src_rows)."""
    src_row, dst_row = [int(r) for r in src_row], [int(r) for r in dst_row]
    if len(src_row) != len(dst_row):
        raise ValueError(f"{len(src_row)} source rows for {len(dst_row)} destination rows")
    act = [(s, d) for s, d in zip(src_row, dst_row) if d >= 0 and s >= SEED_ZERO]
    if any(s >= src_rows for s, _ in act) or any(d >= dst_rows for _, d in act) or len({d for _, d in act}) != len(act):
        raise ValueError(f"rows {src_row} -> {dst_row}: sources must be {SEED_ZERO} (zero) or lie in [0, {src_rows}), destinations "
                         f"distinct in [0, {dst_rows})")
    return src_row, dst_row


def cache_rows_seed(src_tbl, dst_tbl, src_row, dst_row, n: int, layers: int, D: int, H: int):
    """rwkv7_cache_rows_seed_bf16 on the current stream: cache_rows_commit's arguments; an entry whose source row is SEED_ZERO writes
    zeros to its destination row, one whose source row is below that is skipped.  The caller has checked the values (check_seed_rows)."""
    for t in (src_row, dst_row):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.is_cuda and t.numel() >= n
    assert src_tbl.dtype == torch.int64 and dst_tbl.dtype == torch.int64 and src_tbl.numel() == dst_tbl.numel() == 3 * layers
    _lib.call("rwkv7_cache_rows_seed_bf16", dst_tbl, int(layers), int(n), src_tbl, dst_tbl, src_row, dst_row, int(D), int(H))


def check_retain_rows(rows: Sequence[int], capacity: int) -> List[int]:
    """Host check of the per-slot destination rows of rwkv7_cache_rows_retain_bf16 before they go to the device (the kernel does not
    check them): a negative entry names no row; the others lie in [0, capacity) -- inside the store -- and are distinct."""
    rows = [int(r) for r in rows]
    act = [r for r in rows if r >= 0]
    if any(r >= capacity for r in act) or len(set(act)) != len(act):
        raise ValueError(f"retain rows {rows}: the non-negative entries must be distinct rows in [0, {capacity})")
    return rows


def cache_rows_retain(src_tbl, dst_tbl, live, armed, retain_row, ticket, layers: int, D: int, H: int):
    """rwkv7_cache_rows_retain_bf16 on the current stream, one entry per slot (live.numel() slots): src_tbl / dst_tbl from
    cache_field_table (the engine's cache of at least that many rows, the store's cache), live / armed uint8 and retain_row / ticket
    int32 device tensors of one entry per slot; ticket is zero between launches, and the values of retain_row are the caller's
    guarantee (check_retain_rows)."""
    slots = live.numel()
    for t, dt in ((live, torch.uint8), (armed, torch.uint8), (retain_row, torch.int32), (ticket, torch.int32)):
        assert t.dtype == dt and t.is_contiguous() and t.is_cuda and t.numel() == slots
    assert src_tbl.dtype == torch.int64 and dst_tbl.dtype == torch.int64 and src_tbl.numel() == dst_tbl.numel() == 3 * layers
    _lib.call("rwkv7_cache_rows_retain_bf16", dst_tbl, int(layers), slots, src_tbl, dst_tbl, live, armed, retain_row, ticket, int(D), int(H))


class _Bucket:
    def __init__(self, t_al, max_seqs, D, dev):
        self.t_al = t_al
        self.x_in = torch.zeros(t_al, D, dtype=torch.bfloat16, device=dev)
        self.idx = torch.full((3 * max_seqs + 1 + 3 * t_al,), -1, dtype=torch.int32, device=dev)
        o = max_seqs + 1
        self.seq_off, self.state_row, self.last_row = self.idx[:o], self.idx[o:o + max_seqs], self.idx[o + max_seqs:o + 2 * max_seqs]
        o += 2 * max_seqs
        self.prev_src, self.last_dst, self.keep = self.idx[o:o + t_al], self.idx[o + t_al:o + 2 * t_al], self.idx[o + 2 * t_al:]
        self.h_last = torch.zeros(max_seqs, D, dtype=torch.bfloat16, device=dev)
        self.high = 0        # rows of x_in the last use wrote (high-water mark)
        self.graph = None


class PackedPrefill:
    """pp = PackedPrefill(backbone, cache); h_last = pp.run(prompts, rows, fresh=True)

    backbone: a bf16 RWKV7Model on the HIP device, in eval mode; cache: a plain (non-differentiable) bf16 Cache whose tensors the graphs
    are captured on -- their addresses never change.  run leaves in `cache` and returns at the last positions what
    RWKV7Model(inputs_embeds=cat(prompts), cu_seqlens, past_key_values=cache, cache_rows=rows) leaves and returns (with fresh=True:
    after zeroing the named rows); rows not named stay bit for bit.  One graph per bucket, captured on first use (warm() captures
    ahead of time: a capture synchronises), all in one memory pool.  The model's weights are captured by address; the stacked lerp
    coefficients are copies made at construction."""

    def __init__(self, backbone, cache: Cache, max_seqs: int = 8, buckets: Sequence[int] = (256, 512, 1024, 2048, 4096)):
        p = next(backbone.parameters())
        if p.dtype != torch.bfloat16 or not p.is_cuda:
            raise ValueError("PackedPrefill needs a bf16 model on the HIP device (the stateful packed scan is bf16 only)")
        if cache is None or len(cache) != len(backbone.layers) or cache.requires_grad:
            raise ValueError("PackedPrefill updates a plain cache of the model's depth in place: a differentiable cache is not supported")
        if cache[0].att_x_prev.dtype != torch.bfloat16 or not all(t.is_contiguous() for s in cache.states for t in (s.att_x_prev, s.att_kv, s.ffn_x_prev)):
            raise ValueError("PackedPrefill needs contiguous bf16 token-shift rows in the cache")
        plan([1], [0], True, 1, max_seqs, buckets)   # validates buckets / max_seqs
        self.model, self.cache, self.max_seqs, self.buckets = backbone.eval(), cache, int(max_seqs), tuple(sorted(int(b) for b in buckets))
        self.dev, self.D, self.n_rows = p.device, backbone.config.hidden_size, cache[0].att_kv.shape[0]
        with torch.no_grad():
            self._mix6 = [torch.cat([q.detach().reshape(1, -1) for q in l.attn.mix_params()], 0).to(torch.bfloat16).contiguous()
                          for l in backbone.layers]
            self._mix1 = [l.ffn.x_k.detach().reshape(1, -1).to(torch.bfloat16).contiguous() for l in backbone.layers]
        # snapshots of the token-shift rows, taken at the head of every replay: the row kernel reads carried predecessors from them while
        # it writes the new ones into the cache (the first and the last row of a piece are different workgroups)
        self._xp = [t for s in cache.states for t in (s.att_x_prev, s.ffn_x_prev)]
        self._snap = [torch.empty_like(t) for t in self._xp]
        self._b = {}
        self._pool = None

    # ---- host side -----------------------------------------------------------------------------------------------------------------
    def plan(self, lens, rows, fresh=True) -> List[Replay]:
        return plan(lens, rows, fresh, self.n_rows, self.max_seqs, self.buckets)

    @torch.no_grad()
    def warm(self, buckets: Optional[Sequence[int]] = None):
        """Capture the graphs of `buckets` (default: all) now.  The cache is not touched: the warm-up pass runs with every entry inactive."""
        for b in (self.buckets if buckets is None else buckets):
            self._bucket(int(b))
        return self

    @torch.no_grad()
    def run(self, prompts: Sequence[torch.Tensor], rows: Sequence[int], fresh=True) -> torch.Tensor:
        """prompts: [n_i, D] bf16 embeddings on the device; rows: their cache rows (host ints); fresh: a bool, or one bool per prompt
        (False: the prompt continues from what its row holds).  Returns h_last [len(prompts), D]: the final-norm output at every prompt's last token.  Per replay: the bucket's static input row is zeroed up to the high-water
        mark its previous use left (a per-bucket high-water mark, not a full clear), the pieces are copied into their aligned ranges,
        the index block goes over in one pinned host-to-device copy, and the graph is replayed.  No device read-back anywhere."""
        rows = [int(r) for r in rows]
        for e in prompts:
            if e.dim() != 2 or e.shape[1] != self.D or e.dtype != torch.bfloat16 or e.device != self.dev:
                raise ValueError(f"prompt of shape {tuple(e.shape)} / {e.dtype}: expected bf16 [n, {self.D}] on {self.dev}")
        replays = self.plan([e.shape[0] for e in prompts], rows, fresh)
        out = torch.empty(len(prompts), self.D, dtype=torch.bfloat16, device=self.dev)
        for rp in replays:
            b = self._bucket(rp.t_al)
            if b.high:
                b.x_in[:b.high].zero_()
            for i, lo, hi, at in rp.pieces:
                b.x_in[at:at + hi - lo].copy_(prompts[i][lo:hi])
            b.high = max(at + hi - lo for _, lo, hi, at in rp.pieces)
            b.idx.copy_(rp.index_block().pin_memory(), non_blocking=True)
            b.graph.replay()
            # the finished sequences' rows, in runs of consecutive (sequence, entry) pairs: usually one copy
            k = 0
            while k < len(rp.ends):
                i, j = rp.ends[k]
                n = 1
                while k + n < len(rp.ends) and rp.ends[k + n] == (i + n, j + n):
                    n += 1
                out[i:i + n].copy_(b.h_last[j:j + n])
                k += n
        self.cache.seen_tokens += sum(e.shape[0] for e in prompts)
        return out

    # ---- device side ---------------------------------------------------------------------------------------------------------------
    def _bucket(self, t_al) -> _Bucket:
        b = self._b.get(t_al)
        if b is not None:
            return b
        if t_al not in self.buckets:
            raise ValueError(f"{t_al} is not one of the buckets {self.buckets}")
        b = _Bucket(t_al, self.max_seqs, self.D, self.dev)
        # warm-up: every entry inactive (state_row = -1), no row carried or stored (prev_src = last_dst = -1): the cache stays as it is
        b.seq_off.fill_(t_al // C)
        b.last_row.zero_()
        b.keep.zero_()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._forward(b)
        torch.cuda.current_stream().wait_stream(side)
        if self._pool is None:
            self._pool = torch.cuda.graph_pool_handle()
        b.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(b.graph, pool=self._pool):
            self._forward(b)
        self._b[t_al] = b
        return b

    def _forward(self, b: _Bucket):
        m, T, D = self.model, b.t_al, self.D
        H = m.config.num_heads
        keep = b.keep != 0
        mask = keep.to(torch.bfloat16)                 # [T]: the row kernel's and tmix_prepare's mask
        mask3, pad3 = mask.view(1, T, 1), (~keep).view(1, T, 1)
        torch._foreach_copy_(self._snap, self._xp)
        x, delta, v_first = b.x_in, None, None
        for i, layer in enumerate(m.layers):
            st, at = self.cache[i], layer.attn
            if i == 0:
                x = fused.layer_norm(x, layer.pre_norm)
            x, mx = add_ln_mix_rows(x, delta, layer.attn_norm, mask, self._mix6[i], b.prev_src, b.last_dst, self._snap[2 * i], st.att_x_prev)
            xr, xw, xk, xv, xa, xg = (mx[j].unsqueeze(0) for j in range(6))
            r = at.r_proj(xr) * mask3
            k = at.k_proj(xk)
            v = at.v_proj(xv)
            w_pre, a_pre, g = at.w_lora(xw), at.a_lora(xa), at.g_lora(xg)
            v_pre = None if i == 0 else at.v_lora(xv)
            if i == 0:
                v = v * mask3
                v_first = v
            w, k2, v2, a_in, b_in = fused.tmix_prepare(w_pre, k, v, a_pre, v_pre, v_first, at.k_k, at.k_a, mask3, H, i == 0)
            w.masked_fill_(pad3, ops.W_PAD)            # masked rows: exact identity steps of the scan
            y = wkv_state_rows(st.att_kv, r, w, k2, v2, a_in, b_in, b.seq_off, b.state_row)
            y = fused.tmix_post(y, r, k2, v2, g, at.g_norm.weight, at.g_norm.bias, at.r_k, H, at.g_norm.eps)
            att = at.o_proj(y)[0]
            x, mx = add_ln_mix_rows(x, att, layer.ffn_norm, mask, self._mix1[i], b.prev_src, b.last_dst, self._snap[2 * i + 1], st.ffn_x_prev)
            delta = layer.ffn.forward_mixed(mx[0].unsqueeze(0))[0]
        h = fused.add_layer_norm(x, delta, m.norm)[1]
        b.h_last.copy_(h.index_select(0, b.last_row.long()))
