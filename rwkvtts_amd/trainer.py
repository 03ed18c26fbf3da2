"""Batch-sharded data-parallel training step: one process per GPU, RCCL over xGMI.

What it replaces in the reference: the DeepSpeed engine of train_scripts/train_spark_rwkv7speech.py:483-516,
566-572 (ZeRO-2, bf16 grads, reduce bucket 5e6 elements, overlap_comm False) and its step semantics
(:621-691): forward -> NaN flag all_reduce(MAX) (:664-670) -> backward -> gradient reduction -> AdamW
(betas .9/.95, eps 1e-18, weight_decay 0, :178-197) with the linear warmup/decay schedule (:219-232).

MI355X-first choices:
  * the model is replicated (0.4B: 0.8 GB bf16 + 4.8 GB fp32 master/Adam; 1.5B: ~27 GB) -- 288 GB of HBM
    per GPU makes ZeRO sharding/offload pointless at these sizes;
  * parameters and gradients live in two flat bf16 buffers; gradients are all-reduced (AVG) in buckets of
    ~32 MiB fired from post-accumulate-grad hooks in backward order, asynchronously on RCCL's stream, so
    the exchange overlaps the rest of backward; xGMI is point-to-point (7 links/GPU), so few large
    buckets beat DeepSpeed's 10 MB ones;
  * fp32 master weights + fused AdamW on one flat tensor, then one bf16 copy back.
"""
from __future__ import annotations

import json
import math
import os
import shutil
import threading
import warnings
from typing import List, Optional

import torch
import torch.distributed as dist

from . import _lib, digest as _digest

FLUSH_EVERY = int(os.environ.get("RWKV7_FLUSH_EVERY", "48"))   # adopted gradients per in-backward flush (0: one flush at the end)


def init_distributed(backend: Optional[str] = None):
    """Reads RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* (torch.distributed.run contract).  Returns
    (rank, local_rank, world).  No-op for world size 1."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        if backend is None:
            backend = "nccl" if torch.cuda.is_available() else "gloo"  # "nccl" IS RCCL on ROCm
        if backend == "nccl":
            torch.cuda.set_device(local_rank)
            dist.init_process_group(backend, rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    return rank, local_rank, world


class FlatBuffers:
    """Re-homes every parameter (and its .grad) of `model` into two contiguous buffers.

    Gradients reach the flat buffer without an accumulate pass: before backward every .grad is None, so autograd ADOPTS the
    tensor a backward node returns instead of adding it to a zeroed buffer; a post-accumulate hook then copies it into the
    parameter's slice -- unless the node already wrote there (`param._grad_slot`, used by fused._Linear's split weight
    gradient: 14 matrices per layer arrive with no extra launch at all) -- and re-attaches the slice as .grad.  Slices of
    parameters that received no gradient in a pass are zeroed by `finish_backward()`."""

    def __init__(self, model: torch.nn.Module):
        params = [p for p in model.parameters() if p.requires_grad]
        assert params, "no trainable parameters"
        dt, dev = params[0].dtype, params[0].device
        assert all(p.dtype == dt for p in params), "mixed parameter dtypes"
        self.params = params
        self.offsets, n = [], 0
        for p in params:
            self.offsets.append(n)
            n += (p.numel() + 127) // 128 * 128  # 256-B aligned slices
        self.numel = n
        self.flat_param = torch.zeros(n, dtype=dt, device=dev)
        self.flat_grad = torch.zeros(n, dtype=dt, device=dev)
        self.views = []
        self.fired = [False] * len(params)
        self.to_copy = []
        self.on_ready = None   # callable(i): parameter i's slice is final (BucketedAllReduce)
        for i, (p, o) in enumerate(zip(params, self.offsets)):
            self.flat_param[o:o + p.numel()].copy_(p.data.reshape(-1))
            p.data = self.flat_param[o:o + p.numel()].view_as(p)
            v = self.flat_grad[o:o + p.numel()].view_as(p)
            self.views.append(v)
            p.grad = v
            p._grad_slot = v
            p._grad_slot_used = True   # armed by zero_grad()
            p.register_post_accumulate_grad_hook(self._make_hook(i))

    def _make_hook(self, i):
        def hook(param):
            g = param.grad
            if g is not None and g.data_ptr() != self.views[i].data_ptr():
                self.to_copy.append(i)   # moved into its slice by flush(): one multi-tensor copy for many parameters
                # ... in batches WHILE backward runs: left to the end, the ~500 small gradients of a 24-layer model are one burst of
                # host work (list building + multi-tensor launches, 1.4 ms) behind the last backward kernel, with the GPU idle
                # (profiles/r05k_step_busy.txt); a batch flushed from a hook is host work under the layers still queued
                if len(self.to_copy) >= FLUSH_EVERY > 0:
                    self.flush()
            self.fired[i] = True
            if self.on_ready is not None:
                self.on_ready(i)
        return hook

    def flush(self):
        """Copy the adopted gradients collected so far into their slices (one multi-tensor launch) and attach the slices."""
        if self.to_copy:
            # INVARIANT: every gradient in to_copy was produced on the CURRENT stream.  Weight gradients computed on the side stream
            # (fused.WGRAD_SIDE_STREAM) are written straight into their slice (param._grad_slot) and never come through here; a future
            # fused node that hands a side-stream tensor back as .grad must call fused.wgrad_side_sync() before this copy.
            src = [self.params[i].grad for i in self.to_copy]
            dst = [self.views[i] for i in self.to_copy]
            if src[0].is_cuda and all(s.dtype == d.dtype for s, d in zip(src, dst)):
                torch._foreach_copy_(dst, src)
            else:
                for d, s_ in zip(dst, src):
                    d.copy_(s_)
            for i in self.to_copy:
                self.params[i].grad = self.views[i]
            self.to_copy = []

    def zero_grad(self):
        """Plain mode: zero the buffer and attach the slices as .grad; backward then accumulates into them."""
        self.flat_grad.zero_()
        for i, p in enumerate(self.params):
            p.grad = self.views[i]
            p._grad_slot_used = True
            self.fired[i] = False

    def arm(self):
        """Fast mode (DataParallelTrainer.step): nothing is zeroed, the next backward pass overwrites the slices;
        finish_backward() must follow it."""
        for i, p in enumerate(self.params):
            p.grad = None
            p._grad_slot_used = False
            self.fired[i] = False

    def finish_backward(self, reattach=True):
        """After backward: zero the slices that received nothing, re-attach every .grad.
        reattach=False (DataParallelTrainer.step): only what the GPU needs -- the flush and the zeroing -- so that the optimizer can be
        launched at once; the ~800 attribute writes of `reattach()` (about 1 ms of host time during which the GPU sat idle between
        the last backward kernel and AdamW, profiles/r05i_step_busy.txt) run behind that launch."""
        from . import fused
        fused.wgrad_side_sync()   # weight gradients queued on the side stream land before anything reads the buffer
        self.flush()
        for i in range(len(self.params)):
            if not self.fired[i]:
                self.views[i].zero_()
        if reattach:
            self.reattach()

    def reattach(self):
        for i, p in enumerate(self.params):
            p.grad = self.views[i]
            p._grad_slot_used = True


class BucketedAllReduce:
    """Gradient all-reduce in buckets, launched from backward hooks as soon as a bucket is complete."""

    def __init__(self, flat: FlatBuffers, bucket_bytes: int = 32 << 20, group=None, force: bool = False, shard: bool = False):
        """force: run the collectives even in a group of one rank (tests: the whole hook -> flush -> RCCL -> wait path on a
        single GPU, where the exchange is the identity).
        shard: every rank owns one contiguous 1/N slab of the flat buffers (`slab(r)`); a bucket's pieces are REDUCED to their
        owners instead of all-reduced (half the bytes on the wire per step; the other half is the parameter broadcast after the
        owners' optimizer step, DataParallelTrainer) -- SURVEY H6's fallback for an exposed all-reduce tail."""
        self.flat, self.group = flat, group
        self.shard = bool(shard)
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.backend = dist.get_backend(group) if dist.is_initialized() else None
        self.bucket_bytes = bucket_bytes
        # First pass: buckets follow REGISTRATION order backwards (last parameters first), the usual proxy for gradient-ready order.
        # It is wrong where registration and use differ -- the Spark model registers its three input-side embedding tables AFTER
        # lm_head, so they sat in bucket 0 (136 MiB) although their gradients arrive at the very end of backward, and the bucket
        # that should open the exchange was the last to fire.  The order the hooks actually fire in is recorded during the first
        # backward pass and the buckets are re-cut along it once (`rebuild_from_ready_order`, what DDP does after its first
        # iteration).  The flat buffers are NOT re-laid-out: a bucket is a list of contiguous runs of the flat gradient buffer
        # (normally one; the embedding-side bucket has one run per end of the buffer), each run one collective.
        self._cut(list(range(len(flat.params) - 1, -1, -1)))
        self.ready_order: List[int] = []
        self.rebuilt = False
        self.order_differs_from_rank0 = False
        self.works = []          # (bucket, work) in launch order
        self.launched = []       # buckets in launch order (the order finish() hands them to `on_bucket`)
        self.use_avg, self.summed = True, []
        self.measure, self.wait_events = False, []
        self.defer_reattach = False   # DataParallelTrainer sets it: it calls flat.reattach() itself, behind the optimizer launch
        self.pre_exchange = None      # callable(s, e): runs on [s, e) of the flat gradient right before that run goes on the wire
        #                               (DataParallelTrainer: the fold of the accumulated micro-batch gradients, bucket by bucket)
        self.enabled = self.world > 1 or (force and dist.is_initialized())
        if self.enabled:
            flat.on_ready = self._ready

    def _cut(self, order):
        """Buckets of >= bucket_bytes along `order` (parameter indices, first-ready first).  self.buckets[b] = [start, end, n_params]
        with [start, end) the span of the bucket's runs (what bench.py prints); self.runs[b] = the contiguous [s, e) pieces."""
        flat, esz = self.flat, self.flat.flat_grad.element_size()
        size = lambda i: ((flat.params[i].numel() + 127) // 128 * 128)
        self.buckets, self.runs = [], []
        self.param_bucket = [0] * len(flat.params)
        cur, nbytes = [], 0
        for n, i in enumerate(order):
            cur.append(i)
            nbytes += size(i) * esz
            self.param_bucket[i] = len(self.buckets)
            if nbytes >= self.bucket_bytes or n == len(order) - 1:
                pieces = sorted((flat.offsets[j], flat.offsets[j] + size(j)) for j in cur)
                runs = [list(pieces[0])]
                for s_, e_ in pieces[1:]:
                    if s_ == runs[-1][1]:
                        runs[-1][1] = e_
                    else:
                        runs.append([s_, e_])
                self.buckets.append([runs[0][0], runs[-1][1], len(cur)])
                self.runs.append([tuple(r) for r in runs])
                cur, nbytes = [], 0
        self.pending = [b[2] for b in self.buckets]
        self.next_bucket = 0

    def rebuild_from_ready_order(self):
        """Re-cut the buckets along the order in which the gradient hooks fired in the pass just finished (once; parameters whose
        hook did not fire go last).  STEP 0 IS NOT REPRESENTATIVE: until this re-cut the buckets follow reverse registration order and
        go on the wire in index order, and bucket 0 then holds the input-side embedding tables whose gradients arrive LAST -- no
        all-reduce starts before backward ends (no overlap), and the re-cut itself is a host-synchronous broadcast + tolist().  Warm-up
        steps absorb it: bench.py times from step W on (W >= 1) and reports `comm.bucket_order` so a line measured on the initial cut
        is recognisable.  The order is RANK 0's, broadcast to everybody (what DDP does): the order a rank records
        depends on the shapes of ITS batch -- fused.mix_lora_supported needs B*T >= 4096, linear_add_eligible / cmix_eligible
        need M % 256 == 0, and the fused nodes hand over the LoRA / x_* gradients in a different order than the plain ones --
        so two ranks fed differently shaped batches on step 0 would otherwise cut their buckets at different byte boundaries
        and the collectives would mismatch (hang or silently wrong sums).  One host-synchronous broadcast of n_params int32,
        once per run.  tests/test_trainer_dist.py drives the two ranks through different orders and asserts the common cut."""
        n = len(self.flat.params)
        order = list(self.ready_order)
        if self.world > 1:
            dev = self.flat.flat_grad.device if self.backend == "nccl" else torch.device("cpu")
            t = torch.full((n,), -1, dtype=torch.int32, device=dev)
            if self.rank == 0:
                t[:len(order)] = torch.tensor(order, dtype=torch.int32)
            src = dist.get_global_rank(self.group, 0) if self.group is not None else 0
            dist.broadcast(t, src=src, group=self.group)
            theirs = [int(i) for i in t.tolist() if i >= 0]
            self.order_differs_from_rank0 = theirs != order
            order = theirs
        self.ready_order = order
        seen = set(order)
        order = order + [i for i in range(n - 1, -1, -1) if i not in seen]
        self._cut(order)
        self.rebuilt = True

    def slab(self, r):
        """[start, end) of rank r's slab of the flat buffers (128-element aligned, the last one may be shorter or empty)."""
        n = self.flat.numel
        size = -(-n // (self.world * 128)) * 128
        return min(r * size, n), min((r + 1) * size, n)

    def _ready(self, i):
        if not self.rebuilt:
            self.ready_order.append(i)
        b = self.param_bucket[i]
        self.pending[b] -= 1
        # buckets go on the wire strictly in INDEX order (as DDP's reducer does): a bucket that completes early waits for its
        # predecessors.  The sequence of collectives is then the same on every rank at every step even when the ranks' hooks
        # fire in different orders (differently shaped batches take different fused paths) -- a mismatched sequence is a hang.
        while self.next_bucket < len(self.pending) and self.pending[self.next_bucket] == 0:
            self._launch(self.next_bucket)
            self.next_bucket += 1

    def _launch(self, b):
        from . import fused
        fused.wgrad_side_sync()   # ... including the weight gradients still running on fused's side stream
        self.flat.flush()   # the bucket's slices must hold the final gradients
        self.launched.append(b)
        for s, e in self.runs[b]:
            if self.pre_exchange is not None:
                self.pre_exchange(s, e)
            self._exchange(s, e, b)

    def _exchange(self, s, e, b=-1):
        if self.shard:
            for r in range(self.world):   # the run's intersection with every rank's slab goes to that rank only
                lo, hi = self.slab(r)
                lo, hi = max(lo, s), min(hi, e)
                if lo >= hi:
                    continue
                piece = self.flat.flat_grad[lo:hi]
                if self.backend == "nccl":
                    self.works.append((b, dist.reduce(piece, dst=dist.get_global_rank(self.group, r) if self.group is not None else r,
                                                      op=dist.ReduceOp.SUM, group=self.group, async_op=True)))
                    if r == self.rank:
                        self.summed.append((b, lo, hi))
                else:   # gloo (CPU tests): fp32, synchronous
                    tmp = piece.float()
                    dist.reduce(tmp, dst=r, op=dist.ReduceOp.SUM, group=self.group)
                    if r == self.rank:
                        piece.copy_((tmp / self.world).to(piece.dtype))
            return
        view = self.flat.flat_grad[s:e]
        if self.backend == "nccl":
            if self.use_avg:
                try:
                    self.works.append((b, dist.all_reduce(view, op=dist.ReduceOp.AVG, group=self.group, async_op=True)))
                    return
                except RuntimeError:   # a collective library without AVG for this dtype: SUM now, one scale in finish()
                    self.use_avg = False
            self.works.append((b, dist.all_reduce(view, op=dist.ReduceOp.SUM, group=self.group, async_op=True)))
            self.summed.append((b, s, e))
        else:  # gloo (CPU tests): no AVG, and bf16 support varies -> reduce in fp32
            tmp = view.float()
            dist.all_reduce(tmp, op=dist.ReduceOp.SUM, group=self.group)
            view.copy_((tmp / self.world).to(view.dtype))

    def finish(self, on_bucket=None):
        """Wait for every bucket (also launches buckets whose hooks never fired, e.g. unused params).  Backward always runs: a
        NaN step backpropagates like any other and the optimizer kernel substitutes a zero gradient (DataParallelTrainer.step).

        on_bucket(runs): called once per bucket, in launch order, as soon as THAT bucket's collectives have completed on the
        compute stream's timeline (work.wait() = the compute stream waits for RCCL's stream up to that collective) -- the
        optimizer steps bucket b while buckets b+1.. are still on the wire, instead of one replicated pass behind the last
        all-reduce.  Returns True if it was called for every bucket (False: exchange disabled, caller does one whole pass)."""
        self.flat.finish_backward(reattach=self.defer_reattach is False)
        if not self.enabled:
            return False
        for b in range(self.next_bucket, len(self.pending)):   # incomplete buckets (unused parameters) and their successors
            self._launch(b)
        # wait() makes the compute stream wait for RCCL's stream; what the compute stream then stalls is the exposed (non-overlapped)
        # part of the exchange -- bracketed by event pairs when `measure` is on (bench.py): one pair around ALL waits in the one-pass
        # mode, one pair around each bucket's waits in the per-bucket mode (the optimizer launches between them are work, not stall)
        def bracket():
            if self.measure and self.works:
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                return e
            return None
        per_bucket = on_bucket is not None and not self.shard
        if per_bucket:
            by_b, scale_b = {}, {}
            for b, w in self.works:
                by_b.setdefault(b, []).append(w)
            for b, s, e in self.summed:
                scale_b.setdefault(b, []).append((s, e))
            for b in self.launched:
                e0 = bracket()
                for w in by_b.get(b, ()):
                    w.wait()
                e1 = bracket()
                if e0 is not None:
                    self.wait_events.append((e0, e1))
                for s, e in scale_b.get(b, ()):
                    self.flat.flat_grad[s:e].mul_(1.0 / self.world)
                on_bucket(self.runs[b])
        else:
            e0 = bracket()
            for _, w in self.works:
                w.wait()
            e1 = bracket()
            if e0 is not None:
                self.wait_events.append((e0, e1))
            for _, s, e in self.summed:
                self.flat.flat_grad[s:e].mul_(1.0 / self.world)
        self.works, self.summed, self.launched = [], [], []
        if not self.rebuilt and (self.ready_order or self.world > 1):
            self.rebuild_from_ready_order()   # once, after the first backward pass (also resets `pending`)
        else:
            self.pending = [b[2] for b in self.buckets]
            self.next_bucket = 0
        return per_bucket


def linear_warmup_decay(step, total_steps, warmup_steps, lr, lr_final):
    """train_spark_rwkv7speech.py:219-232."""
    if step < warmup_steps:
        return lr * float(step) / float(max(1, warmup_steps))
    progress = float(step - warmup_steps) / float(max(1, total_steps - warmup_steps))
    return lr * max(lr_final / lr, 1.0 - progress * (1.0 - lr_final / lr))


def cosine_warmup_decay(step, total_steps, warmup_steps, lr, lr_final):
    """train_cosy_rwkv7speech_multiple_dataset.py:224-234: warmup from 1 % of lr, then half a cosine down to lr_final."""
    if step < warmup_steps:
        return lr * (0.01 + 0.99 * step / warmup_steps)
    progress = float(step - warmup_steps) / float(max(1, total_steps - warmup_steps))
    progress = max(0.0, min(1.0, progress))
    f = lr_final / lr
    return lr * ((0.5 + f / 2) + (0.5 - f / 2) * math.cos(math.pi * progress))


SCHEDULES = {"linear": linear_warmup_decay, "cosine": cosine_warmup_decay}

CHECKPOINT_FORMAT = 1
DIGEST_NAMES = ("master", "exp_avg", "exp_avg_sq", "param")


def _write_synced(path, data):
    """data (bytes, a uint8 numpy array, or an iterable of such arrays that are written one after the other) to `path`, flushed to
    the disk before the call returns."""
    with open(path, "wb") as f:
        if isinstance(data, (bytes, bytearray)):
            f.write(data)
        elif hasattr(data, "tofile"):
            data.tofile(f)
        else:
            for piece in data:
                piece.tofile(f)
        f.flush()
        os.fsync(f.fileno())


def _write_checkpoint_files(tmp, job, payload):
    """What one rank contributes to <tag>.tmp/, shared by the blocking save and the writer thread of the non-blocking one: the
    range's .bin files and its .json (if the rank writes tensors), rng_rank<r>.pt, and rank 0's meta.json.  job:
    DataParallelTrainer._checkpoint_job's record, complete before the first byte is written; payload(name): the raw bytes of the
    range of buffer `name`, in a form _write_synced takes.  Reads no trainer; _write_synced is looked up at every call."""
    for name, fname in job["files"].items():
        _write_synced(os.path.join(tmp, fname), payload(name))
    if job["files"]:
        _write_synced(os.path.join(tmp, job["stem"] + ".json"), job["range_json"])
    rng_path = os.path.join(tmp, f"rng_rank{job['rank']}.pt")
    torch.save(job["rng"], rng_path)
    with open(rng_path, "rb") as f:
        os.fsync(f.fileno())
    if job["meta_json"] is not None:
        _write_synced(os.path.join(tmp, "meta.json"), job["meta_json"])


CHECKPOINT_PIECE_BYTES = 64 << 20   # each of the TWO pinned host buffers a non-blocking save copies its staging through


def _staged_pieces(staging, pinned, stream):
    """The raw bytes of the device tensor `staging` as uint8 numpy arrays of at most len(pinned[0]) bytes, in order: piece i + 1 is
    on its way into one pinned buffer (on `stream`) while the consumer writes piece i out of the other.  A yielded array is valid
    until the next one is asked for."""
    raw = staging.view(torch.uint8)
    n, step = raw.numel(), pinned[0].numel()
    sizes = [min(step, n - s_) for s_ in range(0, n, step)]
    events = [None, None]

    def issue(i):
        with torch.cuda.stream(stream):
            pinned[i % 2][:sizes[i]].copy_(raw[i * step:i * step + sizes[i]], non_blocking=True)
            events[i % 2] = torch.cuda.Event()
            events[i % 2].record(stream)

    if sizes:
        issue(0)
    for i, m in enumerate(sizes):
        events[i % 2].synchronize()
        if i + 1 < len(sizes):
            issue(i + 1)   # into the buffer of piece i - 1, which the consumer has finished with
        yield pinned[i % 2][:m].numpy()


class PendingCheckpoint:
    """A non-blocking save that has not been finalised (DataParallelTrainer.pending_checkpoint): its tag, the path it will have,
    the step it was taken at and the four digests of this rank's range at that moment."""

    def __init__(self, dir, tag, path, step_idx, digests, keep_last):
        self.dir, self.tag, self.path, self.step_idx, self.digests, self.keep_last = dir, tag, path, step_idx, digests, keep_last
        self.error = None    # the writer thread's exception, if it raised one
        self.thread = None

    def __repr__(self):
        return f"PendingCheckpoint(tag={self.tag!r}, path={self.path!r}, step_idx={self.step_idx})"


def _checkpoint_writer(pending, tmp, job, payload, stream, event):
    """The writer thread of a non-blocking save.  It reads the staging buffers and writes files: no trainer state, no collective."""
    try:
        if stream is not None:
            stream.wait_event(event)   # the snapshot kernels, in the order of the stream they were enqueued on
        _write_checkpoint_files(tmp, job, payload)
    except Exception as e:   # kept for checkpoint_wait(), which raises on the calling thread of every rank
        pending.error = e
    finally:
        if stream is not None:
            stream.synchronize()   # no copy into the pinned buffers is left in flight, whatever happened


def _sync_dir(path):
    fd = os.open(path, os.O_RDONLY)
    try:
        os.fsync(fd)
    finally:
        os.close(fd)


def _read_json(path):
    with open(path) as f:
        return json.load(f)


def complete_checkpoints(dir):
    """[(step_idx, tag)] of the complete checkpoints under `dir`, oldest first.  A `<tag>.tmp` directory (a save that did not
    finish) is never one."""
    out = []
    for tag in os.listdir(dir) if os.path.isdir(dir) else ():
        meta = os.path.join(dir, tag, "meta.json")
        if tag.endswith(".tmp") or not os.path.isfile(meta):
            continue
        try:
            m = _read_json(meta)
        except ValueError:
            continue
        if m.get("format") == CHECKPOINT_FORMAT:
            out.append((int(m["step_idx"]), os.path.getmtime(meta), tag))
    return [(s_, t) for s_, _, t in sorted(out)]


def reference_param_groups(model: torch.nn.Module, weight_decay: float):
    """The parameter groups of configure_optimizer (train_cosy_rwkv7speech_multiple_dataset.py:162-190), one entry per
    trainable parameter in model.parameters() order: (group name, lr scale, weight decay).
      lr_2x    : names containing 'attn.w_lora.lora.2.bias' (the decay bias w0)            -> lr x 2, no decay
      lr_decay : >= 2-D (after squeeze) '.weight' tensors outside the LoRAs, if weight_decay > 0 -> lr x 1, decay
      lr_1x    : everything else                                                            -> lr x 1, no decay"""
    out = []
    for n, p in model.named_parameters():
        if not p.requires_grad:
            continue
        if "attn.w_lora.lora.2.bias" in n:
            out.append(("lr_2x", 2.0, 0.0))
        elif len(p.squeeze().shape) >= 2 and weight_decay > 0 and ".weight" in n and "lora" not in n:
            out.append(("lr_decay", 1.0, float(weight_decay)))
        else:
            out.append(("lr_1x", 1.0, 0.0))
    return out


class DataParallelTrainer:
    """param_groups: None = the Spark trainer's single group (train_spark_rwkv7speech.py:178-197: every parameter lr x 1 and an
    explicit "weight_decay": 0.0 at :188, which overrides the optimizer default -- the reference decays NOTHING there, whatever
    args.weight_decay says; so does this mode: `weight_decay` is ignored); "all" = one group with `weight_decay` on every tensor
    (explicit opt-in; not what either reference trainer does); "reference" = reference_param_groups(model, weight_decay) (the
    Cosy trainer's lr_2x / lr_decay split); or a list of (name, lr scale, weight decay), one per trainable parameter.
    schedule: "linear" (Spark trainer) or "cosine" (Cosy)."""

    def __init__(self, model: torch.nn.Module, lr=1e-4, lr_final=1e-5, warmup_steps=100, total_steps=100000,
                 weight_decay=0.0, betas=(0.9, 0.95), eps=1e-18, bucket_bytes=32 << 20, nan_guard=True,
                 master_fp32=True, param_groups=None, schedule="linear", force_allreduce=False, shard_optimizer=False,
                 bucket_optimizer=True, max_grad_norm=None, logit_stats=False):
        """shard_optimizer: every rank reduces the gradient pieces of ITS 1/N slab only, steps AdamW on that slab and broadcasts
        the slab's new bf16 parameters (reduce-scatter + sharded optimizer + all-gather, ZeRO-1 style: the reference's DeepSpeed
        ZeRO-2 engine does the same exchange, train_spark_rwkv7speech.py:483-516).  Same parameters after every step as the
        default (all-reduce + replicated AdamW) up to the rounding of the reduction; the optimizer pass is 1/N as long.  One flag:
        for the case that the 8-GPU scaling run shows an exposed all-reduce tail.
        NOTE for code that reads gradients after step(): in shard mode only the slices of a rank's OWN slab hold the reduced (mean)
        gradient; `p.grad` of parameters in foreign slabs holds this rank's local, unreduced gradient (gradient-norm logging or
        clipping must all-reduce its own partial over the own slab, `reducer.slab(rank)`).
        bucket_optimizer (default, all-reduce mode with > 1 rank): AdamW runs bucket by bucket, each as soon as its own
        all-reduce has completed, so the optimizer pass (2.1-2.4 ms for the 0.4B model) overlaps the buckets still on the wire
        instead of sitting behind the last one.  Element-wise the same update: identical parameters to the one-pass mode.
        max_grad_norm: clip the (reduced) gradient by its global L2 norm, torch.nn.utils.clip_grad_norm_'s rule (the reference
        hands `gradient_clipping` to DeepSpeed, train_scripts/train_rwkv_tts.py:133,405): coef = min(1, max_grad_norm / (norm +
        1e-6)).  One sum-of-squares pass over the reduced gradient (rwkv7_grad_sumsq_bf16: the whole buffer, or the own slab plus a
        one-element all_reduce(SUM) in shard mode), then ONE AdamW pass that reads the sum from device memory and scales the
        gradient as it loads it (rwkv7_adamw_groups_clip_bf16); the gradient buffer itself is left unscaled.  The norm is not known
        before the last bucket has landed, so clipping GIVES UP the per-bucket optimizer overlap of `bucket_optimizer`: the optimizer
        pass sits behind the last all-reduce.  Every rank computes the factor from identical data: replicas stay bit-identical.
        A non-finite norm makes the step a zero-gradient step, like a NaN loss.  float('inf') = measure only.
        `last_grad_norm` (None without max_grad_norm): device fp32 scalar, the pre-clip norm of the last step; step() never
        reads it on the host.
        logit_stats: keep the scale of the head's logits.  Always on when the model's config has a non-zero
        z_loss or max_logit.  The trainer owns an fp32 [4] device tensor that the model's fused training loss adds (tokens, sum lse,
        sum lse^2, sum max logit) into -- every micro-batch and, for the XY model, every channel -- zeroes it at the start of every
        optimizer step, and after step() exposes `last_logit_stats`: {"mean_lse", "mean_lse_sq", "mean_max", "tokens"}, device
        tensors of THIS rank's rows only (no collective, no synchronisation).  evaluate, score, preference_step and policy_step
        neither see the coefficients nor touch the statistics.  Needs a model whose training loss is the fused cross-entropy (Spark,
        XY)."""
        self.model = model
        self.bucket_optimizer = bool(bucket_optimizer)
        self.flat = FlatBuffers(model)
        self.reducer = BucketedAllReduce(self.flat, bucket_bytes, force=force_allreduce, shard=shard_optimizer)
        self.shard_optimizer = bool(shard_optimizer) and self.reducer.enabled
        self.reducer.defer_reattach = True
        self.world = self.reducer.world
        self.master = self.flat.flat_param.float() if master_fp32 and self.flat.flat_param.dtype != torch.float32 \
            else self.flat.flat_param
        self.betas, self.eps, self.weight_decay = betas, eps, weight_decay
        if param_groups == "reference":
            param_groups = reference_param_groups(model, weight_decay)
        if param_groups is None:
            if weight_decay:
                import warnings
                warnings.warn("DataParallelTrainer(param_groups=None) decays nothing, like the Spark trainer's single group "
                              "(train_spark_rwkv7speech.py:188); weight_decay=%g is ignored -- pass param_groups='all' (decay every "
                              "parameter) or 'reference' (the Cosy trainer's lr_decay group)" % weight_decay, stacklevel=2)
            param_groups = [("all", 1.0, 0.0)] * len(self.flat.params)
        elif param_groups == "all":
            param_groups = [("all", 1.0, float(weight_decay))] * len(self.flat.params)
        assert len(param_groups) == len(self.flat.params), "one (name, lr scale, weight decay) per trainable parameter"
        self.group_defs = []          # distinct (name, lr scale, weight decay)
        self.param_group_idx = []
        for g in param_groups:
            g = (g[0], float(g[1]), float(g[2]))
            if g not in self.group_defs:
                self.group_defs.append(g)
            self.param_group_idx.append(self.group_defs.index(g))
        assert len(self.group_defs) <= 256
        dev = self.master.device
        self.schedule = SCHEDULES[schedule] if isinstance(schedule, str) else schedule
        # bf16 parameters on the HIP device: one kernel reads the bf16 gradients, updates the fp32 master weights and
        # moments and rewrites the bf16 parameters (rwkv7_adamw_groups_bf16) -- no fp32 gradient copy, no separate cast
        # back; the group of every 128-element slab of the flat buffer comes from a uint8 table (FlatBuffers aligns the
        # parameters to 128 elements), the NaN flag stays on the device
        self.hip_adamw = (self.master is not self.flat.flat_param and self.master.is_cuda
                          and self.flat.flat_param.dtype == torch.bfloat16 and self.flat.numel % 128 == 0)
        self.exp_avg = torch.zeros_like(self.master)
        self.exp_avg_sq = torch.zeros_like(self.master)
        if self.hip_adamw:
            slab = torch.zeros(self.flat.numel // 128, dtype=torch.uint8)
            ends = self.flat.offsets[1:] + [self.flat.numel]
            for o, e, gi in zip(self.flat.offsets, ends, self.param_group_idx):
                slab[o // 128:e // 128] = gi
            self.slab_group = slab.to(dev)
            self.group_tab = torch.tensor([[g[1], g[2]] for g in self.group_defs], dtype=torch.float32).to(dev)
        else:
            # CPU (gloo tests) / fp32 models: the same update rule in torch, group by group on runs of the flat buffers
            self.runs = []   # (start, end, group index): consecutive parameters of one group merged
            ends = self.flat.offsets[1:] + [self.flat.numel]
            for o, e, gi in zip(self.flat.offsets, ends, self.param_group_idx):
                if self.runs and self.runs[-1][2] == gi and self.runs[-1][1] == o:
                    self.runs[-1] = (self.runs[-1][0], e, gi)
                else:
                    self.runs.append((o, e, gi))
        self.lr, self.lr_final, self.warmup_steps, self.total_steps = lr, lr_final, warmup_steps, total_steps
        self.nan_guard = nan_guard
        self.nan_flag = torch.zeros(1, dtype=torch.float32, device=dev)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.last_grad_norm = None
        if self.max_grad_norm is not None:
            assert self.max_grad_norm >= 0.0, "max_grad_norm must be >= 0 (float('inf'): measure only)"
            self.last_grad_norm = torch.zeros((), dtype=torch.float32, device=dev)
            # the sum of squares stays on the device: fp32 + per-tile partials for the HIP pass, float64 in the torch fallback
            self._sumsq = torch.zeros(1, dtype=torch.float32 if self.hip_adamw else torch.float64, device=dev)
            if self.hip_adamw:
                nbytes = _lib.lib().rwkv7_grad_sumsq_workspace_bytes(self.flat.numel)
                self._sumsq_partials = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        # micro-batch accumulation (accumulate()): fp32 sum of the gradients of the micro-batches before the one step() runs,
        # allocated on first use; their count; the running max of their NaN flags
        self._acc32 = None
        self._acc_count = 0
        self._acc_flag = torch.zeros(1, dtype=torch.float32, device=dev)
        cfg = getattr(model, "config", None)
        self.last_logit_stats = None
        self._logit_stats = None
        if logit_stats or getattr(cfg, "z_loss", 0.0) or getattr(cfg, "max_logit", 0.0):
            if not hasattr(model, "logit_stats"):
                raise ValueError("DataParallelTrainer(logit_stats=True): the model's training loss does not keep logit statistics "
                                 "(the Spark and XY models do)")
            self._logit_stats = model.logit_stats = torch.zeros(4, dtype=torch.float32, device=dev)
        self.step_idx = 0
        self.last_lr = None
        self._pending = None          # the one non-blocking save in flight (PendingCheckpoint)
        self._ckpt_staging = None     # its staging buffers, allocated on the first non-blocking save and kept
        # modules that cache tensors derived from parameters (RWKV7Attention._stacked_mix): the optimizer kernel rewrites
        # parameter memory through raw pointers without touching autograd's version counters, so they are told explicitly
        self._param_caches = [m for m in model.modules() if hasattr(m, "_mix_key") or hasattr(m, "_stacked_mix")]

    def current_lr(self):
        return self.schedule(self.step_idx, self.total_steps, self.warmup_steps, self.lr, self.lr_final)

    def group_lrs(self):
        """{group name: lr of the next step} -- what update_learning_rate writes into optimizer.param_groups (:236-241)."""
        base = self.current_lr()
        return {g[0]: base * g[1] for g in self.group_defs}

    def _torch_adamw(self, lr, skip, lo_s=None, hi_s=None, coef=None):
        g_all = self.flat.flat_grad
        b1, b2 = self.betas
        t = self.step_idx + 1
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        if lo_s is None:
            lo_s, hi_s = self.reducer.slab(self.reducer.rank) if self.shard_optimizer else (0, self.flat.numel)
        for s, e, gi in self.runs:
            s, e = max(s, lo_s), min(e, hi_s)   # sharded: this rank's slab only
            if s >= e:
                continue
            _, scale, wd = self.group_defs[gi]
            p, m, v = self.master[s:e], self.exp_avg[s:e], self.exp_avg_sq[s:e]
            g = g_all[s:e].to(p.dtype)
            if coef is not None:
                g = g * coef
            g = torch.where(skip.to(torch.bool), torch.zeros_like(g), g)
            lr_g = lr * scale
            p.mul_(1.0 - lr_g * wd)
            m.mul_(b1).add_(g, alpha=1.0 - b1)
            v.mul_(b2).addcmul_(g, g, value=1.0 - b2)
            p.addcdiv_(m, (v.sqrt() / math.sqrt(bc2)).add_(self.eps), value=-lr_g / bc1)
        if self.master is not self.flat.flat_param:
            self.flat.flat_param[lo_s:hi_s].copy_(self.master[lo_s:hi_s])

    def _broadcast_slabs(self):
        """Sharded mode: every rank's freshly stepped parameter slab to everybody (an all-gather written as N broadcasts: the
        slabs need not be equally long), and the fp32 masters of the foreign slabs re-derived from it are not needed -- a rank
        only ever steps its own slab."""
        r_ = self.reducer
        works = []
        for r in range(r_.world):
            lo, hi = r_.slab(r)
            if lo >= hi:
                continue
            piece = self.flat.flat_param[lo:hi]
            src = dist.get_global_rank(r_.group, r) if r_.group is not None else r
            if r_.backend == "nccl":
                works.append(dist.broadcast(piece, src=src, group=r_.group, async_op=True))
            else:
                tmp = piece.float()
                dist.broadcast(tmp, src=src, group=r_.group)
                piece.copy_(tmp.to(piece.dtype))
        for w in works:
            w.wait()

    def _grad_sumsq(self, lo, hi):
        """self._sumsq = sum of squares of flat_grad[lo:hi] (0 for an empty slab), on the device."""
        if hi <= lo:
            self._sumsq.zero_()
        elif self.hip_adamw:
            _lib.call("rwkv7_grad_sumsq_bf16", self.master, hi - lo, self.flat.flat_grad[lo:hi], self._sumsq_partials, self._sumsq, 0)
        else:
            self._sumsq.copy_(self.flat.flat_grad[lo:hi].double().pow(2).sum().reshape(1))

    def _adamw_clip(self, lo, hi, lr):
        """AdamW on [lo, hi) with the gradient scaled by min(1, max_grad_norm / (sqrt(self._sumsq) + 1e-6)); a non-finite sum
        makes it a zero-gradient step.  Neither value is read on the host."""
        if hi <= lo:
            return
        if self.hip_adamw:
            _lib.call("rwkv7_adamw_groups_clip_bf16", self.master,
                      hi - lo, self.master[lo:hi], self.flat.flat_grad[lo:hi], self.exp_avg[lo:hi], self.exp_avg_sq[lo:hi],
                      self.flat.flat_param[lo:hi], self.slab_group[lo // 128:hi // 128], self.group_tab, len(self.group_defs),
                      self.nan_flag, self._sumsq, self.max_grad_norm, lr, self.betas[0], self.betas[1], self.eps, self.step_idx + 1)
        else:
            ss = self._sumsq[0]
            coef = torch.clamp(self.max_grad_norm / (ss.sqrt() + 1e-6), max=1.0).to(self.master.dtype)
            skip = torch.maximum(self.nan_flag, (~torch.isfinite(ss)).to(self.nan_flag.dtype).reshape(1))
            self._torch_adamw(lr, skip, lo, hi, coef=coef)

    def _fold(self, lo, hi, inv_count):
        """flat_grad[lo:hi] = round((fp32 sum of the earlier micro-batches + flat_grad[lo:hi]) * inv_count), in place."""
        if hi <= lo:
            return
        g = self.flat.flat_grad[lo:hi]
        if self.hip_adamw:
            _lib.call("rwkv7_grad_fold_bf16", self.master, hi - lo, self._acc32[lo:hi], g, inv_count)
        else:
            g.copy_(((self._acc32[lo:hi] + g.float()) * inv_count).to(g.dtype))

    def accumulate(self, **batch):
        """One micro-batch of gradient accumulation (`accum_grad` / `gradient_accumulation_steps` of the reference recipes,
        third_party/cosyvoice/utils/train_utils.py:87-89): forward and backward into the flat bf16 buffer, then that gradient is
        added to an fp32 buffer of flat.numel elements (allocated on first use; DeepSpeed's bf16 engine accumulates in fp32 too).
        No collective is issued and the reducer's bucket bookkeeping is left as if the pass had not happened; the NaN flag of the
        micro-batch joins a running max.  k - 1 calls followed by step() make one optimizer step on the mean gradient of the k
        micro-batches.  Returns the (detached) loss tensor."""
        if self._acc32 is None:
            self._acc32 = torch.empty(self.flat.numel, dtype=torch.float32, device=self.flat.flat_grad.device)
        first = self._acc_count == 0
        if first and self._logit_stats is not None:
            self._logit_stats.zero_()
        self.flat.arm()
        on_ready, self.flat.on_ready = self.flat.on_ready, None   # the reducer does not see this pass
        try:
            loss = self.model(**batch).loss
            if self.nan_guard:
                bad = (~torch.isfinite(loss.detach())).reshape(1).to(self._acc_flag.dtype)
                if first:
                    self._acc_flag.copy_(bad)
                else:
                    torch.maximum(self._acc_flag, bad, out=self._acc_flag)
            else:
                self._acc_flag.zero_()
            loss.backward()
            self.flat.finish_backward(reattach=True)
        finally:
            self.flat.on_ready = on_ready
        if self.hip_adamw:
            _lib.call("rwkv7_grad_accum_bf16", self.master, self.flat.numel, self._acc32, self.flat.flat_grad, int(first))
        elif first:
            self._acc32.copy_(self.flat.flat_grad)
        else:
            self._acc32.add_(self.flat.flat_grad.float())
        self._acc_count += 1
        return loss.detach()

    def step(self, **batch):
        """One optimisation step on this rank's shard of the batch.  Returns the (detached) loss tensor.

        No host synchronisation anywhere in the step: the reference's NaN guard (forward -> 1-element all_reduce(MAX) of
        `isnan(loss)` -> every rank backpropagates loss * 0 and steps on a zero gradient, train_spark_rwkv7speech.py:
        664-687) keeps its flag on the device -- the all-reduce is enqueued before backward, backward runs regardless,
        and the optimizer kernel reads the flag and substitutes a zero gradient.  Nothing waits for `flag.item()`, so
        the gradient buckets start as soon as backward reaches them.

        After k - 1 accumulate() calls this batch is the k-th micro-batch: every bucket is folded with the fp32 sum of the earlier
        gradients (rwkv7_grad_fold_bf16, mean over k, one rounding to bf16) right before it goes on the wire, so the exchange still
        overlaps this backward pass; the NaN flag that is all-reduced is the max over the k micro-batches.  Without a preceding
        accumulate() nothing of that runs."""
        if self._logit_stats is None:
            return self._step_on(lambda: (self.model(**batch).loss, None))
        if self._acc_count == 0:
            self._logit_stats.zero_()
        loss = self._step_on(lambda: (self.model(**batch).loss, None))
        n, s_lse, s_sq, s_max = self._logit_stats.clone().unbind(0)
        d = n.clamp(min=1)
        self.last_logit_stats = dict(mean_lse=s_lse / d, mean_lse_sq=s_sq / d, mean_max=s_max / d, tokens=n)
        return loss

    def _step_on(self, loss_fn):
        """The body of step() for any scalar loss: loss_fn() runs the forward pass (after the gradient hooks are armed) and returns
        (loss, bad), bad: None, or a device bool that raises the NaN flag besides a non-finite loss.  Returns the detached loss."""
        k = self._acc_count + 1
        if k > 1:
            self.reducer.pre_exchange = lambda s_, e_: self._fold(s_, e_, 1.0 / k)
        self.flat.arm()
        loss, bad = loss_fn()
        flag_work = None
        if self.nan_guard:
            nonfinite = ~torch.isfinite(loss.detach())
            self.nan_flag.copy_((nonfinite if bad is None else nonfinite | bad).reshape(1))
            if k > 1:
                torch.maximum(self.nan_flag, self._acc_flag, out=self.nan_flag)
            if self.world > 1:
                flag_work = dist.all_reduce(self.nan_flag, op=dist.ReduceOp.MAX, async_op=True)  # :664-670
        else:
            self.nan_flag.zero_()
        loss.backward()
        lr = self.current_lr()
        self.last_lr = lr
        if flag_work is not None:
            flag_work.wait()   # enqueued before backward: long done; the optimizer launches below read the flag

        def adamw(lo, hi):
            if hi <= lo:
                return
            if self.hip_adamw:
                _lib.call("rwkv7_adamw_groups_bf16", self.master,
                          hi - lo, self.master[lo:hi], self.flat.flat_grad[lo:hi], self.exp_avg[lo:hi], self.exp_avg_sq[lo:hi],
                          self.flat.flat_param[lo:hi], self.slab_group[lo // 128:hi // 128], self.group_tab, len(self.group_defs),
                          self.nan_flag, lr, self.betas[0], self.betas[1], self.eps, self.step_idx + 1)
            else:
                self._torch_adamw(lr, self.nan_flag, lo, hi)

        def on_bucket(runs):   # the runs of one bucket tile 128-aligned pieces of the flat buffers
            for s_, e_ in runs:
                adamw(s_, e_)

        clip = self.max_grad_norm is not None
        stepped = self.reducer.finish(on_bucket if self.bucket_optimizer and not self.shard_optimizer and not clip else None)
        if k > 1:
            self.reducer.pre_exchange = None
            if not self.reducer.enabled:
                self._fold(0, self.flat.numel, 1.0 / k)   # no exchange to overlap: one pass
            self._acc_count = 0
        if clip:   # the norm needs every bucket: one sum-of-squares pass, then one optimizer pass behind it
            lo, hi = self.reducer.slab(self.reducer.rank) if self.shard_optimizer else (0, self.flat.numel)
            self._grad_sumsq(lo, hi)
            if self.shard_optimizer:
                dist.all_reduce(self._sumsq, op=dist.ReduceOp.SUM, group=self.reducer.group)
            torch.sqrt(self._sumsq[0], out=self.last_grad_norm)
            self._adamw_clip(lo, hi, lr)
        elif not stepped:
            adamw(*(self.reducer.slab(self.reducer.rank) if self.shard_optimizer else (0, self.flat.numel)))
        if self.shard_optimizer:
            self._broadcast_slabs()
        self.flat.reattach()   # host-only bookkeeping, behind the optimizer launch (see FlatBuffers.finish_backward)
        for m in self._param_caches:
            m._mix_key = None
        self.step_idx += 1
        return loss.detach()

    def preference_step(self, *, beta, ref_logps=None, sft_weight=0.0, **batch):
        """One optimisation step of direct preference optimisation on this rank's 2P utterances: utterance 2i
        is the chosen and 2i + 1 the rejected candidate of pair i.  ref_logps: [2P] (tensor or numpy), the frozen reference's sum of
        log-probabilities per utterance, i.e. -score([batch])["loss_sum"] taken before tuning; None: zeros.  With pi the policy's
        model.sequence_logprobs(**batch)["logp"] (the module's current mode; the backbone forward runs twice, see there):
            margin_i = beta ((pi_c - pi_r) - (ref_c - ref_r)),
            loss = mean_i softplus(-margin_i) + sft_weight (-sum_i pi_c,i / sum_i tokens_c,i),
        in fp64 on the device.  The loss then takes exactly step()'s path (_step_on): armed hooks, the on-device NaN flag (raised by a
        non-finite loss or a non-finite ref_logps entry: a zero-gradient step on every rank), the bucketed exchange, clipping, the
        AdamW launches, reattach, step_idx.  No host read.  Not allowed inside an accumulation window.  Returns device tensors: loss,
        margin (mean), accuracy (share of pairs with margin > 0), logp_chosen [P], logp_rejected [P] (all detached)."""
        if self._acc_count != 0:
            raise RuntimeError(f"preference_step inside an accumulation window ({self._acc_count} micro-batches pending): "
                               "call step() first")
        out = {}

        def loss_fn():
            seq = self.model.sequence_logprobs(**batch)
            logp, tokens = seq["logp"], seq["tokens"]
            ref = torch.zeros_like(logp) if ref_logps is None else \
                torch.as_tensor(ref_logps).to(device=logp.device, dtype=logp.dtype).reshape(-1)
            if logp.numel() % 2 != 0 or logp.numel() == 0 or ref.numel() != logp.numel():
                self.flat.reattach()   # nothing ran backward: the hooks are disarmed again
                raise ValueError(f"preference_step needs chosen/rejected pairs and one ref_logps entry each: {logp.numel()} "
                                 f"utterances, {ref.numel()} reference values")
            pc, pr = logp[0::2], logp[1::2]
            margin = float(beta) * ((pc - pr) - (ref[0::2] - ref[1::2]))
            loss = torch.nn.functional.softplus(-margin).mean()
            if sft_weight:
                loss = loss - float(sft_weight) * (pc.sum() / tokens[0::2].sum().clamp(min=1))
            m = margin.detach()
            out.update(margin=m.mean(), accuracy=(m > 0).double().mean(), logp_chosen=pc.detach(), logp_rejected=pr.detach())
            return loss, ~torch.isfinite(ref).all()

        out["loss"] = self._step_on(loss_fn)
        return {k: out[k] for k in ("loss", "margin", "accuracy", "logp_chosen", "logp_rejected")}

    def policy_step(self, *, advantages, old_logps, ref_logps=None, clip=(0.2, 0.2), kl_beta=0.0, normalize="sequence", **batch):
        """One optimisation step of the token-level clipped policy gradient (GRPO / PPO-clip) on this rank's
        utterances: model.policy_loss(**batch) with one advantage per utterance (losses.group_advantages forms GRPO's from rewards),
        old_logps [rows] the sampling policy's log p(label) of every row of score's flattened rows (token_logprobs gives them) and,
        optionally, ref_logps [rows] a frozen reference's, which adds kl_beta times the k3 KL estimator per token.  The backbone
        forward runs ONCE, on the tape (the module's current mode).  The loss then takes exactly step()'s path (_step_on): armed
        hooks, the on-device NaN flag (raised by a non-finite loss, a non-finite advantage, or a non-finite old_logps / ref_logps
        entry on a row that counts: a zero-gradient step on every rank), the bucketed exchange, clipping, the AdamW launches,
        reattach, step_idx.  No host read.  Not allowed inside an accumulation window.  Returns device tensors (detached): loss,
        clip_frac (share of the rows that count whose clipped branch was the minimum), kl (token mean of the k3 estimator; 0 without
        ref_logps) and ratio_mean (token mean of exp(lp - old_logps))."""
        if self._acc_count != 0:
            raise RuntimeError(f"policy_step inside an accumulation window ({self._acc_count} micro-batches pending): "
                               "call step() first")
        out = {}

        def loss_fn():
            try:
                res = self.model.policy_loss(advantages=advantages, old_logps=old_logps, ref_logps=ref_logps, clip=clip,
                                             kl_beta=kl_beta, normalize=normalize, **batch)
            except BaseException:
                self.flat.reattach()   # whatever it was, nothing ran backward: the hooks are disarmed again
                raise
            valid, lp = res["valid"], res["logp"]
            dev = lp.device
            n = valid.sum().clamp(min=1).double()
            old = torch.as_tensor(old_logps).to(device=dev, dtype=torch.float32).reshape(-1)
            bad = ~torch.isfinite(torch.as_tensor(advantages).to(dev).double()).all() | (~torch.isfinite(old) & valid).any()
            if ref_logps is not None:
                bad = bad | (~torch.isfinite(torch.as_tensor(ref_logps).to(device=dev, dtype=torch.float32).reshape(-1)) & valid).any()
            zero = torch.zeros_like(lp)
            out.update(clip_frac=res["clipped"].double().sum() / n, kl=res["kl"].double().sum() / n,
                       ratio_mean=torch.where(valid, torch.exp(lp - old), zero).double().sum() / n)
            return res["loss"], bad

        out["loss"] = self._step_on(loss_fn)
        return {k: out[k] for k in ("loss", "clip_frac", "kl", "ratio_mean")}

    def token_logprobs(self, batches):
        """log p(label) of every row of this rank's batches: model.token_logprobs per batch (eval mode under no_grad, so nothing of the
        run moves -- see score), a list with one device fp32 tensor [rows] per batch in score's flattened row order, 0 on ignored
        rows.  No collective, no host read.  What policy_step takes as old_logps (from the policy before the update) and ref_logps
        (from a frozen reference).  Not allowed inside an accumulation window."""
        if self._acc_count != 0:
            raise RuntimeError(f"token_logprobs inside an accumulation window ({self._acc_count} micro-batches pending): "
                               "call step() first")
        return [self.model.token_logprobs(**batch) for batch in batches]

    def evaluate(self, batches):
        """Held-out evaluation.  batches: an iterable of batch dicts, this rank's shard (at least one batch on
        every rank).  model.eval_metrics per batch; the sums stay on the device, ONE all_reduce(SUM) at the end when world > 1 (a
        collective: every rank calls evaluate), then ONE host read.  Returns Python numbers: `loss` (recomputed from the global sums
        with the head's own normalisation: loss_sum / tokens for the token-mean heads, summed over the channels for XY), `accuracy`
        (correct / tokens), `tokens`, and for a multi-channel head `per_channel` = {"loss", "accuracy", "tokens"} lists.
        Nothing of the run moves: eval mode under no_grad (no dropout draw, no gradient hook fires), so parameters, masters, moments,
        step_idx, the learning rate, the flat gradient buffer, the NaN flag, the reducer's bucket bookkeeping and the host and device
        random streams are what they were -- k steps, evaluate, m steps is bit-identical to k + m steps.  Not allowed inside an
        accumulation window; allowed while a non-blocking checkpoint's writer is running (it reads its own staged copy)."""
        if self._acc_count != 0:
            raise RuntimeError(f"evaluate inside an accumulation window ({self._acc_count} micro-batches pending): "
                               "call step() first")
        sums = None   # fp64 [4, channels]: loss_sum, denom, tokens, correct (counts are exact in fp64 up to 2^53)
        for batch in batches:
            m = self.model.eval_metrics(**batch)
            cur = torch.stack([m[k].double() for k in ("loss_sum", "denom", "tokens", "correct")])
            sums = cur if sums is None else sums.add_(cur)
        if sums is None:
            raise ValueError("evaluate needs at least one batch on every rank")
        if self.world > 1:
            if self.reducer.backend != "nccl":
                sums = sums.cpu()
            dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=self.reducer.group)
        loss_sum, denom, tokens, correct = sums.tolist()
        nan = float("nan")
        losses = [ls / d if d else nan for ls, d in zip(loss_sum, denom)]
        total = int(sum(tokens))
        out = dict(loss=sum(losses), accuracy=sum(correct) / total if total else nan, tokens=total)
        if len(tokens) > 1:
            out["per_channel"] = dict(loss=losses, accuracy=[c / t if t else nan for c, t in zip(correct, tokens)],
                                      tokens=[int(t) for t in tokens])
        return out

    def score(self, batches):
        """Per-utterance scores.  batches: an iterable of batch dicts, this rank's own (at least one);
        model.score per batch, the outputs concatenated on the device along the utterance axis, then ONE host read.  No collective:
        every rank gets the scores of what it submitted.  Returns a dict of numpy arrays with one entry per utterance in submission
        order ([channels, utterances] for a multi-channel head): loss_sum fp64, tokens, correct, worst_loss, worst_row (-1: no valid
        position) and mean_loss = loss_sum / max(tokens, 1).
        Like evaluate, it moves nothing of the run (eval mode under no_grad: no dropout draw, no gradient hook): parameters, masters,
        moments, step_idx, the learning rate, the flat gradient buffer, the NaN flag, the reducer's bucket bookkeeping, the host and
        device random streams and the train / eval mode are what they were -- k steps, score, m steps is bit-identical to k + m steps.
        Not allowed inside an accumulation window."""
        if self._acc_count != 0:
            raise RuntimeError(f"score inside an accumulation window ({self._acc_count} micro-batches pending): call step() first")
        per = [self.model.score(**batch) for batch in batches]
        if not per:
            raise ValueError("score needs at least one batch")
        keys = list(per[0])
        # one device tensor [5, ..., utterances] in fp64 (counts and rows are exact up to 2^53, an fp32 loss converts exactly): one read
        flat = torch.stack([torch.cat([p[k].double() for p in per], dim=-1) for k in keys]).cpu().numpy()
        out = {k: flat[i] if k == "loss_sum" else flat[i].astype("float32" if k == "worst_loss" else "int64") for i, k in enumerate(keys)}
        out["mean_loss"] = out["loss_sum"] / out["tokens"].clip(min=1)
        return out

    # ---- state digest and checkpoints ------------------------------------------------------------------
    def _own_range(self):
        """[lo, hi) of the flat buffers this rank is the authority on: its slab in shard mode, everything otherwise."""
        return self.reducer.slab(self.reducer.rank) if self.shard_optimizer else (0, self.flat.numel)

    def _range_digests(self, ranges):
        """[[master, exp_avg, exp_avg_sq, param digests as Python ints] for [lo, hi) in ranges], with global word indices (an
        fp32 element is a word, two bf16 elements are one).  HIP path: rwkv7_buf_digest_u32 per buffer and range, then ONE read-back;
        otherwise the numpy restatement.  With an fp32 model master IS flat_param: the two values are the same."""
        bufs = (self.master, self.exp_avg, self.exp_avg_sq, self.flat.flat_param)
        per_word = [4 // b.element_size() for b in bufs]
        if not self.hip_adamw:
            return [[_digest.fallback_digest(b[lo:hi], lo // k) for b, k in zip(bufs, per_word)] for lo, hi in ranges]
        if getattr(self, "_digest_ws", None) is None:
            self._digest_ws = _digest.workspace(self.flat.numel, self.master.device)
        out = torch.zeros(max(1, 4 * len(ranges)), dtype=torch.int64, device=self.master.device)
        for r, (lo, hi) in enumerate(ranges):
            for j, (b, k) in enumerate(zip(bufs, per_word)):
                _digest.launch(b[lo:hi], lo // k, out[4 * r + j:4 * r + j + 1], self._digest_ws)
        vals = [v & _digest.MASK64 for v in out.tolist()]
        return [vals[4 * r:4 * r + 4] for r in range(len(ranges))]

    def _combine_digests(self, own):
        """The four whole-buffer digests from every rank's `own` ones.  Replicated mode: they must be equal on all ranks (MIN and MAX
        of the 32-bit halves agree), RuntimeError naming the first buffer that differs otherwise.  Shard mode: the wrapping sum of
        the slab digests (the digest is additive over disjoint index ranges)."""
        r_ = self.reducer
        dev = self.master.device if r_.backend == "nccl" else torch.device("cpu")
        if self.shard_optimizer:
            mine = torch.tensor([v - (1 << 64) if v >> 63 else v for v in own], dtype=torch.int64, device=dev)
            everyone = [torch.zeros_like(mine) for _ in range(r_.world)]
            dist.all_gather(everyone, mine, group=r_.group)
            return [sum(int(t[j]) for t in everyone) & _digest.MASK64 for j in range(4)]
        halves = torch.tensor([h for v in own for h in (v & 0xffffffff, v >> 32)], dtype=torch.int64, device=dev)
        lo_, hi_ = halves.clone(), halves.clone()
        dist.all_reduce(lo_, op=dist.ReduceOp.MIN, group=r_.group)
        dist.all_reduce(hi_, op=dist.ReduceOp.MAX, group=r_.group)
        differ = (lo_ != hi_).reshape(4, 2).any(dim=1).tolist()
        if any(differ):
            name = DIGEST_NAMES[differ.index(True)]
            raise RuntimeError(f"replicas differ: the digest of `{name}` is not the same on all {r_.world} ranks (step {self.step_idx})")
        return list(own)

    def digest(self, all_ranks=False):
        """{"master", "exp_avg", "exp_avg_sq", "param"}: 64-bit digests (rwkvtts_amd/digest.py) of this rank's authoritative range of
        the fp32 masters, the two moments and the model-dtype parameters, with global indices; one host read-back.
        all_ranks=True (a collective when world > 1): replicated mode checks that every rank holds the same four words and raises
        RuntimeError naming the buffer if not; shard mode returns the digests of the WHOLE buffers, summed from the slabs."""
        own = self._range_digests([self._own_range()])[0]
        if all_ranks and self.world > 1:
            own = self._combine_digests(own)
        return dict(zip(DIGEST_NAMES, own))

    def _layout(self):
        names = {id(p): n for n, p in self.model.named_parameters()}
        return [dict(name=names.get(id(p), f"<parameter {i}>"), shape=list(p.shape), offset=o, numel=p.numel())
                for i, (p, o) in enumerate(zip(self.flat.params, self.flat.offsets))]

    def _barrier(self):
        if self.world > 1:
            dist.barrier(group=self.reducer.group)

    def _checkpoint_job(self, tag, extra_json, own, whole):
        """Everything this rank's checkpoint files hold besides the tensors, taken NOW: the range and its file names, the JSON texts
        (already encoded), the host and device RNG states."""
        rank, world = self.reducer.rank, self.world
        lo, hi = self._own_range()
        hexd = lambda vals: {n: "%016x" % v for n, v in zip(DIGEST_NAMES, vals)}
        same = self.master is self.flat.flat_param
        stem = f"range_{lo:012d}_{hi:012d}"
        files = {}
        if (rank == 0 or self.shard_optimizer) and hi > lo:
            files = {name: f"{stem}.{name}.bin" for name in DIGEST_NAMES if not (name == "param" and same)}
        rng = {"cpu": torch.get_rng_state()}
        if self.master.is_cuda:
            rng["cuda"] = torch.cuda.get_rng_state(self.master.device)
        meta_json = None
        if rank == 0:
            ranges = [self.reducer.slab(r) for r in range(world)] if self.shard_optimizer else [(0, self.flat.numel)]
            sched = [k for k, v in SCHEDULES.items() if v is self.schedule]
            meta = dict(format=CHECKPOINT_FORMAT, step_idx=self.step_idx, last_lr=self.last_lr, world=world,
                        shard_optimizer=self.shard_optimizer, numel=self.flat.numel,
                        param_dtype=str(self.flat.flat_param.dtype), master_dtype=str(self.master.dtype),
                        ranges=[list(r) for r in ranges if r[1] > r[0]], digest=hexd(whole), layout=self._layout(),
                        group_defs=[list(g) for g in self.group_defs],
                        hyper=dict(lr=self.lr, lr_final=self.lr_final, warmup_steps=self.warmup_steps, total_steps=self.total_steps,
                                   weight_decay=self.weight_decay, betas=list(self.betas), eps=self.eps,
                                   max_grad_norm=self.max_grad_norm, nan_guard=self.nan_guard,
                                   schedule=sched[0] if sched else repr(self.schedule)),
                        extra=json.loads(extra_json))
            meta_json = json.dumps(meta, indent=1).encode()
        return dict(rank=rank, stem=stem, files=files, rng=rng, meta_json=meta_json,
                    range_json=json.dumps(dict(lo=lo, hi=hi, rank=rank, files=files, digest=hexd(own)), indent=1).encode())

    def _checkpoint_open(self, dir, tmp):
        """Rank 0 creates <tag>.tmp/ (a stale one is removed first); nobody writes before it exists."""
        if self.reducer.rank == 0:
            os.makedirs(dir, exist_ok=True)
            if os.path.isdir(tmp):
                shutil.rmtree(tmp)
            os.makedirs(tmp)
        self._barrier()

    def _checkpoint_finish(self, dir, tag, keep_last):
        """Every rank's files are written and fsynced: rename, `latest`, stale .tmp directories, keep_last.  Returns the final path."""
        tmp, final = os.path.join(dir, tag + ".tmp"), os.path.join(dir, tag)
        self._barrier()
        if self.reducer.rank == 0:
            _sync_dir(tmp)
            if os.path.isdir(final):
                shutil.rmtree(final)
            os.rename(tmp, final)
            _write_synced(os.path.join(dir, "latest.new"), tag.encode())
            os.replace(os.path.join(dir, "latest.new"), os.path.join(dir, "latest"))
            _sync_dir(dir)
            for d in os.listdir(dir):   # saves that never finished
                if d.endswith(".tmp") and os.path.isdir(os.path.join(dir, d)):
                    shutil.rmtree(os.path.join(dir, d), ignore_errors=True)
            if keep_last:
                old = [t for _, t in complete_checkpoints(dir) if t != tag]
                for t in old[:max(0, len(old) - (int(keep_last) - 1))]:
                    shutil.rmtree(os.path.join(dir, t), ignore_errors=True)
        self._barrier()
        return final

    def save_checkpoint(self, dir, tag=None, extra=None, keep_last=3, blocking=True):
        """Write the training state to <dir>/<tag>/ (tag: "step_<step_idx>" by default) and return that path; what the reference
        scripts ask of `model_engine.save_checkpoint(output_dir)` (train_scripts/train_spark_rwkv7speech.py:199-217, 695, 734).
        A collective when world > 1: every rank calls it with the same arguments, on a directory all ranks can see.

        Written: the fp32 masters and both moments, the model-dtype flat parameters (so that no rounding has to be reproduced),
        step_idx and last_lr, the layout (names, shapes, offsets), group_defs and the hyper-parameters (for information), one digest
        per buffer and written range, `extra` (JSON: epoch, batch index, data cursor) and every rank's host and device RNG state.
        Not written: gradients, the fp32 micro-batch accumulator -- saving inside an accumulation window is a RuntimeError.
        Replicated mode: rank 0 writes the tensors, after the digests have shown the replicas to be identical; shard mode: every
        rank writes its own slab (foreign slabs of the masters and moments are stale on a rank).
        Everything goes to <dir>/<tag>.tmp/, every file is fsynced by its writer; after a barrier rank 0 renames the directory,
        rewrites <dir>/latest and deletes the oldest complete checkpoints beyond keep_last (None: keep all) and stale .tmp directories.
        blocking=True: one device synchronisation and device-to-host copies on the calling thread; nothing of step() changes.

        blocking=False: the call returns the path the checkpoint WILL have once checkpoint_wait() has finalised it.  On the calling
        thread: the same checks; a save still pending is finalised first (one in flight at a time, finalised in the order started);
        the rank's range of the four buffers is copied into staging buffers of the same dtype and length on the current stream, each
        by the one kernel pass that also digests the words it writes (rwkv7_buf_snapshot_digest_u32; host tensors: a copy and the
        numpy digest), so later step() calls cannot reach what is saved; the four digests are read back -- the one device
        synchronisation -- and, with several ranks, compared or combined as in the blocking save, so diverged replicas raise before
        anything is written; RNG states, step_idx, last_lr, layout and hyper-parameters are captured; <tag>.tmp/ is created.  One
        writer thread (not a daemon) then waits for the snapshot on a side stream of its own, copies the staging to the host
        through two pinned buffers of CHECKPOINT_PIECE_BYTES used alternately, and writes and fsyncs the very files, names and bytes
        the blocking save writes.  It touches no trainer state and issues no collective.  step() and accumulate() neither wait for it nor
        finalise it.  The staging buffers are kept for the next save (release_checkpoint_staging() frees them).  Until
        checkpoint_wait() -- or the next save_checkpoint / load_checkpoint on this trainer, which call it -- the checkpoint is not a
        candidate for loading: if the process exits without it, the files may all be complete, but <tag>.tmp/ is never renamed."""
        if self._acc_count != 0:
            raise RuntimeError(f"save_checkpoint inside an accumulation window ({self._acc_count} micro-batches pending): "
                               "checkpoints are taken at step boundaries, the fp32 accumulator is not serialised")
        extra_json = json.dumps(extra)   # not JSON-serialisable: TypeError before anything is written
        tag = f"step_{self.step_idx}" if tag is None else str(tag)
        if not tag or tag.endswith(".tmp") or tag == "latest" or os.path.basename(tag) != tag:
            raise ValueError(f"bad checkpoint tag {tag!r}")
        self.checkpoint_wait()
        world = self.world
        tmp, final = os.path.join(dir, tag + ".tmp"), os.path.join(dir, tag)
        lo, hi = self._own_range()
        bufs = dict(zip(DIGEST_NAMES, (self.master, self.exp_avg, self.exp_avg_sq, self.flat.flat_param)))
        if blocking:
            own = self._range_digests([(lo, hi)])[0]
            whole = self._combine_digests(own) if world > 1 else own   # replicated mode: raises if the replicas have diverged
            self._checkpoint_open(dir, tmp)
            _write_checkpoint_files(tmp, self._checkpoint_job(tag, extra_json, own, whole),
                                    lambda name: bufs[name][lo:hi].detach().cpu().view(torch.uint8).numpy())
            return self._checkpoint_finish(dir, tag, keep_last)
        own, stream, event = self._snapshot(bufs, lo, hi)
        whole = self._combine_digests(own) if world > 1 else own
        job = self._checkpoint_job(tag, extra_json, own, whole)
        self._checkpoint_open(dir, tmp)
        staged = self._ckpt_staging
        if stream is None:
            payload = lambda name: staged["bufs"][name].view(torch.uint8).numpy()
        else:
            payload = lambda name: _staged_pieces(staged["bufs"][name], staged["pinned"], stream)
        p = PendingCheckpoint(dir, tag, final, self.step_idx, dict(zip(DIGEST_NAMES, own)), keep_last)
        p.thread = threading.Thread(target=_checkpoint_writer, args=(p, tmp, job, payload, stream, event),
                                    name=f"checkpoint-writer-{tag}", daemon=False)
        self._pending = p
        p.thread.start()
        return final

    def _snapshot(self, bufs, lo, hi):
        """[lo, hi) of the four state buffers into the staging buffers (allocated on first use: the same dtype and length as the
        range; on the HIP path also the writer's side stream and its two pinned buffers), and the four digests of what was written,
        with global word indices as _range_digests computes them.  HIP path: four rwkv7_buf_snapshot_digest_u32 calls on the current
        stream, an event behind them, ONE read-back; returns (digests, side stream, event).  Otherwise host staging tensors and the
        numpy restatement; returns (digests, None, None).  With an fp32 model master IS flat_param: one staging buffer, one value."""
        same = self.master is self.flat.flat_param
        if self._ckpt_staging is None:
            dev = self.master.device if self.hip_adamw else torch.device("cpu")
            st = dict(bufs={name: torch.empty(hi - lo, dtype=b.dtype, device=dev) for name, b in bufs.items()
                            if not (name == "param" and same)})
            if self.hip_adamw:
                st["stream"] = torch.cuda.Stream(dev)
                st["pinned"] = [torch.empty(CHECKPOINT_PIECE_BYTES, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
            self._ckpt_staging = st
        st = self._ckpt_staging
        per_word = {name: 4 // b.element_size() for name, b in bufs.items()}
        if not self.hip_adamw:
            own = {name: _digest.snapshot_digest(bufs[name][lo:hi].detach(), dst, lo // per_word[name]) for name, dst in st["bufs"].items()}
            return [own["master" if same and name == "param" else name] for name in DIGEST_NAMES], None, None
        if getattr(self, "_digest_ws", None) is None:
            self._digest_ws = _digest.workspace(self.flat.numel, self.master.device)
        out = torch.zeros(4, dtype=torch.int64, device=self.master.device)
        for j, name in enumerate(DIGEST_NAMES):
            _digest.snapshot_launch(bufs[name][lo:hi], st["bufs"][name], lo // per_word[name], out[j:j + 1], self._digest_ws)
        event = torch.cuda.Event()
        event.record()
        return [v & _digest.MASK64 for v in out.tolist()], st["stream"], event

    @property
    def pending_checkpoint(self):
        """None, or the PendingCheckpoint of the non-blocking save that checkpoint_wait() has not finalised yet."""
        return self._pending

    def checkpoint_done(self):
        """True when no save is pending or THIS rank's writer thread has finished.  Local: no collective, no waiting."""
        return self._pending is None or not self._pending.thread.is_alive()

    def checkpoint_wait(self):
        """Finalise the pending non-blocking save and return its path; None when nothing is pending.  A collective when world > 1.
        Joins the writer thread; the ranks agree on whether any writer failed (all-reduce MAX of a flag).  All succeeded: the tail of
        the blocking save in its order -- barrier, rank 0 fsyncs and renames the directory, rewrites `latest`, removes stale .tmp
        directories, prunes to keep_last, barrier.  Any failed: rank 0 removes <tag>.tmp/, `latest` and every complete checkpoint stay
        as they were, and EVERY rank raises RuntimeError naming the tag, chained to the writer's exception on the rank that has it.
        Either way nothing is pending afterwards and the trainer stays usable."""
        p = self._pending
        if p is None:
            return None
        p.thread.join()
        self._pending = None
        failed = p.error is not None
        if self.world > 1:
            r_ = self.reducer
            flag = torch.tensor([int(failed)], dtype=torch.int32, device=self.master.device if r_.backend == "nccl" else "cpu")
            dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=r_.group)
            failed = bool(flag.item())
        if not failed:
            return self._checkpoint_finish(p.dir, p.tag, p.keep_last)
        if self.reducer.rank == 0:   # every writer has been joined: nobody writes into it any more
            shutil.rmtree(os.path.join(p.dir, p.tag + ".tmp"), ignore_errors=True)
        self._barrier()
        where = "on this rank" if p.error is not None else "on another rank"
        raise RuntimeError(f"checkpoint {p.tag!r}: the writer failed {where}; nothing was renamed, "
                           f"`latest` and the complete checkpoints in {p.dir} are unchanged") from p.error

    def release_checkpoint_staging(self):
        """Free the staging buffers of the non-blocking saves (and the pinned buffers and side stream of the HIP path); the next
        non-blocking save allocates them again.  RuntimeError while a save is pending: call checkpoint_wait() first."""
        if self._pending is not None:
            raise RuntimeError(f"checkpoint {self._pending.tag!r} is pending: checkpoint_wait() before releasing its staging buffers")
        self._ckpt_staging = None

    def load_checkpoint(self, dir, tag=None):
        """Restore what save_checkpoint wrote into this FRESHLY constructed trainer (a model of the same architecture) and return
        the saved `extra`.  tag=None: the tag named by <dir>/latest.  Every rank reads the whole checkpoint (a collective only in
        that all ranks are expected to call it).

        The stored layout (names, shapes, offsets, numel, dtypes) must be this trainer's: ValueError naming the first parameter that
        differs, with model and trainer untouched.  The full buffers are assembled from whatever range files the checkpoint has --
        a sharded 2-rank checkpoint loads into one rank and the other way round -- and copied INTO the existing flat buffers: the
        parameters stay views of flat_param.  step_idx and last_lr are set, the modules' parameter-derived caches invalidated.  Then
        the digest of every stored range is recomputed from the buffers (the kernel on the HIP path) and compared with the stored
        one: RuntimeError naming the buffer on a mismatch -- a truncated or corrupted file and a bad copy alike.
        RNG: this rank's host and device states are restored if the checkpoint has them for this rank and the world size is
        unchanged; otherwise they are left alone, with a warning.  Schedule, parameter groups and the clip threshold are the new
        trainer's own (a differing stored group table is a warning); the reducer discovers its buckets again as on any fresh trainer.
        A non-blocking save pending on THIS trainer is finalised first (checkpoint_wait())."""
        self.checkpoint_wait()
        if tag is None:
            try:
                with open(os.path.join(dir, "latest")) as f:
                    tag = f.read().strip()
            except OSError:
                raise FileNotFoundError(f"{dir}: no `latest` file, no checkpoint to resume from") from None
        path = os.path.join(dir, tag)
        if tag.endswith(".tmp") or not os.path.isfile(os.path.join(path, "meta.json")):
            raise FileNotFoundError(f"{path} is not a complete checkpoint")
        meta = _read_json(os.path.join(path, "meta.json"))
        if meta.get("format") != CHECKPOINT_FORMAT:
            raise ValueError(f"{path}: checkpoint format {meta.get('format')!r}, this trainer reads {CHECKPOINT_FORMAT}")
        mine = self._layout()
        for a, b in zip(meta["layout"], mine):
            if a != b:
                raise ValueError(f"{path}: parameter `{b['name']}` is {b['shape']} at offset {b['offset']} here, the checkpoint has "
                                 f"`{a['name']}` {a['shape']} at offset {a['offset']}")
        if len(meta["layout"]) != len(mine) or meta["numel"] != self.flat.numel:
            longer = meta["layout"] if len(meta["layout"]) > len(mine) else mine
            raise ValueError(f"{path}: {len(meta['layout'])} parameters in the checkpoint, {len(mine)} here (first without a partner: "
                             f"`{longer[min(len(meta['layout']), len(mine))]['name']}`)")
        if meta["param_dtype"] != str(self.flat.flat_param.dtype) or meta["master_dtype"] != str(self.master.dtype):
            raise ValueError(f"{path}: stored as {meta['param_dtype']} parameters with {meta['master_dtype']} masters, this trainer "
                             f"holds {self.flat.flat_param.dtype} with {self.master.dtype}")
        ranges = sorted(tuple(r) for r in meta["ranges"])
        if not ranges or ranges[0][0] != 0 or ranges[-1][1] != self.flat.numel or any(a[1] != b[0] for a, b in zip(ranges, ranges[1:])):
            raise RuntimeError(f"{path}: the stored ranges {ranges} do not tile [0, {self.flat.numel})")
        same = self.master is self.flat.flat_param
        bufs = dict(zip(DIGEST_NAMES, (self.master, self.exp_avg, self.exp_avg_sq, self.flat.flat_param)))
        todo, stored = [], []
        for lo, hi in ranges:   # everything that can be checked on the host before a buffer is touched
            rj = os.path.join(path, f"range_{lo:012d}_{hi:012d}.json")
            if not os.path.isfile(rj):
                raise RuntimeError(f"{path}: the file of range [{lo}, {hi}) is missing")
            info = _read_json(rj)
            if (info["lo"], info["hi"]) != (lo, hi):
                raise RuntimeError(f"{rj} describes [{info['lo']}, {info['hi']})")
            stored.append([int(info["digest"][n], 16) for n in DIGEST_NAMES])
            for name, buf in bufs.items():
                if name == "param" and same:
                    continue
                f = os.path.join(path, info["files"][name])
                want = (hi - lo) * buf.element_size()
                if not os.path.isfile(f) or os.path.getsize(f) != want:
                    raise RuntimeError(f"{path}: `{name}` of range [{lo}, {hi}) is missing or truncated "
                                       f"({os.path.getsize(f) if os.path.isfile(f) else 0} bytes, {want} expected)")
                todo.append((f, buf, lo, hi))
        import numpy as np
        with torch.no_grad():
            for f, buf, lo, hi in todo:
                buf[lo:hi].copy_(torch.from_numpy(np.fromfile(f, dtype=np.uint8)).view(buf.dtype))
        self.step_idx, self.last_lr = int(meta["step_idx"]), meta["last_lr"]
        self._acc_count = 0
        for m in self._param_caches:
            m._mix_key = None
        for (lo, hi), want, got in zip(ranges, stored, self._range_digests(ranges)):
            for name, w, g in zip(DIGEST_NAMES, want, got):
                if w != g:
                    raise RuntimeError(f"{path}: digest mismatch in `{name}`, range [{lo}, {hi}): stored {w:016x}, in memory after "
                                       f"the load {g:016x} -- a corrupted file or a bad copy")
        rng_file = os.path.join(path, f"rng_rank{self.reducer.rank}.pt")
        if meta["world"] == self.world and os.path.isfile(rng_file):
            rng = torch.load(rng_file, map_location="cpu", weights_only=True)
            torch.set_rng_state(rng["cpu"])
            if "cuda" in rng and self.master.is_cuda:
                torch.cuda.set_rng_state(rng["cuda"], self.master.device)
            elif self.master.is_cuda:
                warnings.warn(f"{path}: no device RNG state for rank {self.reducer.rank}; the device generator is left as it is")
        else:
            warnings.warn(f"{path}: saved by {meta['world']} rank(s), loaded by {self.world}: the RNG states are left as they are")
        if [list(g) for g in self.group_defs] != meta["group_defs"]:
            warnings.warn(f"{path}: the stored parameter groups {meta['group_defs']} differ from this trainer's "
                          f"{[list(g) for g in self.group_defs]}; this trainer's are used")
        return meta["extra"]
