"""CPU: DataParallelTrainer.save_checkpoint(blocking=False) / checkpoint_wait / checkpoint_done / pending_checkpoint on the toy fp32
network of test_trainer_dist.py (host staging tensors and the numpy digest; the protocol -- the snapshot, the writer thread, who
finalises what and when -- is the same code as on the GPU).

The guarantee: a non-blocking save at step K holds the state AT STEP K whatever the trainer does while the writer runs.  The writer
is held inside trainer._write_synced by a threading.Event, so "while the writer runs" does not depend on timing."""
import json
import os
import threading

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from rwkvtts_amd import digest, trainer
from test_trainer_checkpoint import K, LR, M, _advance, _assert_same_state, _other_init, _state, ref_digest
from test_trainer_dist import Toy, _data, _free_port


class Gate:
    """trainer._write_synced replaced: every call first waits until `release` is set (`entered` tells that a call has arrived), and
    call number `fail_on` (1-based) raises OSError instead of writing."""

    def __init__(self, monkeypatch, fail_on=None, held=True):
        self.release, self.entered, self.calls = threading.Event(), threading.Event(), 0
        if not held:
            self.release.set()
        real = trainer._write_synced

        def gated(path, data):
            self.entered.set()
            assert self.release.wait(120), "the test never released the writer"
            self.calls += 1
            if self.calls == fail_on:
                raise OSError(28, "No space left on device", path)
            return real(path, data)

        monkeypatch.setattr(trainer, "_write_synced", gated)


def _hex(d):
    return {k: "%016x" % v for k, v in d.items()}


def _same_files(a, b):
    """Two checkpoint directories hold the same files: every .bin and .json byte for byte, the RNG files by their tensors."""
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and "meta.json" in names and any(n.endswith(".bin") for n in names)
    for n in names:
        if n.endswith(".pt"):
            ra, rb = (torch.load(os.path.join(d, n), weights_only=True) for d in (a, b))
            assert sorted(ra) == sorted(rb) and all(torch.equal(ra[k], rb[k]) for k in ra), n
        else:
            with open(os.path.join(a, n), "rb") as fa, open(os.path.join(b, n), "rb") as fb:
                assert fa.read() == fb.read(), n


@pytest.mark.parametrize("earlier", [False, True], ids=["first-save", "after-an-earlier-save"])
def test_held_writer_saves_the_state_at_step_k_and_the_run_resumes_from_it(earlier, tmp_path, monkeypatch):
    ta = trainer.DataParallelTrainer(Toy(), **LR)
    _advance(ta, 0, range(K + M))
    tb = trainer.DataParallelTrainer(Toy(), **LR)
    _advance(tb, 0, [0])
    if earlier:
        tb.save_checkpoint(str(tmp_path))                       # step_1, complete
    _advance(tb, 0, range(1, K))
    at_k, digest_k = _state(tb), tb.digest()
    gate = Gate(monkeypatch)
    extra = {"epoch": 3, "cursor": [1, 2, {"shard": "a"}]}
    path = tb.save_checkpoint(str(tmp_path), extra=extra, blocking=False)
    assert path == str(tmp_path / f"step_{K}")
    _advance(tb, 0, range(K, K + M))                            # M more steps while the writer is held
    assert gate.entered.wait(120) and gate.calls == 0
    assert (tmp_path / f"step_{K}.tmp").is_dir() and not (tmp_path / f"step_{K}").exists()
    assert (tmp_path / "latest").read_text() == "step_1" if earlier else not (tmp_path / "latest").exists()
    p = tb.pending_checkpoint
    assert not tb.checkpoint_done() and (p.step_idx, p.tag, p.path, p.digests) == (K, f"step_{K}", path, digest_k)
    gate.release.set()
    assert tb.checkpoint_wait() == path
    assert not (tmp_path / f"step_{K}.tmp").exists() and (tmp_path / f"step_{K}" / "meta.json").is_file()
    assert (tmp_path / "latest").read_text() == f"step_{K}"
    assert tb.pending_checkpoint is None and tb.checkpoint_done() and tb.checkpoint_wait() is None
    _assert_same_state(_state(ta), _state(tb))                  # the save did not disturb the run it was taken from
    mc = _other_init(Toy())
    tc = trainer.DataParallelTrainer(mc, **LR)
    assert not torch.equal(tc.master, at_k["master"])
    assert tc.load_checkpoint(str(tmp_path)) == extra
    _assert_same_state(at_k, _state(tc))                        # the state at step K, not at K + M
    meta = json.loads((tmp_path / f"step_{K}" / "meta.json").read_text())
    assert meta["digest"] == _hex(digest_k) == _hex(tc.digest()) and meta["step_idx"] == K
    _advance(tc, 0, range(K, K + M))
    _assert_same_state(_state(ta), _state(tc))


def test_files_equal_those_of_a_blocking_save_of_the_same_state(tmp_path):
    tr = trainer.DataParallelTrainer(Toy(), **LR)
    _advance(tr, 0, range(K))
    extra = {"cursor": 5}
    tr.save_checkpoint(str(tmp_path / "a"), tag="x", extra=extra, blocking=False)
    assert tr.checkpoint_wait() == str(tmp_path / "a" / "x")
    tr.save_checkpoint(str(tmp_path / "b"), tag="x", extra=extra)
    _same_files(str(tmp_path / "a" / "x"), str(tmp_path / "b" / "x"))


def test_a_second_save_finalises_the_first_and_keep_last_prunes_in_order(tmp_path):
    tr = trainer.DataParallelTrainer(Toy(), **LR)
    for step in range(3):
        _advance(tr, 0, [step])
        tr.save_checkpoint(str(tmp_path), keep_last=2, blocking=False)
        assert tr.pending_checkpoint.tag == f"step_{step + 1}"
        if step:                                                # the earlier save was finalised before this one started
            assert (tmp_path / "latest").read_text() == f"step_{step}" and (tmp_path / f"step_{step}" / "meta.json").is_file()
    tr.checkpoint_wait()
    assert sorted(p.name for p in tmp_path.iterdir()) == ["latest", "step_2", "step_3"]
    assert (tmp_path / "latest").read_text() == "step_3"
    assert trainer.complete_checkpoints(str(tmp_path)) == [(2, "step_2"), (3, "step_3")]


def test_writer_failure_raises_in_checkpoint_wait_and_leaves_everything_as_it_was(tmp_path, monkeypatch):
    tr = trainer.DataParallelTrainer(Toy(), **LR)
    _advance(tr, 0, [0])
    tr.save_checkpoint(str(tmp_path))                           # step_1: the earlier checkpoint
    at_1 = _state(tr)
    _advance(tr, 0, range(1, K))
    before = _state(tr)
    with monkeypatch.context() as mp_:
        gate = Gate(mp_, fail_on=2, held=False)                 # the second file cannot be written
        tr.save_checkpoint(str(tmp_path), blocking=False)
        with pytest.raises(RuntimeError, match=f"step_{K}") as e:
            tr.checkpoint_wait()
        assert isinstance(e.value.__cause__, OSError) and gate.calls == 2
    assert sorted(p.name for p in tmp_path.iterdir()) == ["latest", "step_1"]
    assert (tmp_path / "latest").read_text() == "step_1"
    t2 = trainer.DataParallelTrainer(_other_init(Toy()), **LR)
    t2.load_checkpoint(str(tmp_path))
    _assert_same_state(at_1, _state(t2))
    _assert_same_state(before, _state(tr))                      # the trainer's buffers are untouched ...
    assert tr.pending_checkpoint is None and tr.checkpoint_wait() is None
    _advance(tr, 0, [K])                                        # ... it steps ...
    path = tr.save_checkpoint(str(tmp_path), blocking=False)    # ... and saves
    assert tr.checkpoint_wait() == path and (tmp_path / "latest").read_text() == f"step_{K + 1}"
    t2 = trainer.DataParallelTrainer(_other_init(Toy()), **LR)
    t2.load_checkpoint(str(tmp_path))
    _assert_same_state(_state(tr), _state(t2))


def test_blocking_save_and_load_finalise_a_pending_save_first(tmp_path):
    tr = trainer.DataParallelTrainer(Toy(), **LR)
    _advance(tr, 0, range(K))
    at_k = _state(tr)
    tr.save_checkpoint(str(tmp_path), tag="a", blocking=False)
    _advance(tr, 0, [K])
    tr.save_checkpoint(str(tmp_path), tag="b")                  # blocking: `a` is finalised, then `b` written
    assert tr.pending_checkpoint is None and (tmp_path / "latest").read_text() == "b"
    assert [t for _, t in trainer.complete_checkpoints(str(tmp_path))] == ["a", "b"]
    tr.save_checkpoint(str(tmp_path), tag="c", blocking=False)
    _advance(tr, 0, [K + 1])
    tr.load_checkpoint(str(tmp_path), tag="a")                  # finalises `c` first, then loads `a` into this trainer
    assert tr.pending_checkpoint is None and (tmp_path / "latest").read_text() == "c" and (tmp_path / "c" / "meta.json").is_file()
    _assert_same_state(at_k, _state(tr))


def test_the_earlier_checks_hold_without_blocking_too(tmp_path):
    tr = trainer.DataParallelTrainer(Toy(), **LR)
    x, y = _data(0, 0)
    tr.accumulate(x=x, y=y)
    with pytest.raises(RuntimeError, match="accumulation window"):
        tr.save_checkpoint(str(tmp_path / "ck"), blocking=False)
    tr.step(x=x, y=y)
    for tag in ("", "x.tmp", "latest", "a/b"):
        with pytest.raises(ValueError, match="bad checkpoint tag"):
            tr.save_checkpoint(str(tmp_path / "ck"), tag=tag, blocking=False)
    with pytest.raises(TypeError):
        tr.save_checkpoint(str(tmp_path / "ck"), extra={"t": torch.zeros(1)}, blocking=False)
    assert not (tmp_path / "ck").exists() and tr.pending_checkpoint is None and tr._ckpt_staging is None


def test_nothing_pending_and_the_staging_buffers(tmp_path, monkeypatch):
    tr = trainer.DataParallelTrainer(Toy(), **LR)
    assert tr.checkpoint_wait() is None and tr.checkpoint_done() and tr.pending_checkpoint is None
    tr.release_checkpoint_staging()                             # nothing allocated yet: fine
    _advance(tr, 0, [0])
    gate = Gate(monkeypatch)
    tr.save_checkpoint(str(tmp_path), blocking=False)
    staged = tr._ckpt_staging["bufs"]
    assert sorted(staged) == ["exp_avg", "exp_avg_sq", "master"]            # fp32 model: master IS flat_param, one buffer
    assert all(b.dtype == tr.master.dtype and b.numel() == tr.flat.numel and b.data_ptr() != tr.master.data_ptr() for b in staged.values())
    with pytest.raises(RuntimeError, match="pending"):
        tr.release_checkpoint_staging()
    gate.release.set()
    tr.checkpoint_wait()
    _advance(tr, 0, [1])
    tr.save_checkpoint(str(tmp_path), blocking=False)
    assert tr._ckpt_staging["bufs"]["master"] is staged["master"], "the staging buffers are kept and reused"
    tr.checkpoint_wait()
    tr.release_checkpoint_staging()
    assert tr._ckpt_staging is None
    _advance(tr, 0, [2])
    tr.save_checkpoint(str(tmp_path), blocking=False)           # allocated again
    assert tr.checkpoint_wait() == str(tmp_path / "step_3")
    t2 = trainer.DataParallelTrainer(_other_init(Toy()), **LR)
    t2.load_checkpoint(str(tmp_path))
    _assert_same_state(_state(tr), _state(t2))


def test_snapshot_digest_on_host_tensors():
    g = torch.Generator().manual_seed(0)
    f = torch.randn(257, generator=g)
    dst = torch.full_like(f, 7.0)
    assert digest.snapshot_digest(f, dst, 3) == digest.fallback_digest(f, 3) == ref_digest(f.numpy().view(np.uint32), 3)
    assert np.array_equal(dst.numpy().view(np.uint32), f.numpy().view(np.uint32))
    b = torch.randn(512, generator=g).bfloat16()
    b.view(torch.int16)[:2] = torch.tensor([0x7fc0, 0x7f80], dtype=torch.int16)      # a NaN and an Inf: copied as bits
    dst = torch.zeros_like(b)
    assert digest.snapshot_digest(b[64:192], dst[:128], 32) == digest.fallback_digest(b[64:192], 32)
    assert torch.equal(dst[:128].view(torch.int16), b[64:192].view(torch.int16)) and not dst[128:].any()
    assert digest.snapshot_digest(b, dst) == ref_digest(b.view(torch.int16).numpy().view(np.uint32))
    assert torch.equal(dst.view(torch.int16), b.view(torch.int16))
    with pytest.raises(ValueError):
        digest.snapshot_digest(b, torch.zeros(512))             # another dtype


def test_write_synced_takes_pieces(tmp_path):
    pieces = [np.arange(5, dtype=np.uint8), np.zeros(0, np.uint8), np.arange(250, 256, dtype=np.uint8)]
    trainer._write_synced(str(tmp_path / "f"), iter(pieces))
    assert (tmp_path / "f").read_bytes() == bytes([0, 1, 2, 3, 4, 250, 251, 252, 253, 254, 255])


# ---- two gloo ranks --------------------------------------------------------------------------------------------------------------
def _own(tr):
    lo, hi = tr._own_range()
    out = {n: getattr(tr, n)[lo:hi].numpy().copy() for n in ("master", "exp_avg", "exp_avg_sq")}
    out["param"] = tr.flat.flat_param[lo:hi].numpy().copy()
    return out


def _worker(rank, world, port, q, shard, d, fail_rank):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    trainer.init_distributed("gloo")
    torch.set_num_threads(1)
    tb = trainer.DataParallelTrainer(Toy(), bucket_bytes=4096, shard_optimizer=shard, **LR)
    _advance(tb, rank, [0])
    tb.save_checkpoint(d)                                       # step_1: the earlier checkpoint
    _advance(tb, rank, range(1, K))
    at_k, whole_k = _own(tb), tb.digest(all_ranks=True)
    if rank == fail_rank:
        def refuse(path, data):
            raise OSError(28, "No space left on device", path)
        trainer._write_synced = refuse
    tb.save_checkpoint(d, extra={"cursor": 5}, blocking=False)
    _advance(tb, rank, range(K, K + M))
    raised = cause = None
    try:
        tb.checkpoint_wait()
    except RuntimeError as e:
        raised, cause = str(e), type(e.__cause__).__name__
    q.put((rank, tb._own_range(), at_k, whole_k, _own(tb), (tb.step_idx, tb.last_lr), raised, cause, tb.pending_checkpoint is None))
    dist.barrier()
    dist.destroy_process_group()


def _run_two(shard, d, fail_rank=None):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, shard, d, fail_rank)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    return res


@pytest.mark.timeout(300)
@pytest.mark.parametrize("shard", [False, True], ids=["allreduce", "shard"])
def test_two_ranks_save_without_blocking_and_one_rank_continues_their_run(shard, tmp_path):
    d = str(tmp_path)
    res = _run_two(shard, d)
    assert all(r[6] is None and r[8] for r in res)
    assert (tmp_path / "latest").read_text() == f"step_{K}" and not (tmp_path / f"step_{K}.tmp").exists()
    gathered = lambda i, name: torch.cat([torch.from_numpy(r[i][name]) for r in (res if shard else res[:1])])
    t1 = trainer.DataParallelTrainer(_other_init(Toy()), **LR)
    with pytest.warns(UserWarning, match="RNG"):
        assert t1.load_checkpoint(d) == {"cursor": 5}
    bufs = lambda: (("master", t1.master), ("exp_avg", t1.exp_avg), ("exp_avg_sq", t1.exp_avg_sq), ("param", t1.flat.flat_param))
    for name, buf in bufs():
        assert torch.equal(buf, gathered(2, name)), name      # the two ranks' state at step K, not at K + M
    assert t1.digest() == res[0][3] == res[1][3] and t1.step_idx == K
    assert _hex(t1.digest()) == json.loads((tmp_path / f"step_{K}" / "meta.json").read_text())["digest"]
    # one rank continues the two-rank run: the mean of two fp32 gradients is the same number whether a collective forms it
    # (sum, then / 2) or the micro-batch accumulator does (sum, then * 0.5)
    for step in range(K, K + M):
        t1.accumulate(**dict(zip("xy", _data(0, step))))
        t1.step(**dict(zip("xy", _data(1, step))))
    for name, buf in bufs():
        assert torch.equal(buf, gathered(4, name)), name
    assert (t1.step_idx, t1.last_lr) == res[0][5] == res[1][5]


@pytest.mark.timeout(300)
def test_a_writer_failure_on_one_rank_raises_on_both(tmp_path):
    res = _run_two(True, str(tmp_path), fail_rank=1)
    assert all(r[6] is not None and f"step_{K}" in r[6] and r[8] for r in res), "checkpoint_wait() must raise on every rank"
    assert [r[7] for r in res] == ["NoneType", "OSError"]      # chained to the writer's exception on the rank that has it
    assert sorted(p.name for p in tmp_path.iterdir()) == ["latest", "step_1"]
    assert (tmp_path / "latest").read_text() == "step_1"
    t1 = trainer.DataParallelTrainer(_other_init(Toy()), **LR)
    with pytest.warns(UserWarning, match="RNG"):
        t1.load_checkpoint(str(tmp_path))
    assert t1.step_idx == 1
