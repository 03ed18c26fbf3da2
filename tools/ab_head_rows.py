"""Same-process A/B of the three loss-head row kernels (csrc/head_loss.hip) between two builds of librwkv7_hip.so: the parent commit's
and this tree's, both loaded into ONE process with ctypes.CDLL and typed from include/rwkv7_hip.h as rwkvtts_amd/_lib.py types them.

    python tools/ab_head_rows.py --old tools/ab/librwkv7_hip_parent.so [--new rwkvtts_amd/lib/librwkv7_hip.so]
                                 [--step bits|time0|time1|time2] [--out profiles/head_rows_ab.txt]
Build the parent's library from a checkout of the parent commit (python -m rwkvtts_amd.build --force) and copy it aside.  Without
--step every step runs in turn; a job that wants each step under its own time limit runs one invocation per step
(timeout ... --step bits && timeout ... --step time0 && ...): the output is APPENDED to --out.  The tool stops, with a non-zero exit
status, at the first call that fails, the first differing byte and the first missed bar.

bits : the same seeded inputs through rwkv7_ce_fwd_bwd_ld_bf16 (in place), rwkv7_kl_acc_fwd_bwd_bf16 (in place, and out of place with
       dlogits one element off the logits' 16-byte phase: the kernel's all-singles route) and rwkv7_head_eval_bf16 (both kinds) of both
       libraries.  Byte equality of loss_rows, correct_rows, argmax_rows (67-row arrays, so rows the call must not write count too) and
       of the whole logits / d logits allocation, pad columns and the canary row on each side included.
       V in VS x ld in {V, V rounded up to 8, + 8} x base offset {0, 1} element x rows in ROWS x smoothing {0, 0.1} x three fills:
       N(0, 3); magnitude 80 (whole rows at -80 / +80, the label at -80 under a +80 maximum); maxima planted twice or three times across
       piece (8 elements), wave (512) and workgroup-round (2048) boundaries, and a whole row tied.  A third of the rows ignored, labels 0
       and V - 1 present.  One line per case.
time : the chunk shapes of tools/bench_eval_head.py (8192 x 8193, 8192 x 6562, 2048 x 66661; rows padded to 16 bytes, smoothing 0.1, a
       tenth of the rows ignored), one per step.  Three libraries: the parent's, this tree's and a second COPY of the parent's (loaded
       from a temporary file, so it is a code object of its own).  Per entry BLOCKS blocks of ROUNDS rounds; a round times one call of
       every library (device events around the call; the logits are restored before each call, outside the events), in an order that
       rotates with the round.  Per block the median of each library.
       Bar (stated before the first run): spread = the largest |parent copy - parent| among the blocks' medians -- what this run shows
       two identical kernels to differ by; excess = the median over the blocks of (new - parent).  excess <= spread, every entry."""
import argparse
import ctypes
import os
import shutil
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rwkvtts_amd import _lib  # noqa: E402

DEV = "cuda:0"
NAN_BITS = 0x7FC1   # a quiet NaN with a payload: pad columns and canary rows must keep it bit for bit
VS = [2, 9, 16, 1025, 6562, 8192, 8193, 66661]   # 9 at offset 1: head = 7, no piece, a two-element tail; 8193: the KL kernel without REG
ROWS = [1, 3, 4, 5, 67]
SHAPES = [(8192, 8193), (8192, 6562), (2048, 66661)]
ENTRIES = ("rwkv7_ce_fwd_bwd_ld_bf16", "rwkv7_kl_acc_fwd_bwd_bf16", "rwkv7_head_eval_bf16")
BLOCKS, ROUNDS = 5, 20
SCALE = 0.37   # d logits = (softmax - target) * SCALE: the multiply is part of what is compared


def load(path):
    so = ctypes.CDLL(os.path.abspath(path))
    for name in ENTRIES:
        fn = getattr(so, name)
        fn.restype, fn.argtypes = _lib.prototypes()[name]
    return so


class Fail(Exception):
    pass


def call(so, name, *args):
    rc = getattr(so, name)(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise Fail(f"{name} returned {rc}")


class Buf:
    """[rows, ld] bf16 logits inside a NaN-filled allocation: `offset` elements, a canary row, the rows, a canary row."""

    def __init__(self, rows, V, ld, offset, fill=None):
        self.flat = torch.full((offset + (rows + 2) * ld,), NAN_BITS, dtype=torch.int16, device=DEV).view(torch.bfloat16)
        self.x = self.flat[offset + ld:offset + ld + rows * ld].view(rows, ld)
        if fill is not None:
            self.x[:, :V] = fill
        assert self.x.data_ptr() % 16 == (2 * (offset + ld)) % 16

    def copy(self):
        c = Buf.__new__(Buf)
        c.flat = self.flat.clone()
        off = (self.x.data_ptr() - self.flat.data_ptr()) // 2
        c.x = c.flat[off:off + self.x.numel()].view(self.x.shape)
        assert c.x.data_ptr() % 16 == self.x.data_ptr() % 16
        return c


def fills(V, g):
    """{name: [67, V] bf16} and the labels [67] (ignored rows: -1)"""
    n = ROWS[-1]
    labels = torch.randint(0, V, (n,), generator=g)
    labels[0], labels[1] = 0, V - 1
    labels[2::3] = -1   # a third of the rows ignored
    normal = torch.randn(n, V, generator=g) * 3.0
    pm80 = (torch.randn(n, V, generator=g) * 30.0).clamp(-80, 80)
    pm80[0, V - 1], pm80[0, 0] = 80.0, -80.0   # label 0 at -80 under a maximum of +80
    pm80[1, V - 1] = 80.0                      # label V - 1 is the maximum
    pm80[3, :] = -80.0                         # a whole row at -80
    pm80[4, :] = 80.0                          # ... and one at +80
    ties = torch.randn(n, V, generator=g) * 3.0
    # element 8 i is piece i's first (aligned rows); pieces 63 | 64 meet at a wave boundary of the KL kernel, 255 | 256 at the end of
    # a round of its workgroup, 64 k at a round of the CE kernel's wave
    marks = [c for c in (0, 1, 7, 8, 15, 16, 511, 512, 519, 2047, 2048, 2055, V // 2, V - 9, V - 8, V - 2, V - 1) if 0 <= c < V]
    for r in range(n - 2):
        cols = [marks[(r + 5 * k) % len(marks)] for k in range(2 + r % 2)]   # two or three maxima
        ties[r, cols] = 40.0
        if r >= 2 and labels[r] != -1:
            labels[r] = min(cols) if r % 4 < 2 else max(cols)   # the label on the first maximum (correct) or on the last (not)
    ties[n - 2, :] = 1.0   # the whole row tied: index 0 wins
    ties[n - 1, :] = 1.0
    labels[n - 2], labels[n - 1] = 0, min(17, V - 1)
    return {"normal": normal.bfloat16().to(DEV), "pm80": pm80.bfloat16().to(DEV), "ties": ties.bfloat16().to(DEV)}, labels.to(DEV)


def outputs(n):
    return (torch.full((n,), -7.0, dtype=torch.float32, device=DEV), torch.full((n,), -7, dtype=torch.int32, device=DEV),
            torch.full((n,), -7, dtype=torch.int32, device=DEV))


def run_case(so, b, V, ld, rows, lab_ce, lab_kl, s):
    """every output of the five calls, as a list of (name, tensor)"""
    n, res = ROWS[-1], []
    ce, (loss, _, _) = b.copy(), outputs(n)
    call(so, ENTRIES[0], rows, V, ld, ce.x, lab_ce, -100, SCALE, loss, s)
    res += [("ce loss_rows", loss), ("ce logits allocation", ce.flat)]
    kl, (loss, corr, _) = b.copy(), outputs(n)
    call(so, ENTRIES[1], rows, V, ld, kl.x, kl.x, lab_kl, -1, s, SCALE, loss, corr)
    res += [("kl loss_rows", loss), ("kl correct_rows", corr), ("kl logits allocation", kl.flat)]
    # out of place, dlogits one element further into its allocation than the logits: x and dx differ modulo 16 bytes
    src, (loss, corr, _) = b.copy(), outputs(n)
    dst = Buf(n, V, ld, (b.x.data_ptr() - b.flat.data_ptr()) // 2 - ld + 1)
    assert (dst.x.data_ptr() - src.x.data_ptr()) % 16 != 0
    call(so, ENTRIES[1], rows, V, ld, src.x, dst.x, lab_kl, -1, s, SCALE, loss, corr)
    res += [("kl-oop loss_rows", loss), ("kl-oop correct_rows", corr), ("kl-oop logits allocation", src.flat),
            ("kl-oop dlogits allocation", dst.flat)]
    for kind, lab, ign in ((0, lab_ce, -100), (1, lab_kl, -1)):
        ev, (loss, corr, amax) = b.copy(), outputs(n)
        call(so, ENTRIES[2], rows, V, ld, ev.x, lab, ign, kind, s, loss, corr, amax)
        res += [(f"eval{kind} loss_rows", loss), (f"eval{kind} correct_rows", corr), (f"eval{kind} argmax_rows", amax),
                (f"eval{kind} logits allocation", ev.flat)]
    return res


def raw(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def step_bits(old, new, say):
    cases = 0
    for V in VS:
        sets, lab_kl = fills(V, torch.Generator().manual_seed(V))
        lab_ce = lab_kl.masked_fill(lab_kl == -1, -100)
        for name, fill in sets.items():
            for ld in (V, -(-V // 8) * 8 + 8):
                for offset in (0, 1):
                    b = Buf(ROWS[-1], V, ld, offset, fill)
                    for rows in ROWS:
                        for s in (0.0, 0.1):
                            a, c = run_case(old, b, V, ld, rows, lab_ce, lab_kl, s), run_case(new, b, V, ld, rows, lab_ce, lab_kl, s)
                            torch.cuda.synchronize()
                            tag = f"bits {name:6s} V={V:5d} ld={ld:5d} off={offset} rows={rows:2d} s={s}"
                            for (what, x), (_, y) in zip(a, c):
                                if not torch.equal(raw(x), raw(y)):
                                    n = (raw(x) != raw(y)).sum().item()
                                    raise Fail(f"{tag}: {what} DIFFERS in {n} of {x.numel()} elements")
                            say(f"{tag}: {len(a)} outputs of 5 calls byte-equal")
                            cases += 1
    say(f"# bits: {cases} cases, every output of every entry byte-equal between the two libraries")


def step_time(libs, shape, say):
    rows, V = SHAPES[shape]
    ld = -(-V // 8) * 8
    g = torch.Generator().manual_seed(V)
    labels = torch.randint(0, V, (rows,), generator=g)
    labels[::10] = -1
    labels = labels.to(DEV)
    x = torch.zeros(rows, ld, dtype=torch.bfloat16, device=DEV)
    x[:, :V] = (torch.randn(rows, V, generator=g) * 3).bfloat16().to(DEV)
    work = x.clone()
    loss, corr, _ = outputs(rows)
    entries = {
        "ce_fwd_bwd_ld": lambda so: call(so, ENTRIES[0], rows, V, ld, work, labels, -1, 1.0, loss, 0.1),
        "kl_acc_fwd_bwd": lambda so: call(so, ENTRIES[1], rows, V, ld, work, work, labels, -1, 0.1, 1.0, loss, corr),
        "head_eval kind 0": lambda so: call(so, ENTRIES[2], rows, V, ld, work, labels, -1, 0, 0.1, loss, corr, None),
        "head_eval kind 1": lambda so: call(so, ENTRIES[2], rows, V, ld, work, labels, -1, 1, 0.1, loss, corr, None),
    }
    names = list(libs)   # parent, new, parent-copy
    for ename, fn in entries.items():
        for so in libs.values():   # warm-up: code objects loaded, clocks up
            for _ in range(3):
                work.copy_(x)
                fn(so)
        torch.cuda.synchronize()
        med = {n: [] for n in names}
        for _ in range(BLOCKS):
            ev = {n: [] for n in names}
            for r in range(ROUNDS):
                for k in range(len(names)):
                    n = names[(k + r) % len(names)]
                    work.copy_(x)
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    fn(libs[n])
                    t1.record()
                    ev[n].append((t0, t1))
            torch.cuda.synchronize()
            for n in names:
                med[n].append(statistics.median(a.elapsed_time(b) * 1e3 for a, b in ev[n]))
        spread = max(abs(c - p) for p, c in zip(med["parent"], med["parent-copy"]))
        excess = statistics.median(n - p for p, n in zip(med["parent"], med["new"]))
        tag = f"time {rows:5d} x {V:5d} {ename:16s}"
        for n in names:
            say(f"{tag} | {n:11s} | median of block medians {statistics.median(med[n]):8.2f} us | blocks "
                + " ".join(f"{m:8.2f}" for m in med[n]))
        ok = excess <= spread
        say(f"{tag} | new - parent = {excess:+.2f} us, parent-copy spread {spread:.2f} us: {'meets' if ok else 'MISSES'} the bar")
        if not ok:
            raise Fail(f"{tag}: the new kernel exceeds the parent's median by more than the old-versus-old spread")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", required=True, help="the parent commit's librwkv7_hip.so, copied aside")
    ap.add_argument("--new", default=_lib.SO_PATH)
    ap.add_argument("--step", choices=["bits", "time0", "time1", "time2"], help="one step only (default: all four in turn)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_rows_ab.txt"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f, tempfile.TemporaryDirectory() as tmp:
        def say(line):
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        old, new = load(a.old), load(a.new)
        say(f"# tools/ab_head_rows.py --step {a.step or 'all'}: old {os.path.basename(a.old)}, new {os.path.relpath(a.new, ROOT)}; "
            f"{torch.cuda.get_device_name(0)}; torch {torch.__version__}")
        try:
            for step in [a.step] if a.step else ["bits", "time0", "time1", "time2"]:
                if step == "bits":
                    step_bits(old, new, say)
                else:
                    libs = {"parent": old, "new": new, "parent-copy": load(shutil.copy(a.old, os.path.join(tmp, "parent_copy.so")))}
                    if step in ("time0", a.step):
                        say(f"# time: {BLOCKS} blocks of {ROUNDS} rounds per entry, one call per library and round, device events, us")
                    step_time(libs, int(step[-1]), say)
        except Fail as e:
            say(f"FAILED: {e}")
            sys.exit(1)


if __name__ == "__main__":
    main()
