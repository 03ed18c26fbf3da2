"""Same-process timing of the dense projections' weight gradients (dy^T x over M = 32768 rows): rwkv7_wgrad_tn_bf16 + reduction against the
library slabs + reduction, interleaved round by round, operands rotating through several buffers so that no round starts on a warm
cache.  Run under rocprofv3 --kernel-trace --stats for the per-kernel split.

    python tools/wgrad_tn_ab.py            # the three 0.4B classes
    python tools/wgrad_tn_ab.py xy         # and the 1.5B XY classes
"""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rwkvtts_amd import fused
DEV = "cuda"
M = 32768
# (N, K, slab counts tried for the own kernel); the library side keeps wgrad_splitk's own choice (8 up to 1024 x 1024, else 4)
SHAPES = [(4096, 1024, (4, 8)), (1024, 4096, (4, 8)), (1024, 1024, (8, 16, 32))]
if "xy" in sys.argv[1:]:
    SHAPES += [(2048, 2048, (4, 8)), (8192, 2048, (1, 2)), (2048, 8192, (1, 2))]
ROUNDS, N_IT = int(os.environ.get("AB_ROUNDS", "5")), int(os.environ.get("AB_ITERS", "20"))


def timed(bufs, own, S):
    fused.TN_WGRAD = own
    for dy, x in bufs[:2]:
        fused.wgrad_splitk(dy, x, slabs=S)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(N_IT):
        dy, x = bufs[i % len(bufs)]
        fused.wgrad_splitk(dy, x, slabs=S)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / N_IT * 1e3


for N, K, slab_counts in SHAPES:
    nbuf = max(2, -(-(1 << 30) // (M * (N + K) * 2)))   # at least 1 GB of operands in rotation
    torch.manual_seed(N + K)
    bufs = [(torch.randn(M, N, device=DEV, dtype=torch.bfloat16), torch.randn(M, K, device=DEV, dtype=torch.bfloat16)) for _ in range(nbuf)]
    fused.TN_WGRAD_CLASSES = {**fused.TN_WGRAD_CLASSES, (N, K): slab_counts[0]}
    res = {"lib": []}
    for rnd in range(ROUNDS):
        res["lib"].append(timed(bufs, False, None))
        for S in slab_counts:
            res.setdefault(S, []).append(timed(bufs, True, S))
    flop = 2.0 * M * N * K
    print(f"dW [{N}][{K}], M = {M}, {nbuf} operand sets in rotation, {ROUNDS} rounds x {N_IT} calls (us per call, kernel(s) + reduction)")
    for key, ts in res.items():
        name = "library slabs" if key == "lib" else f"own kernel, S = {key:2d}"
        med = sorted(ts)[len(ts) // 2]
        print(f"  {name:22s} median {med:7.1f}   min {min(ts):7.1f}   max {max(ts):7.1f}   ({flop / med / 1e9:5.2f} PF/s incl. reduction)   rounds: "
              + " ".join(f"{t:.1f}" for t in ts), flush=True)
    del bufs
    torch.cuda.empty_cache()
