"""Records what the closed-batch token draws (RowSampler / SampleTail / ras_step) produce on the fixed inputs of tests/draw_cases.py:

    python tools/pin_draw_ids.py            # run on the GPU, compare with tests/golden/draw_ids.npz
    python tools/pin_draw_ids.py --write    # ... and write that file

The record is only meaningful from a library whose draw kernels are known good, i.e. one in which every draw kernel still has its
own body; once written it is not to be regenerated after a change under csrc/.  RWKV7_HIP_SO selects the library.  Only ids and
small state arrays are stored, no logits."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np

import draw_cases

PATH = os.path.join(ROOT, "tests", "golden", "draw_ids.npz")

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    res = draw_cases.run_groups("cuda:0")
    if a.write:
        np.savez_compressed(PATH, **res)
        print(f"wrote {PATH}: {len(res)} arrays, {os.path.getsize(PATH)} bytes")
    elif not os.path.exists(PATH):
        sys.exit(f"{PATH} is missing: nothing to compare with (see --write)")
    else:
        old = np.load(PATH)
        bad = [k for k in res if k not in old.files or not np.array_equal(old[k], res[k])] + [k for k in old.files if k not in res]
        print(f"{len(res)} arrays, {len(bad)} differ from {PATH}", *bad[:20], sep="\n")
        sys.exit(1 if bad else 0)
