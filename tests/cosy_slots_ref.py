"""Pure-Python restatement of what rwkv7_ras_slots_f32 does with a live slot's drawn id (include/rwkv7_hip.h): the streaming loop of
RWKV7CosyLM.inference for one slot.  Shared by tests/test_continuous_cosy.py and tests/test_continuous_cosy_gpu.py."""


def new_slot(limit, win_size, step=0, live=1):
    return dict(step=step, limit=limit, ptr=0, n_out=0, live=live, ids=None, recent=[-1] * win_size, seq=[])


def slot_bookkeeping(s, drawn, eos, win_size):
    """Updates the slot dict `s` (keys of new_slot) in place for the id `drawn` and returns it.  A slot that is not live is untouched."""
    if not s["live"]:
        return s
    s["ids"] = drawn
    if drawn != eos:   # the reference appends emitted ids only
        s["seq"].append(drawn)
        s["recent"][s["ptr"]] = drawn
        s["ptr"] = (s["ptr"] + 1) % win_size
        s["n_out"] += 1
    s["step"] += 1
    s["live"] = int(drawn != eos and s["step"] < s["limit"])
    return s
