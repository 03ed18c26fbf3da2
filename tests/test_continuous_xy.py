"""CPU: the device-free parts of continuous batching for the XY model -- the column map of the concatenated head, the ValueError
paths of ContinuousXYDecoder that need no device, and the new entries' argument checks (nothing is launched)."""
import ctypes

import pytest
import torch

from rwkvtts_amd import _lib
from rwkvtts_amd.continuous_xy import ContinuousXYDecoder, XYSlotState, head_column_map
from rwkvtts_amd.sampling import RowSampler
from rwkvtts_amd.xy_llm import RWKV7XYConfig, RWKV7XYLM


def test_head_column_map_real_xy_config():
    cm = head_column_map(66661, 1025, 8, 65536)
    assert cm.sizes == (66661,) + (1025,) * 7
    assert cm.allow == ((65536, 66561),) + ((0, 1025),) * 7
    assert cm.head0_rows == (65536, 66561)
    assert cm.col0 == tuple(1025 * c for c in range(8))
    assert cm.seg_off == (-65536,) + tuple(1025 * c for c in range(1, 8))
    assert cm.width == 8200 and cm.max_domain == 1025
    # every channel's allowed ids land on its own columns, back to back, and nowhere else
    cols = [range(o + lo, o + hi) for o, (lo, hi) in zip(cm.seg_off, cm.allow)]
    assert [c.start for c in cols] == list(cm.col0) and cols[-1].stop == cm.width
    assert all(a.stop == b.start for a, b in zip(cols, cols[1:]))


def test_head_column_map_toy_config_matches_row_sampler_layout():
    cm = head_column_map(120, 16, 4, 100)
    assert cm.sizes == (120, 16, 16, 16) and cm.allow == ((100, 116), (0, 16), (0, 16), (0, 16))
    assert cm.col0 == (0, 16, 32, 48) and cm.seg_off == (-100, 16, 32, 48) and cm.width == 64 and cm.max_domain == 16
    # what RWKV7XYLM.generate hands to RowSampler for the same layout (xy_llm.make_sampler: seg_off = col0 - allow_lo)
    assert list(cm.seg_off) == [c - a[0] for c, a in zip([0] + [16 + 16 * (i - 1) for i in range(1, 4)], cm.allow)]
    assert RowSampler.supported(torch.device("cuda"), list(cm.sizes), list(cm.allow), None) is None


@pytest.mark.parametrize("args", [(120, 16, 0, 100), (120, 16, 17, 100), (110, 16, 4, 100), (120, 0, 4, 100), (40000, 15361, 2, 0)])
def test_head_column_map_rejects(args):
    with pytest.raises(ValueError):
        head_column_map(*args)


def _cpu_model():
    cfg = RWKV7XYConfig(vocab_size=120, speech_vocab_size=16, num_channels=4, text_shift_size=100, hidden_size=128,
                        num_hidden_layers=1, decay_low_rank_dim=32, a_low_rank_dim=32, v_low_rank_dim=32, gate_low_rank_dim=32)
    return RWKV7XYLM(cfg)


@pytest.mark.parametrize("kw", [dict(slots=0), dict(slots=33), dict(admission="lazy"), dict(max_new_frames_cap=0), dict(check_every=0),
                                dict(eos_token_id=120), dict(eos_token_id=-2), dict()])
def test_decoder_value_errors_without_a_device(kw):
    # the last case: a model that is not on the HIP device
    with pytest.raises(ValueError):
        ContinuousXYDecoder(_cpu_model(), **kw)


def test_new_entries_are_exported(hip_lib):
    names = _lib.exported_symbols()
    for n in ("rwkv7_xy_slots_draw_f32", "rwkv7_xy_slots_frame_bf16"):
        assert n in names and hasattr(hip_lib, n)


def test_new_entries_argument_errors_do_not_launch(hip_lib):
    one = 16   # never dereferenced: the checks fire first
    p = ctypes.c_void_p

    def state(**kw):
        st = XYSlotState()
        for f in ("step", "limit", "seed", "inv_temp", "top_k", "top_p", "do_sample", "live", "needs", "nt", "row", "seq", "x"):
            setattr(st, f, one)
        st.seq_ld, st.D, st.C, st.slots, st.top_k_max = 8, 128, 4, 32, 64
        for c in range(16):
            st.tables[c] = one
        st.text_shift, st.speech_vocab, st.pad, st.eos0, st.eos_list, st.n_eos = 100, 16, 15, -1, None, 0
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    draw = lambda st, rows=1, logits=one, seg=one, lo=one, hi=one, dom=16: hip_lib.rwkv7_xy_slots_draw_f32(
        rows, p(logits), ctypes.c_long(64), None, p(seg), p(seg), p(lo), p(hi), dom, ctypes.byref(st) if st is not None else None, None)
    frame = lambda st, rows=1: hip_lib.rwkv7_xy_slots_frame_bf16(rows, None, ctypes.byref(st) if st is not None else None, None)
    EINVAL, ESHAPE = -1, -4
    assert draw(None) == EINVAL and frame(None) == EINVAL
    assert draw(state(), rows=0) == EINVAL and frame(state(), rows=0) == EINVAL
    assert draw(state(), logits=None) == EINVAL and draw(state(), seg=None) == EINVAL and draw(state(), dom=0) == EINVAL
    assert draw(state(), lo=None) == EINVAL                      # allow_lo without allow_hi
    for bad in (dict(live=None), dict(needs=None), dict(nt=None), dict(seq_ld=0), dict(slots=0), dict(C=0), dict(D=0), dict(n_eos=1)):
        assert draw(state(**bad)) == EINVAL and frame(state(**bad)) == EINVAL, bad
    st = state()
    st.tables[3] = None
    assert draw(st) == EINVAL and frame(st) == EINVAL
    assert draw(state(), dom=15361) == ESHAPE
    assert draw(state(top_k_max=65)) == ESHAPE and draw(state(top_k_max=-1)) == ESHAPE
    assert draw(state(C=17)) == ESHAPE and frame(state(C=17)) == ESHAPE
    assert draw(state(D=100)) == ESHAPE and frame(state(D=100)) == ESHAPE
