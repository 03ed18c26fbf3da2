"""CPU: the device-free parts of continuous batching for the Cosy model -- cosy_request against the pieces RWKV7CosyLM.inference
builds, the pure-Python restatement of the slot bookkeeping (tests/cosy_slots_ref.py, reused by the GPU tests), the slicing of
ContinuousCosyDecoder.stream on fake read-backs, and the ValueError paths that need no device."""
import pytest
import torch

from cosy_slots_ref import new_slot, slot_bookkeeping
from rwkvtts_amd import _lib
from rwkvtts_amd.continuous_cosy import ContinuousCosyDecoder, CosyRequest, RasSlotState, StreamCursor, cosy_request
from rwkvtts_amd.cosy_llm import RWKV7CosyConfig, RWKV7CosyLM


@pytest.fixture(scope="module")
def model():
    cfg = RWKV7CosyConfig(vocab_size=65536, speech_token_size=96, hidden_size=64, num_hidden_layers=1, decay_low_rank_dim=32,
                          a_low_rank_dim=32, v_low_rank_dim=32, gate_low_rank_dim=32)
    m = RWKV7CosyLM(cfg)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():   # only the embeddings are touched
        for e in (m.llm_embedding, m.text_embedding, m.speech_embedding):
            e.weight.copy_(torch.randn(e.weight.shape, generator=g))
    return m.eval()


def _inference_pieces(m, text, prompt_text, prompt_speech, max_ratio=20, min_ratio=0.5):
    """RWKV7CosyLM.inference up to its loop, on [1, T] tensors as it receives them."""
    text_len, prompt_text_len = torch.tensor([text.shape[1]]), torch.tensor([prompt_text.shape[1]])
    text = torch.cat([prompt_text, text], dim=1)
    n_text = int((text_len + prompt_text_len).item())
    hits = (text[0] == 65531).nonzero()
    n_instr = int(hits[0, 0].item()) + 1 if hits.numel() else 0
    content_length = original_text_len = n_text - n_instr
    emb_w = m.llm_embedding.weight
    pieces = [emb_w[m.sos_eos].view(1, 1, -1), m.text_embedding(text), emb_w[m.task_id].view(1, 1, -1)]
    if prompt_speech.shape[1] != 0:
        pieces.append(m.speech_embedding(prompt_speech))
    return torch.cat(pieces, dim=1)[0], int(content_length * min_ratio), int(content_length * max_ratio), original_text_len


@pytest.mark.parametrize("prefix", [False, True])
@pytest.mark.parametrize("speech", [False, True])
def test_cosy_request_equals_what_inference_builds(model, prefix, speech):
    g = torch.Generator().manual_seed(3)
    text = torch.randint(0, 65000, (1, 13), generator=g)
    prompt_text = torch.randint(0, 65000, (1, 7), generator=g)
    if prefix:
        prompt_text[0, 4] = 65531   # five ids of instruction, the separator included
    prompt_speech = torch.randint(0, 96, (1, 11 if speech else 0), generator=g)
    want, min_len, max_len, otl = _inference_pieces(model, text, prompt_text, prompt_speech)
    req = cosy_request(model, text, prompt_text, prompt_speech if speech else None)
    assert req.embeds.shape == (1 + 20 + 1 + (11 if speech else 0), 64)
    assert torch.equal(req.embeds, want)                                   # row for row
    assert torch.equal(req.embeds[0], model.llm_embedding.weight[0]) and torch.equal(req.embeds[21], model.llm_embedding.weight[1])
    assert torch.equal(req.embeds[1:8], model.text_embedding.weight[prompt_text[0]])
    assert torch.equal(req.embeds[8:21], model.text_embedding.weight[text[0]])
    if speech:
        assert torch.equal(req.embeds[22:], model.speech_embedding.weight[prompt_speech[0]])
    content = 15 if prefix else 20
    assert (req.min_len, req.max_len, req.original_text_len) == (min_len, max_len, otl) == (content // 2, content * 20, content)
    assert req.n_ignore == content // 2 - content and req.limit == content * 20
    # flat ids and the [1, T] form are the same request; other ratios
    flat = cosy_request(model, text[0].tolist(), prompt_text[0], prompt_speech[0] if speech else None, max_token_text_ratio=3.3,
                        min_token_text_ratio=1.5)
    assert torch.equal(flat.embeds, want)
    assert (flat.min_len, flat.max_len) == (int(content * 1.5), int(content * 3.3)) and flat.n_ignore == int(content * 1.5) - content


def test_cosy_request_without_a_prompt_and_bad_sampling(model):
    text = torch.tensor([5, 65531, 9, 10, 11])
    req = cosy_request(model, text)
    assert req.embeds.shape == (7, 64) and (req.min_len, req.max_len, req.original_text_len) == (1, 60, 3)
    for k in (0, 129):
        with pytest.raises(ValueError):
            cosy_request(model, text, sampling=k)


def test_slot_bookkeeping_ring_pointer_eos_and_limit():
    EOS, W = 96, 4
    s = new_slot(limit=7, win_size=W)
    for i, d in enumerate([5, 6, 7, 8, 9]):                               # the ring of four wraps on the fifth id
        slot_bookkeeping(s, d, EOS, W)
        assert s["step"] == s["n_out"] == i + 1 and s["ptr"] == (i + 1) % W and s["live"] == 1 and s["ids"] == d
    assert s["recent"] == [9, 6, 7, 8] and s["seq"] == [5, 6, 7, 8, 9]
    before = dict(s, recent=list(s["recent"]), seq=list(s["seq"]))
    slot_bookkeeping(s, EOS, EOS, W)                                       # EOS: nothing is appended, the slot ends
    assert s["ids"] == EOS and s["step"] == 6 and s["live"] == 0
    assert (s["recent"], s["seq"], s["ptr"], s["n_out"]) == (before["recent"], before["seq"], before["ptr"], before["n_out"])
    dead = dict(s, recent=list(s["recent"]), seq=list(s["seq"]))
    slot_bookkeeping(s, 3, EOS, W)                                         # a slot that is not live is untouched
    assert s == dead
    t = new_slot(limit=3, win_size=W)
    for d in (1, 1, 1):
        slot_bookkeeping(t, d, EOS, W)
    assert t["live"] == 0 and t["step"] == 3 and t["seq"] == [1, 1, 1]     # the limit ends it on the exact step
    u = new_slot(limit=1, win_size=W)
    slot_bookkeeping(u, 2, EOS, W)
    assert u["live"] == 0 and u["n_out"] == 1                               # limit 1: finished with its first id


def test_stream_cursor_slices_on_fake_read_backs():
    LD = 100
    cur = StreamCursor(LD)
    seq = torch.arange(4 * LD).view(4, LD)                                 # seq[s, c] = s * LD + c
    got = {7: [], 8: [], 9: []}

    def read_back(running):
        flat, counts = cur.take(running)
        assert [h for h, _ in counts] == [h for _, h, _ in running]
        pieces = seq.view(-1)[torch.tensor(flat, dtype=torch.int64)].split([n for _, n in counts])
        for (h, n), p in zip(counts, pieces):
            assert p.numel() == n
            got[h] += p.tolist()
        return [n for _, n in counts]

    assert read_back([(0, 7, 3), (2, 8, 0)]) == [3, 0]                     # nothing emitted yet: an empty piece
    assert read_back([(0, 7, 3), (2, 8, 5)]) == [0, 5]                     # no progress (the slot drew EOS): empty again
    assert read_back([(2, 8, 9)]) == [4] and 7 not in cur.seen             # handle 7 retired: forgotten
    assert read_back([(0, 9, 2), (2, 8, 9)]) == [2, 0]                     # slot 0 reused by handle 9: starts at column 0
    cur.finish(8)
    assert read_back([(0, 9, LD + 5)]) == [LD - 2] and cur.seen == {9: LD}  # never past the row
    assert got[7] == [0, 1, 2] and got[8] == list(range(2 * LD, 2 * LD + 9)) and got[9] == list(range(LD))


def test_request_dataclass_and_struct_layout():
    r = CosyRequest(torch.zeros(3, 8), min_len=12, max_len=40, original_text_len=5)
    assert r.n_ignore == 7 and r.limit == 40
    names = [f[0] for f in RasSlotState._fields_]
    assert names == ["step", "limit", "n_ignore", "seed", "top_k", "top_p", "tau_r", "live", "recent", "win_ld", "ptr", "ids", "n_out",
                     "seq", "seq_ld", "emb", "x", "D", "slots", "win_size", "top_k_max", "eos"]
    # the struct as include/rwkv7_hip.h declares it: same members in the same order
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "rwkv7_hip.h")).read()
    body = re.search(r"typedef struct rwkv7_ras_slot_state \{(.*?)\} rwkv7_ras_slot_state;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [re.search(r"(\w+);", d + ";").group(1) for d in body.split(";") if d.strip()] == names


def test_new_entry_is_exported(hip_lib):
    assert "rwkv7_ras_slots_f32" in _lib.exported_symbols() and hasattr(hip_lib, "rwkv7_ras_slots_f32")


@pytest.mark.parametrize("kw", [dict(slots=0), dict(slots=33), dict(admission="lazy"), dict(max_len_cap=0), dict(check_every=0),
                                dict(win_size=0), dict(win_size=129), dict()])
def test_decoder_value_errors_without_a_device(model, kw):
    # the last case: an fp32 model ("needs a bf16 model")
    with pytest.raises(ValueError):
        ContinuousCosyDecoder(model, **kw)


def test_decoder_refuses_a_head_that_is_not_speech_token_size_plus_one(model):
    import copy
    m = copy.copy(model)
    m.__dict__ = dict(model.__dict__)
    m.speech_token_size = 90
    with pytest.raises(ValueError, match="speech_token_size"):
        ContinuousCosyDecoder(m)
