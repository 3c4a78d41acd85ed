"""The return codes of the Whisper decoder and encoder entry points for one bad call per shared argument check
(include/cbw.h: -1 CBW_ERR_INVALID, -3 CBW_ERR_OOM, -4 CBW_ERR_STATE): a `micro` decoder and encoder with max_len 8;
where a buffer is only checked, never touched, it is 1 MB of device memory."""
import numpy as np
import pytest
import torch

from cbw import _lib, synth

pytestmark = pytest.mark.gpu

MAX_LEN, B, BENC = 8, 4, 2
INVALID, OOM, STATE = -1, -3, -4


@pytest.fixture(scope="module")
def dec():
    from cbw.decoder import DecoderEngine
    eng = DecoderEngine(synth.WHISPER_DECODERS["micro"], synth.synth_whisper_decoder_state_dict("micro", seed=0),
                        max_len=MAX_LEN)
    d = eng.device
    eng.nb = eng.lib.cbw_decoder_state_bytes(eng.h, B, BENC)
    assert 0 < eng.nb
    eng.buf = torch.zeros(max(eng.nb, 1 << 20), dtype=torch.uint8, device=d)      # the state
    eng.out = torch.zeros(max(17 * eng.vpad * 4, 1 << 20), dtype=torch.uint8, device=d)   # logits / probs
    eng.i32 = torch.zeros(1 << 18, dtype=torch.int32, device=d)                  # tokens / positions / rows: zeros
    eng.enc = torch.zeros((1500, eng.d_model), device=d)
    return eng


def state_tail(eng, rows=B, benc=BENC, nb=None):
    return rows, benc, eng.buf.data_ptr(), eng.nb if nb is None else nb


def test_decoder_step(dec):
    lib, h, st = dec.lib, dec.h, _lib.stream_handle()
    tok, out = dec.i32.data_ptr(), dec.out.data_ptr()
    assert lib.cbw_decoder_step(h, tok, 0, *state_tail(dec), out, st) == 0
    assert lib.cbw_decoder_step(h, None, 0, *state_tail(dec), out, st) == INVALID
    assert lib.cbw_decoder_step(h, tok, MAX_LEN, *state_tail(dec), out, st) == INVALID
    assert lib.cbw_decoder_step(h, tok, 0, *state_tail(dec, rows=B + 1), out, st) == INVALID
    assert lib.cbw_decoder_step(h, tok, 0, *state_tail(dec, nb=dec.nb - 1), out, st) == OOM


def test_decoder_step_after_set_param():
    """a parameter set after finalize un-finalizes the handle"""
    from cbw.decoder import DecoderEngine
    sd = synth.synth_whisper_decoder_state_dict("micro", seed=0)
    eng = DecoderEngine(synth.WHISPER_DECODERS["micro"], sd, max_len=MAX_LEN)
    nb = eng.lib.cbw_decoder_state_bytes(eng.h, 1, 1)
    state = torch.zeros(nb, dtype=torch.uint8, device=eng.device)
    tok = torch.zeros(1, dtype=torch.int32, device=eng.device)
    out = torch.zeros(eng.vpad, device=eng.device)
    w = np.ascontiguousarray(sd["layer_norm.bias"], dtype=np.float32)
    assert eng.lib.cbw_decoder_set_param(eng.h, b"layer_norm.bias", w.ctypes.data, w.size) == 0
    assert eng.lib.cbw_decoder_step(eng.h, tok.data_ptr(), 0, 1, 1, state.data_ptr(), nb, out.data_ptr(),
                                    _lib.stream_handle()) == STATE


def test_decoder_step_dev(dec):
    lib, h, st = dec.lib, dec.h, _lib.stream_handle()
    tok, out = dec.i32.data_ptr(), dec.out.data_ptr()
    assert lib.cbw_decoder_step_dev(h, tok, None, *state_tail(dec), out, st) == INVALID
    nb17 = lib.cbw_decoder_state_bytes(h, 17, 1)
    assert 0 < nb17 <= dec.buf.numel()
    assert lib.cbw_decoder_step_dev(h, tok, tok, 17, 1, dec.buf.data_ptr(), nb17, out, st) == INVALID


def test_decoder_prefill(dec):
    lib, h, st = dec.lib, dec.h, _lib.stream_handle()
    tok, out = dec.i32.data_ptr(), dec.out.data_ptr()
    assert lib.cbw_decoder_prefill(h, tok, 2, *state_tail(dec), out, st) == INVALID   # Benc = 2
    rows = lambda T, slot, r0, nb: lib.cbw_decoder_prefill_rows(h, tok, T, slot, r0, nb, *state_tail(dec), out, st)  # noqa: E731
    assert rows(2, 1, 2, 2) == 0
    assert rows(MAX_LEN + 1, 1, 2, 2) == INVALID
    assert rows(2, BENC, 2, 2) == INVALID
    assert rows(2, 1, 3, 2) == INVALID   # r0 + nb > B


def test_decoder_cross_attn_probs(dec):
    lib, h, st = dec.lib, dec.h, _lib.stream_handle()
    tok, out = dec.i32.data_ptr(), dec.out.data_ptr()

    def probs(heads, n):
        heads = np.array(heads, dtype=np.int32)
        return lib.cbw_decoder_cross_attn_probs(h, tok, 2, heads.ctypes.data, n, *state_tail(dec), out, st)
    assert probs([0, 0], 1) == 0
    assert probs([dec.n_layers, 0], 1) == INVALID
    assert probs([0, 0], 0) == INVALID


def test_decoder_reorder(dec):
    lib, h, st = dec.lib, dec.h, _lib.stream_handle()
    rows = dec.i32.data_ptr()
    assert lib.cbw_decoder_reorder(h, rows, B, BENC, MAX_LEN + 1, dec.buf.data_ptr(), dec.nb, st) == INVALID
    assert lib.cbw_decoder_reorder(h, rows, B, BENC, 0, dec.buf.data_ptr(), dec.nb, st) == 0


def test_decoder_cross_kv_slot(dec):
    lib, h, st = dec.lib, dec.h, _lib.stream_handle()
    slot = lambda s: lib.cbw_decoder_cross_kv_slot(h, dec.enc.data_ptr(), s, BENC, dec.buf.data_ptr(), dec.nb, B, st)  # noqa: E731
    assert slot(1) == 0
    assert slot(BENC) == INVALID
    torch.cuda.synchronize()


def test_encoder_hs():
    from cbw.whisper import EncoderEngine
    eng = EncoderEngine(synth.WHISPER_CONFIGS["micro"], synth.synth_whisper_encoder_state_dict("micro", seed=0))
    d, lib = eng.device, eng.lib
    nb = lib.cbw_encoder_workspace_bytes(eng.h, 1)
    mel = torch.zeros((3000, eng.cpad), dtype=torch.bfloat16, device=d)
    hs = torch.zeros((1, 1, 1500, eng.d_model), device=d)
    ws = torch.zeros(nb, dtype=torch.uint8, device=d)

    def call(layer, nbytes):
        ids = np.array([layer], dtype=np.int32)
        return lib.cbw_encoder_hs(eng.h, mel.data_ptr(), 1, ids.ctypes.data, 1, 0, hs.data_ptr(), ws.data_ptr(), nbytes,
                                  _lib.stream_handle())
    assert call(eng.n_layers + 1, nb) == INVALID
    assert call(0, nb - 1) == OOM
    assert call(0, nb) == 0
    torch.cuda.synchronize()
