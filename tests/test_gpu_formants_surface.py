"""The formant analysis at the Python surface (GPU): megatts2.extract_formants puts the candidates on the mel's frames and is the
handle call on the resampled audio, bit for bit; Megatts.output_formants analyses a synthesis call's own audio and leaves `aux` alone;
and what existed before - synthesize, forward (on a 22.05 kHz prompt, so through from_audio and the resampler), output_prosody, the
resampler - gives the same bits with the new calls made in between, and the resampler's new sr_out at its default is the call without it."""
import numpy as np
import pytest

import formant_ref as F
from conftest import synth_models
from test_gpu_prosody import synth_inputs, tiny_tts

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def tone_rows(lens, seed=0):
    """voiced audio at 16 kHz, one row per length, NaN behind each row"""
    w = np.full((len(lens), max(lens) + 3), np.nan, np.float32)
    for b, n in enumerate(lens):
        w[b, :n] = F.voiced_signal(max(n, 200), period=145 + 10 * b, sr=16000)[:n]
    return dev(w), np.asarray(lens, np.int32)


@pytest.mark.parametrize("lens", [(256 * 20 - 1,), (256 * 20,), (256 * 20 + 1,), (256 * 31 - 1, 5000, 256 * 9 - 1, 700)])
def test_extract_formants_lies_on_the_mel_frames(lens):
    from megatts2_amd import megatts2 as M
    from megatts2_amd import runtime as rt
    fe = M._frontend()
    w, ln = tone_rows(lens)
    out = M.extract_formants(w, None, ln)
    T = 1 + max(lens) // 256
    assert out["rate"] == 11000 and out["hop"] == 176 and out["frame_lens"].tolist() == [1 + n // 256 for n in lens]
    assert out["freq"].shape == (len(lens), T, 5) and out["bw"].shape == (len(lens), T, 5) and out["count"].shape == (len(lens), T)
    assert fe(w.nan_to_num(), ln).shape[1] == T                 # the mel's own width
    # the handle call on the resampled audio, bit for bit
    x, xl = fe.resample(w, 16000, ln, sr_out=11000)
    assert xl.tolist() == [-(-11 * n // 16) for n in lens]
    ref = fe.formants(x, xl, rt.Formants(), hop=176, sample_rate=11000)
    Tr = ref["count"].shape[1]
    assert Tr in (T, T + 1) and (Tr == T + 1) == (max(lens) % 256 == 255)
    for k in ("freq", "bw", "count"):
        assert torch.equal(out[k], ref[k][:, :T]), k
    assert int(out["count"].max()) >= 4
    # one row alone is the row of the batch, and a 1-D input drops the batch axis
    one = M.extract_formants(w[0, :lens[0]])
    assert one["freq"].shape == (1 + lens[0] // 256, 5) and torch.equal(one["freq"], out["freq"][0, :1 + lens[0] // 256])
    st = M.formant_stats(out["freq"], out["count"], None, out["frame_lens"])
    assert sorted(st) == sorted(M.FORMANT_STAT_NAMES) and st["frames"].shape == (len(lens),)


def test_extract_formants_rates():
    from megatts2_amd import megatts2 as M
    from megatts2_amd import runtime as rt
    fe = M._frontend()
    x = dev(F.voiced_signal(6000, sr=16000)[None])
    # max_formant_hz = sample_rate / 2 skips the resampler: the handle call on the audio as it is
    out = M.extract_formants(x, None, None, rt.Formants(max_formant_hz=8000.0))
    ref = fe.formants(x, None, rt.Formants(max_formant_hz=8000.0), hop=256, sample_rate=16000)
    assert out["rate"] == 16000 and out["hop"] == 256 and all(torch.equal(out[k], ref[k]) for k in ("freq", "bw", "count"))
    # a rate at which the mel's hop is no whole number of samples is refused, not rounded
    with pytest.raises(ValueError, match="whole number"):
        M.extract_formants(x, None, None, rt.Formants(max_formant_hz=5512.5))
    # audio at another rate: the frame count is the mel's of the same audio at 16 kHz
    y = dev(F.voiced_signal(9000, period=200, sr=22050)[None])
    out = M.extract_formants(y, 22050)
    assert out["frame_lens"].tolist() == [1 + rt.resample_query(22050, 16000, 9000)[0] // 256] and out["count"].shape[1] == out["frame_lens"][0]


def test_both_handles_give_the_same_bits():
    from megatts2_amd import megatts2 as M
    from megatts2_amd import runtime as rt
    fe, nat = M._frontend(), tiny_tts(None).native
    w, ln = tone_rows((3000, 1200))
    kw = dict(hop=176, sample_rate=11000, return_lpc=True, return_err=True, return_autocorr=True, return_roots=True, return_iters=True)
    a, b = nat.formants(w, ln, rt.Formants(order=12), **kw), fe.formants(w, ln, rt.Formants(order=12), **kw)
    assert sorted(a) == sorted(b) == sorted(("freq", "bw", "count", "lpc", "err", "autocorr", "roots", "iters"))
    assert all(torch.equal(torch.view_as_real(a[k]) if a[k].is_complex() else a[k], torch.view_as_real(b[k]) if b[k].is_complex() else b[k])
               for k in a)
    assert a["roots"].shape == (2, 18, 12) and a["roots"].dtype == torch.complex128 and a["lpc"].shape == (2, 18, 13)
    fl = 1 + ln // 176
    assert torch.equal(nat.formant_stats(a["freq"], a["count"], None, fl), fe.formant_stats(b["freq"], b["count"], None, fl))
    # the defaults of the model's handle are the mel's: 16 kHz, hop 256
    assert torch.equal(nat.formants(w, ln)["freq"], fe.formants(w, ln)["freq"]) and nat.formants(w, ln)["count"].shape == (2, 1 + 3000 // 256)


def snapshot(tts, inputs):
    phone, prompt, pl, ml = inputs
    mel, mel_lens, aux = tts.synthesize(phone, prompt, pl, ml, griffin_lim={"n_iter": 2}, return_aux=True)
    pros = tts.output_prosody(mel_lens, aux, phone_lens=pl)
    return mel, mel_lens, aux, pros


def forward_snapshot(tts, prompts):
    """Megatts.forward with none of the new arguments on a prompt directory that holds a 22.05 kHz file - so the call goes through
    MelFrontEnd.from_audio and the resampler, whose rate now passes through `sr_out` - -> (mel, lens, the tensors of aux)"""
    phone = np.random.default_rng(6).integers(1, synth_models("tiny")[0][0].mrte.phone_vocab_size, 6)
    mel, lens, aux = tts.forward(prompts, phone_tokens=phone, out_path=None)
    return mel, np.asarray(lens), {k: v for k, v in aux.items() if hasattr(v, "is_cuda")}


def test_output_formants_and_the_calls_that_were_there(tmp_path):
    from megatts2_amd import audio_io
    from megatts2_amd import megatts2 as M
    tts = tiny_tts(None)
    inputs = synth_inputs()
    fe = M._frontend()
    w, ln = tone_rows((4000, 2500))
    audio_io.write_wav(str(tmp_path / "prompt.wav"), F.voiced_signal(int(0.6 * 22050), period=200, sr=22050), 22050)
    fwd0 = forward_snapshot(tts, str(tmp_path))
    assert {"dur", "codes"} <= set(fwd0[2])
    mel0, lens0, aux0, pros0 = snapshot(tts, inputs)
    rs0 = fe.resample(w, 22050, ln)
    keys, before = sorted(aux0), {k: v.clone() for k, v in aux0.items() if hasattr(v, "clone")}
    out = tts.output_formants(lens0, aux0)
    assert set(M.FORMANT_STAT_NAMES) <= set(out) and all(out[k].shape == (2,) and out[k].dtype == np.float64 for k in M.FORMANT_STAT_NAMES)
    assert sorted(aux0) == keys and all(torch.equal(aux0[k], v) for k, v in before.items())      # aux is not altered
    ml = np.asarray(lens0, np.int32)
    assert out["f0"].shape[1] == out["count"].shape[1] == int(ml.max()) and (out["frame_lens"] <= ml).all()
    # its figures are formant_stats of its own tracks over the voiced frames
    again = M.formant_stats(out["freq"], out["count"], out["f0"], out["frame_lens"])
    assert all(np.array_equal(again[k], out[k]) for k in M.FORMANT_STAT_NAMES)
    assert torch.equal(out["f0"], pros0["f0"])
    with pytest.raises(ValueError):
        tts.output_formants(lens0, {"dur": aux0["dur"]})
    # ... and with the new calls made, what was there gives the bits it gave
    mel1, lens1, aux1, pros1 = snapshot(tts, inputs)
    assert torch.equal(mel0, mel1) and np.array_equal(lens0, lens1)
    assert all(torch.equal(aux0[k], aux1[k]) for k in before)
    assert torch.equal(pros0["f0"], pros1["f0"]) and torch.equal(pros0["energy"], pros1["energy"])
    assert all(np.array_equal(pros0["phones"][k], pros1["phones"][k], equal_nan=True) for k in pros0["phones"])
    fwd1 = forward_snapshot(tts, str(tmp_path))
    assert torch.equal(fwd0[0], fwd1[0]) and np.array_equal(fwd0[1], fwd1[1]) and sorted(fwd0[2]) == sorted(fwd1[2])
    assert all(torch.equal(fwd0[2][k], fwd1[2][k]) for k in fwd0[2])
    rs1, rs2 = fe.resample(w, 22050, ln), fe.resample(w, 22050, ln, sr_out=16000)
    assert torch.equal(rs0[0], rs1[0]) and torch.equal(rs0[0], rs2[0]) and np.array_equal(rs0[1], rs1[1]) and np.array_equal(rs0[1], rs2[1])
