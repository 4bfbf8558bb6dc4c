"""The prompt-audio resampler on the GPU (csrc/resample.hip, mt2_resample) against the float64 restatement of its rule
(tests/resample_ref.py) applied with the LIBRARY's f32 filter table to the same f32 input.

Bars: per sample |y_gpu - y_ref| <= (K + 2) * 2^-24 * sum_k |h_k| |x_k| - the forward error bound of an f32 dot product of depth K
in any order, with or without fma, plus the final rounding; per utterance relative L2 <= 2e-6 (the bar of the other kernel tests).
Input padding beyond lens[b] is NaN (a read of it poisons the output), the output buffer is pre-filled with a sentinel and is wider
than needed."""
import functools
import math

import numpy as np
import pytest

import resample_ref as R
from conftest import synth_models

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SR_OUT = 16000
SENT = np.float32(-77.25)
GPU_RATES = (48000, 44100, 22050, 24000, 8000, 11025)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def frontend():
    from megatts2_amd.runtime import MelFrontEnd
    return MelFrontEnd()


@functools.lru_cache(maxsize=None)
def lib_table(sr_in):
    from megatts2_amd import runtime
    return runtime.resample_table(sr_in, SR_OUT)


@functools.lru_cache(maxsize=None)
def signal(sr_in, L, seed=0):
    """0.2 N(0, 1) noise + the three tones, f32"""
    rng = np.random.default_rng(1000 * seed + sr_in % 997 + L)
    x = (0.2 * rng.standard_normal(L) + R.tones(sr_in, L, sr_in)).astype(np.float32)
    x.setflags(write=False)
    return x


def run(rows, sr_in, normalize=False, extra_L=7, extra_out=5, fe=None):
    """resample the utterances `rows` as one batch -> (out [B, Lw] with Lw = max L_out + extra_out, out_lens, tail beyond the buffer)"""
    fe = fe or frontend()
    B, lens = len(rows), np.asarray([r.size for r in rows], np.int32)
    wav = np.full((B, int(lens.max()) + extra_L), np.nan, np.float32)
    for b, r in enumerate(rows):
        wav[b, :r.size] = r
    Lw = max(R.out_len(sr_in, SR_OUT, int(n)) for n in lens) + extra_out
    buf = torch.full((B * Lw + 11,), float(SENT), device="cuda", dtype=torch.float32)
    _, out_lens = fe.resample(dev(wav), sr_in, lens, normalize=normalize, out=buf[:B * Lw].view(B, Lw))
    got = buf.cpu().numpy()
    return got[:B * Lw].reshape(B, Lw), out_lens, got[B * Lw:]


def check_against_reference(y, x, sr_in):
    o, n, width, K = R.rule(sr_in, SR_OUT)
    h = lib_table(sr_in)
    ref = R.apply(h, x, o, width, y.size)
    lim = (K + 2) * 2.0 ** -24 * R.bound(h, x, o, width, y.size)
    err = np.abs(y.astype(np.float64) - ref)
    rel = np.linalg.norm(y - ref) / np.linalg.norm(ref)
    print(f"sr_in {sr_in} L {x.size}: worst err / bound {np.max(err / np.maximum(lim, 1e-300)):.3g}, rel L2 {rel:.3g}")
    assert np.isfinite(y).all()
    assert (err <= lim).all()
    assert rel <= 2e-6


@pytest.mark.parametrize("sr_in", GPU_RATES)
def test_ratios_and_lengths(sr_in):
    """one utterance per launch: a single sample, shorter than every filter, whole blocks, a partial last block, one second
    (several workgroup tiles at every ratio: the seams between tiles)"""
    o, n, _, _ = R.rule(sr_in, SR_OUT)
    for L in (1, 50, o * 37, o * 37 + 1, sr_in):
        x = signal(sr_in, L)
        out, out_lens, tail = run([x], sr_in)
        Lo = math.ceil(n * L / o)
        assert out_lens.tolist() == [Lo]
        assert not out[0, Lo:].any() and (tail == SENT).all()
        check_against_reference(out[0, :Lo], x, sr_in)


def test_ragged_batch_is_its_utterances_alone():
    sr_in = 44100
    rows = [signal(sr_in, L, seed=1) for L in (44100, 50, 17001)]
    out, out_lens, tail = run(rows, sr_in)
    from megatts2_amd import runtime
    assert out_lens.tolist() == [runtime.resample_query(sr_in, SR_OUT, r.size)[0] for r in rows]
    assert (tail == SENT).all()
    wider, wider_lens, _ = run(rows, sr_in, extra_L=7 + 13)
    assert np.array_equal(out, wider) and np.array_equal(out_lens, wider_lens)
    for b, r in enumerate(rows):
        Lo = int(out_lens[b])
        assert np.isfinite(out[b]).all()                    # the NaN padding was not read
        assert not out[b, Lo:].any()
        alone, _, _ = run([r], sr_in)
        assert np.array_equal(out[b, :Lo], alone[0, :Lo])
        check_against_reference(out[b, :Lo], r, sr_in)


def test_normalize_is_division_by_the_peak():
    sr_in = 48000
    rows = [signal(sr_in, 24000, seed=2), np.zeros(3000, np.float32), (1e-3 * signal(sr_in, 1000, seed=3)).astype(np.float32)]
    raw, out_lens, _ = run(rows, sr_in)
    nrm, nrm_lens, tail = run(rows, sr_in, normalize=True)
    assert np.array_equal(out_lens, nrm_lens) and (tail == SENT).all()
    for b, r in enumerate(rows):
        Lo = int(out_lens[b])
        want = R.normalize(raw[b, :Lo])
        assert np.array_equal(nrm[b, :Lo], want) and not nrm[b, Lo:].any()
        if r.any():
            assert np.abs(nrm[b, :Lo]).max() == 1.0
        else:
            assert not nrm[b].any()
        alone, _, _ = run([r], sr_in, normalize=True)       # no utterance sees another's peak
        assert np.array_equal(nrm[b, :Lo], alone[0, :Lo])


def test_from_audio_composes_resample_normalize_mel():
    from megatts2_amd import audio_io, config
    from megatts2_amd.runtime import MelFrontEnd
    fe = MelFrontEnd(config.AudioConfig(sample_rate=SR_OUT, n_fft=64, hop_length=16, win_length=64, n_mels=8, f_min=0.0, f_max=8000.0))
    rows = [signal(44100, L, seed=4) for L in (9000, 4410)]
    lens = np.asarray([r.size for r in rows], np.int32)
    wav = np.zeros((2, 9000), np.float32)
    for b, r in enumerate(rows):
        wav[b, :r.size] = r
    mel, mel_lens = fe.from_audio(dev(wav), 44100, lens)
    y, out_lens = fe.resample(dev(wav), 44100, lens, normalize=True)
    assert np.array_equal(mel_lens, 1 + out_lens // 16)
    assert torch.equal(mel, fe(y, out_lens))
    # audio at the model's rate: normalised only
    host = np.stack([np.concatenate([audio_io.normalize(wav[b, :n]), np.zeros(9000 - n, np.float32)]) for b, n in enumerate(lens)])
    mel16, mel16_lens = fe.from_audio(dev(wav), SR_OUT, lens)
    assert np.array_equal(mel16_lens, 1 + lens // 16)
    assert torch.equal(mel16, fe(dev(host), lens))
    fe.close()


def test_forward_accepts_a_44k1_prompt(tmp_path):
    """Megatts.forward on a 44.1 kHz prompt is forward on the 16 kHz file the GPU resampler makes of it (float WAV is lossless;
    the host normalises that file with the same f32 division the device applies)."""
    from megatts2_amd import audio_io
    from megatts2_amd import megatts2 as M
    (g, p, a, _), (sd_g, sd_p, sd_a, _) = synth_models("tiny")
    tts = M.Megatts(models=(M.MegaG(g, sd_g), M.MegaPLM(p, sd_p), M.MegaADM(a, sd_a)))
    x = (0.3 * signal(44100, int(0.6 * 44100), seed=5)).astype(np.float32)
    dir_a, dir_b = tmp_path / "a", tmp_path / "b"
    dir_a.mkdir()
    dir_b.mkdir()
    audio_io.write_wav(str(dir_a / "prompt.wav"), x, 44100)
    raw, out_lens = frontend().resample(dev(x[None]), 44100)
    audio_io.write_wav(str(dir_b / "prompt.wav"), raw[0, :int(out_lens[0])].cpu().numpy(), SR_OUT)
    phone = np.random.default_rng(6).integers(0, g.mrte.phone_vocab_size, 6)
    mel_a, lens_a, aux_a = tts.forward(str(dir_a), phone_tokens=phone, out_path=None)
    mel_b, lens_b, aux_b = tts.forward(str(dir_b), phone_tokens=phone, out_path=None)
    assert np.array_equal(np.asarray(lens_a), np.asarray(lens_b))
    assert torch.equal(mel_a, mel_b) and torch.equal(aux_a["dur"], aux_b["dur"]) and torch.equal(aux_a["codes"], aux_b["codes"])
    with pytest.raises(ValueError):
        tts.forward(str(dir_a), phone_tokens=phone, out_path=None, resample=False)


def test_device_call_rejects_before_launch():
    """each case is refused on the host: nothing is launched and the output keeps its sentinel"""
    from megatts2_amd import runtime
    fe, sr_in = frontend(), 24000
    x = np.stack([signal(sr_in, 3000, seed=7), signal(sr_in, 3000, seed=8)])
    Lo = runtime.resample_query(sr_in, SR_OUT, 3000)[0]

    def refused(lens, width):
        out = torch.full((2, width), float(SENT), device="cuda", dtype=torch.float32)
        with pytest.raises(runtime.NativeError):
            fe.resample(dev(x), sr_in, np.asarray(lens, np.int32), out=out)
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == SENT).all()

    refused([3000, 3000], Lo - 1)          # Lout_max too small
    refused([3000, 0], Lo)                 # an empty utterance
    refused([3001, 3000], Lo + 1)          # longer than L_max
    out = torch.full((2, Lo), float(SENT), device="cuda", dtype=torch.float32)
    fe.resample(dev(x), sr_in, out=out)    # and the same call with valid arguments goes through
    assert np.isfinite(out.cpu().numpy()).all() and not (out.cpu().numpy() == SENT).all()
