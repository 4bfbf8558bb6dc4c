"""The prompt-audio silence trimmer on the GPU (csrc/trim.hip, mt2_trim_silence) against the float64 restatement of its rule
(tests/trim_ref.py) applied to the same f32 input.

Bars: the bounds EQUAL the reference's - asserted only after the reference itself shows that no frame of the input lies within
relative 1e-3 of the threshold (an f32 sum of 2052 non-negative terms errs by at most 2052 * 2^-24 = 1.2e-4 relative, in any order,
with or without fma) -, the output is a bit-exact slice, and each frame energy is within 2052 * 2^-24 * e_ref of the reference.
Input padding beyond lens[b] is NaN (a read of it poisons the energies), the output buffer is pre-filled with a sentinel and is
wider than needed.  The block sums run 16 blocks = 8192 samples to a workgroup: L = 16000 spans 2 workgroups, L = 48000 spans 6,
every other length here one."""
import functools

import numpy as np
import pytest

import trim_ref as T
from conftest import synth_models

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT = np.float32(-77.25)
EPS_SUM = 2052 * 2.0 ** -24
MARGIN = 1e-3
LENGTHS = (1, 511, 512, 513, 2047, 2048, 2049, 5000, 16000, 48000)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def frontend():
    from megatts2_amd.runtime import MelFrontEnd
    return MelFrontEnd()


def run(rows, top_db, extra_L=7, extra_out=5, fe=None):
    """trim the utterances `rows` as one batch -> (out [B, Lw] with Lw = max L + extra_out, out_lens, bounds, energy [B, F],
    the words behind the output buffer)"""
    fe = fe or frontend()
    B, lens = len(rows), np.asarray([r.size for r in rows], np.int32)
    wav = np.full((B, int(lens.max()) + extra_L), np.nan, np.float32)
    for b, r in enumerate(rows):
        wav[b, :r.size] = r
    Lw = int(lens.max()) + extra_out
    buf = torch.full((B * Lw + 11,), float(SENT), device="cuda", dtype=torch.float32)
    _, out_lens, bounds, energy = fe.trim(dev(wav), lens, top_db, out=buf[:B * Lw].view(B, Lw), return_energy=True)
    got = buf.cpu().numpy()
    return got[:B * Lw].reshape(B, Lw), out_lens, bounds, energy.cpu().numpy(), got[B * Lw:]


def check_against_reference(x, top_db, out_row, out_len, bound, energy_row):
    L = x.size
    m = T.margin(x, top_db)
    assert m >= MARGIN, f"the test input has a frame within {m:.3g} of the threshold: choose another input, not another bar"
    start, end = T.bounds(x, top_db)
    assert (int(bound[0]), int(bound[1])) == (start, end) and int(out_len) == end - start
    assert start % 512 == 0 and 0 <= start < end <= L
    assert np.array_equal(out_row[:end - start], x[start:end])            # a bit-exact slice
    assert not out_row[end - start:].any()                                # zeros up to Lout_max
    e_ref, F = T.energies(x), 1 + L // 512
    assert np.isfinite(energy_row).all() and not energy_row[F:].any()
    err = np.abs(energy_row[:F].astype(np.float64) - e_ref)
    print(f"L {L} top_db {top_db}: cut [{start}, {end}), margin {m:.3g}, worst energy error / bound "
          f"{np.max(err / np.maximum(EPS_SUM * e_ref, 1e-300)):.3g}")
    assert (err <= EPS_SUM * e_ref).all()


@pytest.mark.parametrize("L", LENGTHS)
def test_lengths_thresholds_and_burst_places(L):
    """one utterance per launch"""
    for where in ("start", "interior", "end"):
        x = T.burst_signal(L, where)
        for top_db in (20, 40):
            out, out_lens, bounds, energy, tail = run([x], top_db)
            assert (tail == SENT).all()
            check_against_reference(x, top_db, out[0], out_lens[0], bounds[0], energy[0])


def test_the_cut_really_cuts():
    """the inputs above are not all left whole: at one second with the burst inside, both ends go"""
    x = T.burst_signal(16000, "interior")
    _, out_lens, bounds, _, _ = run([x], 40)
    assert bounds[0, 0] >= 2048 and bounds[0, 1] <= 16000 - 2048 and out_lens[0] == bounds[0, 1] - bounds[0, 0]


def test_ragged_batch_is_its_utterances_alone():
    rows = [T.burst_signal(16000, "interior", seed=1), np.array([0.25], np.float32), T.burst_signal(5000, "end", seed=2),
            np.zeros(3000, np.float32)]
    out, out_lens, bounds, energy, tail = run(rows, 40)
    assert (tail == SENT).all()
    assert bounds[3].tolist() == [0, 3000] and bounds[1].tolist() == [0, 1]          # silence and a single sample are left whole
    assert not energy[3].any() and not out[3].any()
    wider = run(rows, 40, extra_L=7 + 13)
    for a, w in zip((out, out_lens, bounds, energy), wider):
        assert np.array_equal(a, w)
    for b, r in enumerate(rows):
        alone, alone_lens, alone_bounds, alone_energy, _ = run([r], 40)
        n, F = int(out_lens[b]), 1 + r.size // 512
        assert np.array_equal(alone_bounds[0], bounds[b]) and alone_lens[0] == n
        assert np.array_equal(out[b, :n], alone[0, :n]) and not out[b, n:].any()
        assert np.array_equal(energy[b, :F], alone_energy[0, :F]) and not energy[b, F:].any()      # bit-identical, energies included
        if r.any():
            check_against_reference(r, 40, out[b], out_lens[b], bounds[b], energy[b])


def test_non_finite_samples_give_bounds_inside_the_utterance():
    x = T.burst_signal(5000, "interior", seed=3).copy()
    x[1234], x[4000] = np.nan, np.inf
    _, out_lens, bounds, _, tail = run([x, x[:700]], 20)
    assert (tail == SENT).all()
    for b, L in enumerate((5000, 700)):
        assert 0 <= bounds[b, 0] <= bounds[b, 1] <= L and out_lens[b] == bounds[b, 1] - bounds[b, 0]


def test_device_call_rejects_before_launch():
    """each case is refused on the host: nothing is launched and the output keeps its sentinel"""
    from megatts2_amd import runtime
    fe = frontend()
    base = torch.full((9000,), float(SENT), device="cuda", dtype=torch.float32)
    x = base[:6000].view(2, 3000)
    x.copy_(dev(np.stack([T.burst_signal(3000, "interior", seed=4), T.burst_signal(3000, "end", seed=5)])))

    def refused(lens, width, top_db=40.0, energy_frames=None, out=None):
        out = torch.full((2, width), float(SENT), device="cuda", dtype=torch.float32) if out is None else out
        before = out.clone()
        with pytest.raises(runtime.NativeError):
            if energy_frames is None:
                fe.trim(x, np.asarray(lens, np.int32), top_db, out=out)
            else:           # the C entry point itself, with an energy buffer that is too narrow
                ln, energy = np.asarray(lens, np.int32), torch.full((2, energy_frames), float(SENT), device="cuda")
                runtime._check(fe.lib.mt2_trim_silence(fe.h, runtime._stream(), runtime._ptr(x), runtime._iptr(ln), 3000, 2, top_db,
                                                       runtime._ptr(out), width, None, runtime._ptr(energy), energy_frames))
        torch.cuda.synchronize()
        assert torch.equal(out, before)

    refused([3000, 3000], 3000, top_db=0.0)
    refused([3000, 3000], 3000, top_db=-20.0)
    refused([3000, 3000], 3000, top_db=float("nan"))
    refused([3000, 3000], 3000, top_db=float("inf"))
    refused([3000, 0], 3000)                       # an empty utterance
    refused([3001, 3000], 3001)                    # longer than L_max
    refused([3000, 2000], 2999)                    # Lout_max below the longest utterance
    refused([3000, 3000], 3000, energy_frames=1 + 3000 // 512 - 1)
    refused([3000, 3000], 3000, out=x)             # out is wav
    refused([3000, 3000], 3000, out=base[3000:9000].view(2, 3000))          # out's first row is wav's second
    out = torch.full((2, 3000), float(SENT), device="cuda", dtype=torch.float32)
    fe.trim(x, out=out, top_db=40.0)               # and the same call with valid arguments goes through
    assert np.isfinite(out.cpu().numpy()).all() and not (out.cpu().numpy() == SENT).all()


def test_from_audio_composes_resample_normalize_trim_mel():
    fe = frontend()
    assert fe.audio.hop_length == 256
    rows = [T.burst_signal(L, where, seed=6) for L, where in ((30000, "interior"), (14000, "end"))]       # "44.1 kHz" audio
    lens = np.asarray([r.size for r in rows], np.int32)
    wav = np.zeros((2, 30000), np.float32)
    for b, r in enumerate(rows):
        wav[b, :r.size] = r
    mel, mel_lens, bounds = fe.from_audio(dev(wav), 44100, lens, trim_db=40, return_bounds=True)
    y, y_lens = fe.resample(dev(wav), 44100, lens, normalize=True)
    cut, cut_lens, cut_bounds = fe.trim(y, y_lens, 40)
    assert np.array_equal(bounds, cut_bounds) and np.array_equal(cut_lens, bounds[:, 1] - bounds[:, 0])
    assert (cut_lens < y_lens).all()                                                     # something was cut
    assert np.array_equal(mel_lens, 1 + (bounds[:, 1] - bounds[:, 0]) // 256)
    assert torch.equal(mel, fe(cut, cut_lens))
    assert len(fe.from_audio(dev(wav), 44100, lens, trim_db=40)) == 2
    # trim_db=None: the parent's two steps, bit for bit
    mel0, mel0_lens = fe.from_audio(dev(wav), 44100, lens)
    assert np.array_equal(mel0_lens, 1 + y_lens // 256) and torch.equal(mel0, fe(y, y_lens))
    whole = fe.from_audio(dev(wav), 44100, lens, return_bounds=True)[2]
    assert np.array_equal(whole, np.stack([np.zeros_like(y_lens), y_lens], axis=1))


def test_forward_trims_every_prompt(tmp_path):
    """Megatts.forward(trim_db=40) on one 16 kHz and one 44.1 kHz prompt with silence around the speech is `synthesize` on the
    concatenated from_audio(trim_db=40) mels; trim_db=None still takes the untrimmed files."""
    from megatts2_amd import audio_io
    from megatts2_amd import megatts2 as M
    (g, p, a, _), (sd_g, sd_p, sd_a, _) = synth_models("tiny")
    tts = M.Megatts(models=(M.MegaG(g, sd_g), M.MegaPLM(p, sd_p), M.MegaADM(a, sd_a)))
    files = []
    for name, sr, seed in (("a16k.wav", 16000, 7), ("b44k.wav", 44100, 8)):
        speech = 0.6 * T.burst_signal(int(0.4 * sr), "interior", seed=seed, floor=0.05)
        x = np.concatenate([np.zeros(int(0.3 * sr), np.float32), speech, np.zeros(int(0.2 * sr), np.float32)]).astype(np.float32)
        audio_io.write_wav(str(tmp_path / name), x, sr)
        files.append((x, sr))
    fe = M._frontend()
    parts = [fe.from_audio(dev(x[None]), sr, trim_db=40, return_bounds=True) for x, sr in files]
    for mel, mel_lens, bounds in parts:
        assert bounds[0, 0] > 0 and mel.shape[1] == mel_lens[0] == 1 + (bounds[0, 1] - bounds[0, 0]) // 256
    mels = torch.cat([mel[0] for mel, _, _ in parts], dim=0).unsqueeze(0)
    phone = np.random.default_rng(9).integers(0, g.mrte.phone_vocab_size, 6)
    want_mel, want_lens, want_aux = tts.synthesize(dev(phone.reshape(1, -1).astype(np.int64)), mels, return_aux=True)
    mel, mel_lens, aux = tts.forward(str(tmp_path), phone_tokens=phone, out_path=None, trim_db=40)
    assert np.array_equal(np.asarray(mel_lens), np.asarray(want_lens))
    assert torch.equal(mel, want_mel) and torch.equal(aux["dur"], want_aux["dur"]) and torch.equal(aux["codes"], want_aux["codes"])
    untrimmed = torch.cat([fe.from_audio(dev(x[None]), sr)[0][0] for x, sr in files], dim=0).unsqueeze(0)
    assert untrimmed.shape[1] > mels.shape[1]
    mel_u, lens_u, _ = tts.forward(str(tmp_path), phone_tokens=phone, out_path=None)
    want_u, want_lens_u = tts.synthesize(dev(phone.reshape(1, -1).astype(np.int64)), untrimmed)
    assert np.array_equal(np.asarray(lens_u), np.asarray(want_lens_u)) and torch.equal(mel_u, want_u)
