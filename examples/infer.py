"""The reference's infer.py (infer.py:1-18) on the MI355X path.

    python examples/infer.py --g-ckpt generator.ckpt --g-config configs/config_gan.yaml \
        --plm-ckpt plm.ckpt --plm-config configs/config_plm.yaml --adm-ckpt adm.ckpt --adm-config configs/config_adm.yaml \
        --symbol-table unique_text_tokens.k2symbols --wavs-dir prompts/ --text "..." [--phones 12,7,...]

Checkpoints are the reference's Lightning files (or `.mt2` packed files written by
`megatts2_amd.audio_io.save_packed`); configs are the reference's YAML files.  Text input needs the reference's
G2P on sys.path (pypinyin + its MFA dictionary); `--phones` passes token ids directly.  With `--synthetic` the
name-seeded synthetic weights are used instead of checkpoints (no checkpoint ships with the reference).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> None:
    ap = argparse.ArgumentParser()
    for k in ("g", "plm", "adm"):
        ap.add_argument(f"--{k}-ckpt")
        ap.add_argument(f"--{k}-config")
    ap.add_argument("--symbol-table")
    ap.add_argument("--wavs-dir", required=True, help="prompt *.wav files, any sample rate (resampled to 16 kHz on the GPU)")
    ap.add_argument("--trim-db", type=float, help="cut the prompts' leading / trailing silence below this many dB under their peak frame (e.g. 40)")
    ap.add_argument("--vocoder", choices=("hifigan", "griffin-lim"), default="hifigan",
                    help="hifigan: the hub model's generator, when a local copy is found; griffin-lim: no weights needed (buzzy: a fallback)")
    ap.add_argument("--gl-iters", type=int, default=32, help="Griffin-Lim iterations")
    ap.add_argument("--report-pitch", action="store_true",
                    help="print the pitch moments (F0 tracked on the GPU, see --pitch-tracker) of the first prompt and, when a vocoder produced audio, of the generated audio")
    ap.add_argument("--pitch-tracker", choices=("yin", "viterbi"), default="yin",
                    help="--report-pitch by plain YIN, or by the Viterbi pass over its lag costs (robust to octave errors)")
    ap.add_argument("--report-prosody", action="store_true",
                    help="print the duration moments of the output and, when a vocoder produced audio, one line per phone (frames, voiced frames, "
                         "mean Hz, semitones above 55 Hz, energy in dB; F0 by --pitch-tracker) and the DTW pitch-contour distance between the "
                         "first prompt and the generated audio")
    ap.add_argument("--output-lufs", type=float,
                    help="bring the vocoded prompt and the generated audio each to this integrated loudness (ITU-R BS.1770, e.g. -23) before they are written")
    ap.add_argument("--peak-ceiling", type=float, default=0.0, help="with --output-lufs: cap the gain so that the sample peak stays at or below this (e.g. 0.99)")
    ap.add_argument("--true-peak-ceiling", type=float, metavar="DB",
                    help="with --output-lufs: cap the gain so that the true peak (oversampled to at least 192 kHz) stays at or below this many dBTP "
                         "(e.g. -1, what EBU R 128 delivery asks); not together with --peak-ceiling")
    ap.add_argument("--limiter", action="store_true",
                    help="with --output-lufs and --true-peak-ceiling: reach the loudness under the ceiling by a look-ahead limiter that turns down the "
                         "crests alone, where one gain would land under the target; --report-ebu then prints what it did")
    ap.add_argument("--limiter-window-ms", type=float, default=5.0, metavar="MS", help="with --limiter: how far the gain looks ahead and behind (default 5)")
    ap.add_argument("--limiter-passes", type=int, default=2, metavar="P", help="with --limiter: passes that re-measure and correct the loudness, 1 to 4 (default 2)")
    ap.add_argument("--report-ebu", action="store_true",
                    help="print true peak in dBTP, loudness range (EBU Tech 3342) and maximum short-term and momentary loudness (measured on the "
                         "GPU) of the first prompt and, when a vocoder produced audio, of the generated audio")
    ap.add_argument("--report-loudness", action="store_true",
                    help="print integrated LUFS, sample peak in dBFS and block counts (measured on the GPU) of the first prompt and, when a vocoder produced audio, of the generated audio")
    ap.add_argument("--denoise-prompt", action="store_true",
                    help="suppress stationary noise (hiss, room tone, hum) in every prompt file on the GPU before its mel is taken: a per-bin "
                         "quantile noise floor and a spectral gate; a STEADY tone is removed like hum")
    ap.add_argument("--denoise-percentile", type=int, default=20, metavar="P",
                    help="with --denoise-prompt: the percentile of a bin's power over time taken as its noise floor, 1 to 99 (default 20); "
                         "speech present in a bin for more than 100 - P %% of the frames raises that bin's floor")
    ap.add_argument("--denoise-strength", type=float, default=3.0, metavar="BETA", help="with --denoise-prompt: the over-subtraction factor (default 3)")
    ap.add_argument("--denoise-floor-db", type=float, default=-20.0, metavar="DB", help="with --denoise-prompt: the least gain of a cell in dB, at most 0 (default -20)")
    ap.add_argument("--report-noise", action="store_true",
                    help="print, for each prompt file, the estimated noise power and SNR, the share of cells at the floor gain and the power "
                         "reduction in dB (measured on the GPU; the prompts are denoised only with --denoise-prompt)")
    ap.add_argument("--dereverb-prompt", action="store_true",
                    help="remove late reverberation from every prompt file on the GPU before its mel is taken (and before --denoise-prompt): "
                         "weighted prediction error, a per-bin prediction filter; discrete reflections go, diffuse tails are helped only "
                         "modestly, a STEADY tone is removed like a reflection")
    ap.add_argument("--dereverb-taps", type=int, default=10, metavar="K", help="with --dereverb-prompt: the length of the prediction filter in frames, 1 to 16 (default 10)")
    ap.add_argument("--dereverb-delay", type=int, default=3, metavar="D", help="with --dereverb-prompt: the frames skipped before the prediction, 1 to 8 (default 3)")
    ap.add_argument("--dereverb-iterations", type=int, default=3, metavar="I", help="with --dereverb-prompt: variance / filter passes, 1 to 8 (default 3)")
    ap.add_argument("--report-reverb", action="store_true",
                    help="print, for each prompt file, the power the de-reverberation removes in dB and the bins filtered and passed through "
                         "(measured on the GPU; the prompts are de-reverberated only with --dereverb-prompt)")
    ap.add_argument("--declip-prompt", action="store_true",
                    help="restore the clipped samples of every prompt file on the GPU, first of all and at the file's own sample rate (sparse "
                         "restoration, A-SPADE): hard clipping with flat tops only - soft clipping, or clipping behind a resampler or a lossy "
                         "codec, is not detected; the restoration is a sparse guess, not the original")
    ap.add_argument("--declip-frame", type=int, default=1024, metavar="N", help="with --declip-prompt: the frame length, 256, 512, 1024 or 2048 samples (default 1024)")
    ap.add_argument("--declip-tol", type=float, default=1e-3, metavar="X", help="with --declip-prompt / --report-clipping: samples within X of the extreme, relative, count as clipped (default 1e-3)")
    ap.add_argument("--declip-eps", type=float, default=0.02, metavar="E", help="with --declip-prompt: a frame stops once its residual is under E of its norm (default 0.02)")
    ap.add_argument("--report-clipping", action="store_true",
                    help="print, for each prompt file, whether it is clipped, the two levels and the share of samples at them, and with "
                         "--declip-prompt the iterations and the power change; alone it only detects (on the GPU) and warns")
    ap.add_argument("--cut-prompt-pauses", action="store_true",
                    help="cut the pauses out of every prompt file on the GPU, its ends included (speech segments by frame energy, in place of "
                         "--trim-db): the threshold is relative to the loudest frame, so room tone above it reads as speech and nothing is cut; "
                         "a breath is speech or pause by its level alone; no cross-fade")
    ap.add_argument("--pause-db", type=float, default=40.0, metavar="DB", help="with --cut-prompt-pauses / --report-pauses: a frame is active above this many dB under the loudest frame (default 40)")
    ap.add_argument("--min-pause-ms", type=float, default=320.0, metavar="MS", help="... pauses shorter than this stay (default 320)")
    ap.add_argument("--min-speech-ms", type=float, default=96.0, metavar="MS", help="... runs of speech shorter than this are dropped (default 96)")
    ap.add_argument("--pause-pad-ms", type=float, default=64.0, metavar="MS", help="... kept on both sides of every segment; under half of --min-pause-ms (default 64)")
    ap.add_argument("--report-pauses", action="store_true",
                    help="print, for each prompt file, its speech segments, the seconds of speech of the total, the longest pause and the "
                         "speech / pause energy ratio in dB (measured on the GPU); alone it only reports, nothing is cut")
    ap.add_argument("--report-formants", action="store_true",
                    help="print, for the first prompt file and for the generated audio, the voiced frames used, the mean and sigma of F1 .. F4 "
                         "and the vocal-tract length they imply (linear prediction on the GPU), then the length ratio and the formants' "
                         "differences in per cent: whether the output has the prompt's vocal tract, whatever the text; alone it only reports")
    ap.add_argument("--max-formant", type=float, default=5500.0, metavar="HZ",
                    help="with --report-formants: the formant ceiling; the audio is analysed at twice this rate (5500 for a female voice, 5000 for a male one)")
    ap.add_argument("--lpc-order", type=int, default=10, metavar="P", help="with --report-formants: the order of the all-pole fit, even, 2 to 32 (default 10)")
    ap.add_argument("--track-formants", action="store_true",
                    help="with --report-formants: track the candidates across frames first (a Viterbi pass on the GPU: of every frame's candidates "
                         "those on the cheapest smooth path), so that one spurious root does not shift every formant above it; also prints the "
                         "share of frames where the tracked selection differs from the first K candidates")
    ap.add_argument("--formant-tracks", type=int, default=4, metavar="K", help="with --track-formants: the number of tracks, 1 to 5 (default 4; the figures need 4)")
    ap.add_argument("--formant-jump-cost", type=float, default=1.0, metavar="X",
                    help="with --track-formants: the cost of a relative change of a track between frames (default 1; 0: every frame on its own)")
    ap.add_argument("--reference-wav", metavar="PATH",
                    help="a recording of the same sentence: print the mel-cepstral distortion (dB, along the DTW path of the cepstra), the largest "
                         "cell, and F0 RMSE, register offset and voiced / unvoiced error along the same path, of the generated audio against it")
    ap.add_argument("--mcd-order", type=int, default=13, metavar="K", help="with --reference-wav: cepstral coefficients c1 .. cK compared (default 13)")
    ap.add_argument("--text")
    ap.add_argument("--phones", help="comma separated phone token ids (bypasses the G2P)")
    ap.add_argument("--out", default="test.wav")
    ap.add_argument("--synthetic", action="store_true")
    a = ap.parse_args()

    from megatts2_amd import config as C, megatts2 as M, weights
    if a.synthetic:
        g, p, d, h = C.production_g(), C.production_plm(), C.production_adm(), C.production_hifigan()
        sd = lambda inv, pre: weights.synth_state_dict(inv, 0, pre)   # noqa: E731
        tts = M.Megatts(models=(M.MegaG(g, sd(weights.inventory_g(g), "G.")), M.MegaPLM(p, sd(weights.inventory_plm(p), "plm.")),
                                M.MegaADM(d, sd(weights.inventory_adm(d), "adm."))),
                        hifi_gan=M.HIFIGAN(h, sd(weights.inventory_hifigan(h), "hifigan.")))
    else:
        tts = M.Megatts(a.g_ckpt, a.g_config, a.plm_ckpt, a.plm_config, a.adm_ckpt, a.adm_config, a.symbol_table)
    tts.eval()
    phones = [int(v) for v in a.phones.split(",")] if a.phones else None
    gl = {"n_iter": a.gl_iters} if a.vocoder == "griffin-lim" else None
    dn = M.Denoise(a.denoise_percentile, a.denoise_strength, 10.0 ** (a.denoise_floor_db / 20.0))
    dr = M.Dereverb(delay=a.dereverb_delay, taps=a.dereverb_taps, iterations=a.dereverb_iterations)
    dc = M.Declip(frame=a.declip_frame, tol=a.declip_tol, eps=a.declip_eps)
    pa = M.Pauses(top_db=a.pause_db, min_pause_ms=a.min_pause_ms, min_speech_ms=a.min_speech_ms, pad_ms=a.pause_pad_ms)
    mel, lens, aux = tts(a.wavs_dir, a.text, phone_tokens=phones, out_path=a.out, trim_db=a.trim_db, vocoder=gl, loudness_lufs=a.output_lufs,
                         peak_ceiling=a.peak_ceiling, true_peak_ceiling_dbtp=a.true_peak_ceiling,
                         **({"limiter": M.Limiter(a.limiter_window_ms, a.limiter_passes)} if a.limiter else {}),
                         **({"denoise": dn} if a.denoise_prompt else {}), **({"dereverb": dr} if a.dereverb_prompt else {}),
                         **({"declip": dc} if a.declip_prompt else {}), **({"cut_pauses": pa} if a.cut_prompt_pauses else {}))
    wrote = gl is not None or tts.hifi_gan is not None
    print(f"{int(lens[0])} mel frames -> {a.out if wrote else '(no vocoder loaded: mel only; --vocoder griffin-lim needs none)'}")
    if a.report_pauses:
        import glob
        import math
        from megatts2_amd import audio_io
        paths = sorted(glob.glob(f"{a.wavs_dir}/*.wav"))
        # with --cut-prompt-pauses the figures of the stage that ran (at 16 kHz, behind the other stages); without it a measurement of
        # the file as it is, at its own rate, nothing is changed
        rows = []
        for i, path in enumerate(paths):
            if a.cut_prompt_pauses:
                rows.append((aux["prompt_pauses"][i], C.HIFIGAN_SR))
            else:
                y, sr = audio_io.read_wav(path)
                st = M.speech_segments(y, sr, pauses=pa)
                rows.append(({k: float(st[k if k != "segments" else "n_segments"][0]) for k in M.PAUSES_NAMES}, sr))
        for path, (st, sr) in zip(paths, rows):
            total = 512 * (st["frames"] - 1)            # to a frame
            speech = st["kept_samples"] if st["segments"] > 0 else 0.0
            ratio = (f"{10 * math.log10(st['kept_energy'] / st['dropped_energy']):.1f} dB" if st["kept_energy"] > 0 and st["dropped_energy"] > 0
                     else "n/a (nothing on one side)")
            if st["segments"] < 0:
                print(f"pauses of the prompt {path}: no speech segment found at {a.pause_db:g} dB: the file is left whole")
            else:
                print(f"pauses of the prompt {path}{' (cut)' if a.cut_prompt_pauses else ''}: {int(st['segments'])} segments, {speech / sr:.2f} s of speech "
                      f"of about {total / sr:.2f} s, longest pause {512 * st['longest_pause'] / sr:.2f} s, speech / pause energy {ratio}")
    if a.report_clipping:
        import glob
        from megatts2_amd import audio_io
        paths = sorted(glob.glob(f"{a.wavs_dir}/*.wav"))
        # with --declip-prompt the figures of the stage that ran; without it detection alone on the file as it is, nothing is changed
        rows = aux["prompt_clipping"] if a.declip_prompt else [{k: float(v[0]) for k, v in M.detect_clipping(audio_io.read_wav(p)[0], declip=dc).items()}
                                                                 for p in paths]
        for path, st in zip(paths, rows):
            if not st["clipped"]:
                print(f"clipping of the prompt {path}: none detected (extremes {st['lo']:.4f} and {st['hi']:.4f})")
            elif a.declip_prompt:
                print(f"clipping of the prompt {path} (restored): levels {st['lo']:.4f} and {st['hi']:.4f}, {100 * st['share']:.2f} % of the samples, "
                      f"{int(st['frames_iterated'])} frames iterated, {st['mean_iterations']:.1f} iterations on average and {int(st['max_iterations'])} "
                      f"at most, power {st['power_change_db']:+.2f} dB")
            else:
                print(f"WARNING: the prompt {path} is clipped: levels {st['lo']:.4f} and {st['hi']:.4f}, {100 * st['share']:.2f} % of the samples; its "
                      f"distortion goes into the cloned voice (--declip-prompt restores it)")
    if a.report_reverb:
        import glob
        from megatts2_amd import audio_io
        paths = sorted(glob.glob(f"{a.wavs_dir}/*.wav"))
        # with --dereverb-prompt the figures of the stage that ran; without it a measurement of the file, nothing is changed
        rows = aux["prompt_reverb"] if a.dereverb_prompt else [{k: float(v[0]) for k, v in M.dereverb_audio(*audio_io.read_wav(p), dereverb=dr)[1].items()
                                                                 if k in M.WPE_NAMES} for p in paths]
        for path, st in zip(paths, rows):
            print(f"reverberation of the prompt {path}{' (removed)' if a.dereverb_prompt else ' (measured only)'}: power {st['reduction_db']:.2f} dB, "
                  f"{int(st['bins_filtered'])} bins filtered and {int(st['bins_passed'])} passed through over {int(st['frames'])} frames, largest tap "
                  f"{st['max_tap']:.3f}")
    if a.report_noise:
        import glob
        from megatts2_amd import audio_io
        paths = sorted(glob.glob(f"{a.wavs_dir}/*.wav"))
        # with --denoise-prompt the figures of the suppression that ran; without it a measurement of the file, nothing is changed
        rows = aux["prompt_noise"] if a.denoise_prompt else [{k: float(v[0]) for k, v in M.denoise_audio(*audio_io.read_wav(p), denoise=dn)[1].items()
                                                               if k in M.DENOISE_NAMES} for p in paths]
        for path, st in zip(paths, rows):
            print(f"noise of the prompt {path}{' (suppressed)' if a.denoise_prompt else ' (measured only)'}: floor {st['noise_db']:.2f} dB, "
                  f"estimated SNR {st['snr_db']:.2f} dB, {100 * st['floored_share']:.1f} % of the cells at the floor gain, power "
                  f"{st['reduction_db']:.2f} dB, percentile {a.denoise_percentile} = rank {int(st['rank'])} of {int(st['frames'])} frames")
    if a.report_loudness:
        import glob
        import math
        from megatts2_amd import audio_io
        path = sorted(glob.glob(f"{a.wavs_dir}/*.wav"))[0]
        y, sr = audio_io.read_wav(path)
        report = [(f"first prompt ({path}, as the file holds it)", M.measure_loudness(y, sr))]
        if wrote:          # the generated audio alone, as the vocoder (and --output-lufs) left it on the device - not the written file
            n = (int(lens[0]) - 1) * C.HIFIGAN_HOP_LENGTH if gl is not None else (int(lens[0]) + 2 * tts.hifi_gan.cfg.inference_padding) * tts.hifi_gan.cfg.hop
            report.append(("generated audio", M.measure_loudness(aux["wav"][:1], C.HIFIGAN_SR, lens=[n])))
        for what, st in report:
            pk = float(st["sample_peak"][0])
            print(f"loudness of the {what}: {float(st['integrated_lufs'][0]):.2f} LUFS integrated, sample peak "
                  f"{20 * math.log10(pk) if pk > 0 else float('-inf'):.2f} dBFS, {int(st['blocks'][0])} blocks of 400 ms, "
                  f"{int(st['blocks_over_absolute_gate'][0])} over -70 LUFS, {int(st['blocks_over_both_gates'][0])} over the relative gate at "
                  f"{float(st['relative_gate_lufs'][0]):.2f} LUFS")
    if a.report_ebu:
        import glob
        from megatts2_amd import audio_io
        path = sorted(glob.glob(f"{a.wavs_dir}/*.wav"))[0]
        y, sr = audio_io.read_wav(path)
        report = [(f"first prompt ({path}, as the file holds it)", M.measure_loudness(y, sr, ebu=True))]
        if wrote:          # the generated audio alone, as the vocoder (and --output-lufs / --true-peak-ceiling) left it on the device
            n = (int(lens[0]) - 1) * C.HIFIGAN_HOP_LENGTH if gl is not None else (int(lens[0]) + 2 * tts.hifi_gan.cfg.inference_padding) * tts.hifi_gan.cfg.hop
            report.append(("generated audio", M.measure_loudness(aux["wav"][:1], C.HIFIGAN_SR, lens=[n], ebu=True)))
        for what, st in report:
            print(f"EBU-mode figures of the {what}: true peak {float(st['true_peak_dbtp'][0]):.2f} dBTP ({int(st['oversampling'][0])}x oversampled), "
                  f"loudness range {float(st['lra'][0]):.2f} LU over {int(st['short_term_blocks_over_both_gates'][0])} of "
                  f"{int(st['short_term_blocks'][0])} blocks of 3 s, maximum short-term {float(st['short_term_max'][0]):.2f} LUFS, maximum "
                  f"momentary {float(st['max_momentary_lufs'][0]):.2f} LUFS")
        if a.limiter and wrote:
            import math
            ls = aux["limiter_stats"][0].cpu().numpy()
            print(f"limiter on the generated audio: {ls[23]:.2f} LUFS reached (target {a.output_lufs:.2f}), maximum gain reduction "
                  f"{-20 * math.log10(ls[19] * ls[22]) if ls[19] * ls[22] > 0 else float('inf'):.2f} dB, {100.0 * ls[20] / max(n, 1):.2f} % of the samples "
                  f"limited (half window {int(ls[18])} samples, pre-gain {20 * math.log10(ls[7]) if ls[7] > 0 else float('-inf'):+.2f} dB)")
    if a.report_pitch:
        import glob
        from megatts2_amd import audio_io
        report = [("prompt", sorted(glob.glob(f"{a.wavs_dir}/*.wav"))[0], a.trim_db)] + ([("generated", a.out, None)] if wrote else [])
        for what, path, trim_db in report:
            y, sr = audio_io.read_wav(path)
            st = M.pitch_stats(M.extract_f0(y, sr, trim_db=trim_db, method=a.pitch_tracker))
            print(f"pitch of the {what} ({path}): " + ", ".join(f"{k} {float(v[0]):.4g}" for k, v in st.items()))
    if a.reference_wav:
        from megatts2_amd import audio_io
        if not wrote:
            print("no distortion against --reference-wav: no vocoder produced audio to compare (--vocoder griffin-lim needs no weights)")
        else:              # the generated audio alone, as the vocoder left it on the device - not the written file (prompt in front)
            n = (int(lens[0]) - 1) * C.HIFIGAN_HOP_LENGTH if gl is not None else (int(lens[0]) + 2 * tts.hifi_gan.cfg.inference_padding) * tts.hifi_gan.cfg.hop
            y, sr = audio_io.read_wav(a.reference_wav)
            st = M.compare_audio(aux["wav"][0, :n], y, (C.HIFIGAN_SR, sr), tracker=a.pitch_tracker, order=a.mcd_order, trim_db=a.trim_db)
            print(f"generated audio against {a.reference_wav}: MCD {float(st['mcd_db'][0]):.3f} dB over {int(st['cells'][0])} DTW cells of c1 .. c{a.mcd_order} "
                  f"(a DCT of the 80-bin log-mel: comparable with itself only), largest cell {float(st['max_db'][0]):.3f} dB; F0 RMSE "
                  f"{float(st['f0_rmse_cents'][0]):.1f} cents and register offset {float(st['f0_offset_cents'][0]):+.1f} cents over "
                  f"{int(st['voiced_cells'][0])} cells voiced on both sides, voiced / unvoiced error {100.0 * float(st['vuv_error'][0]):.2f} %")
    if a.report_formants:
        import glob
        from megatts2_amd import audio_io
        fm = M.Formants(max_formant_hz=a.max_formant, order=a.lpc_order)
        path = sorted(glob.glob(f"{a.wavs_dir}/*.wav"))[0]
        y, sr = audio_io.read_wav(path)
        f0 = M.extract_f0(y, sr, method=a.pitch_tracker)
        ft = M.FormantTrack(tracks=a.formant_tracks, jump_cost=a.formant_jump_cost) if a.track_formants else None
        fk, ck = ("track_freq", "track_count") if ft else ("freq", "count")
        tr = M.extract_formants(y, sr, formants=fm, track=ft)
        n = min(int(f0.shape[0]), int(tr["count"].shape[0]))
        report = [(f"first prompt ({path})", M.formant_stats(tr[fk][:n], tr[ck][:n], f0[:n], [min(n, int(tr["frame_lens"][0]))]), tr)]
        if wrote:          # the generated audio alone, as the vocoder left it on the device - not the written file (prompt in front)
            g = tts.output_formants(lens, aux, tracker=a.pitch_tracker, formants=fm, track=ft)
            report.append(("generated audio", g, {k: v[0] for k, v in g.items() if k in ("sel", "track_count")}))
        for what, st, _ in report:
            print(f"formants of the {what}: {int(st['frames'][0])} voiced frames with four candidates ({100 * float(st['share'][0]):.1f} %), " +
                  ", ".join(f"F{k} {float(st[f'f{k}'][0]):.0f} +- {float(st[f'f{k}_sigma'][0]):.0f} Hz" for k in range(1, 5)) +
                  f", dispersion {float(st['dispersion'][0]):.0f} Hz, vocal-tract length {float(st['vtl_cm'][0]):.2f} cm")
        if ft:
            for what, _, t in report:
                on = t["track_count"] > 0
                first = list(range(a.formant_tracks))
                moved = ((t["sel"][..., :a.formant_tracks] != t["sel"].new_tensor(first)).any(-1) & on).sum()
                print(f"formant tracks of the {what}: {int(on.sum())} tracked frames, on {100 * float(moved) / max(int(on.sum()), 1):.1f} % of them "
                      f"the {a.formant_tracks} tracks are not the first {a.formant_tracks} candidates (jump cost {a.formant_jump_cost:g})")
        if len(report) == 2 and all(float(st["frames"][0]) > 0 for _, st, _ in report):
            p, g = report[0][1], report[1][1]
            print(f"generated against the prompt: vocal-tract length ratio {float(g['vtl_cm'][0]) / float(p['vtl_cm'][0]):.3f}, " +
                  ", ".join(f"F{k} {100 * (float(g[f'f{k}'][0]) / float(p[f'f{k}'][0]) - 1):+.1f} %" for k in range(1, 5)) +
                  " (LPC by the autocorrelation method at order " + f"{a.lpc_order}, {a.max_formant:g} Hz ceiling; per-frame candidates, " +
                  ("tracked across frames)" if ft else "untracked)"))
    if a.report_prosody:
        import glob
        import math
        from megatts2_amd import audio_io
        ds = M.duration_stats(aux["dur"])
        print("durations of the output: " + ", ".join(f"{k} {float(v[0]):.4g}" for k, v in ds.items()))
        if not wrote:
            print("no phone-level pitch, energy or pitch distance: no vocoder produced audio to track (--vocoder griffin-lim needs no weights)")
            return
        pr = tts.output_prosody(lens, aux, tracker=a.pitch_tracker)      # the generated audio alone, not the written file (prompt in front)
        ph = pr["phones"]
        ids = phones if phones is not None else ["-"] * ph["frames"].shape[1]      # ids made from --text stay inside the call
        for i, tok in enumerate(ids):
            e = float(ph["mean_energy"][0, i])
            db = f"{10 * math.log10(e):.1f} dB" if e > 0 else "-inf dB"
            print(f"phone {i:3d} token {tok}: frames {int(ph['frames'][0, i])}, voiced {int(ph['voiced_frames'][0, i])}, "
                  f"{float(ph['mean_hz'][0, i]):.1f} Hz, {float(ph['mean_semitones'][0, i]):.2f} st above 55 Hz, {db}")
        path = sorted(glob.glob(f"{a.wavs_dir}/*.wav"))[0]
        y, sr = audio_io.read_wav(path)
        pd = M.pitch_distance(M.extract_f0(y, sr, trim_db=a.trim_db, method=a.pitch_tracker), pr["f0"][0], lens_b=pr["frame_lens"][:1])
        print(f"pitch-contour distance, first prompt ({path}) to the generated audio: {float(pd['rms_semitones'][0]):.3f} semitones rms over "
              f"{int(pd['steps'][0])} DTW steps ({int(pd['voiced_a'][0])} and {int(pd['voiced_b'][0])} voiced frames; centred, so the register does not count)")


if __name__ == "__main__":
    main()
