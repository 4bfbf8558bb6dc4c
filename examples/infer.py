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
    mel, lens, _ = tts(a.wavs_dir, a.text, phone_tokens=phones, out_path=a.out, trim_db=a.trim_db, vocoder=gl)
    wrote = gl is not None or tts.hifi_gan is not None
    print(f"{int(lens[0])} mel frames -> {a.out if wrote else '(no vocoder loaded: mel only; --vocoder griffin-lim needs none)'}")
    if a.report_pitch:
        import glob
        from megatts2_amd import audio_io
        report = [("prompt", sorted(glob.glob(f"{a.wavs_dir}/*.wav"))[0], a.trim_db)] + ([("generated", a.out, None)] if wrote else [])
        for what, path, trim_db in report:
            y, sr = audio_io.read_wav(path)
            st = M.pitch_stats(M.extract_f0(y, sr, trim_db=trim_db, method=a.pitch_tracker))
            print(f"pitch of the {what} ({path}): " + ", ".join(f"{k} {float(v[0]):.4g}" for k, v in st.items()))


if __name__ == "__main__":
    main()
