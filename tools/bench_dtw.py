"""Row f3 measurement: the DTW prompt aligner (NativeModel.dtw, csrc/dtw.hip) on the GPU, next to the synthesis it is to be read
against.  Shapes Tx = Ty = 431 (the C3 prompt) and 1875 (C5's 30 s prompt), D = 80, B = 1 and 8, production-size synthetic weights.
X is the model's own synthesis of the prompt's phones under the prompt (greedy PLM, durations forced to sum to the prompt's frames so
that Tx = Ty), Y the prompt mel.  dtw_ms: the whole call between device events, median of 20.  cost / accumulate / backtrack_ms: per
kernel, from the handle's stage events (set_profiling: the call then waits for its last event), median of 20 calls.  synth_ms: the
same `synthesize_batch` (mel only, no vocoder) that align_prompt starts with, median of 5.  durations_ms: align_durations, which
waits for the device, by the host clock.
usage: python tools/bench_dtw.py [phones per 431 frames]   -> one JSON line per (T, B)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from megatts2_amd import config as C, weights  # noqa: E402
from megatts2_amd.runtime import NativeModel  # noqa: E402

NP431 = int(sys.argv[1]) if len(sys.argv) > 1 else 70
K, K_SYNTH = 20, 5
g, p, a = C.production_g(), C.production_plm(), C.production_adm()
nat = NativeModel(g, p, a, None, weights.synth_state_dict(weights.inventory_g(g), 0, "G."),
                  weights.synth_state_dict(weights.inventory_plm(p), 0, "plm."), weights.synth_state_dict(weights.inventory_adm(a), 0, "adm."))


def median_ms(fn, k):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


for T in (431, 1875):
    for B in (1, 8):
        rng = np.random.default_rng(T + B)
        Np = max(1, NP431 * T // 431)
        phone = torch.from_numpy(rng.integers(0, g.mrte.phone_vocab_size, (B, Np))).cuda()
        mel = torch.from_numpy((np.cumsum(rng.standard_normal((B, T, 80)), axis=1) * 0.3 - 4.0).astype(np.float32)).cuda()
        fd = np.full((B, Np), T // Np, np.int32)
        fd[:, :T % Np] += 1                                                   # sums to T
        synth = lambda: nat.synthesize_batch(phone, None, mel, None, forced_dur=fd, tm_cap=T)
        syn, syn_lens = synth()
        assert syn.shape[1] == T and (np.asarray(syn_lens) == T).all()
        synth_ms = median_ms(synth, K_SYNTH)
        dtw_ms = median_ms(lambda: nat.dtw(syn, mel), K)
        nat.set_profiling(True)
        stages = {"dtw_cost": [], "dtw_accumulate": [], "dtw_backtrack": []}
        for _ in range(K):
            path = nat.dtw(syn, mel)
            for k, v in nat.last_stage_ms().items():
                stages[k].append(v)
        nat.set_profiling(False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(K):
            dur = nat.align_durations(path["hi"], None, fd)
        durations_ms = (time.perf_counter() - t0) / K * 1e3
        assert (dur.sum(axis=1) == T).all()
        med = {k: float(np.median(v)) for k, v in stages.items()}
        print(json.dumps({"metric": "dtw ms per call (median of %d)" % K, "T": T, "D": 80, "batch": B, "phones": Np,
                          "dtw_ms": round(dtw_ms, 4), "cost_ms": round(med["dtw_cost"], 4), "accumulate_ms": round(med["dtw_accumulate"], 4),
                          "backtrack_ms": round(med["dtw_backtrack"], 4), "durations_ms_host_clock": round(durations_ms, 4),
                          "path_steps": int(path["steps"][0]), "synthesize_batch_mel_only_ms_same_prompt": round(synth_ms, 3),
                          "dtw_over_synthesis": round(dtw_ms / synth_ms, 4), "workspace_mib": round(nat.workspace_high_water() / 2 ** 20, 1)}),
              flush=True)
