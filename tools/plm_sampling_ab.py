"""PLM stage time, greedy vs sampled decoding, interleaved in one process at the C3 shape (B = 32, forced durations, ADM
skipped): `mt2_last_stage_ms()["plm"]` of synthesize_batch with profiling on.  Also the run to put under
`rocprofv3 --kernel-trace --stats -- python tools/plm_sampling_ab.py 3` for the per-launch time of sample_rows_kernel.
usage: python tools/plm_sampling_ab.py [pairs]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from megatts2_amd import config as C, synth, weights  # noqa: E402
from megatts2_amd.runtime import NativeModel  # noqa: E402
from megatts2_amd.sampling import PLMSampling  # noqa: E402

pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 10
g, p = C.production_g(), C.production_plm()
sd_g = weights.synth_state_dict(weights.inventory_g(g), 0, "G.")
emb = np.load(os.path.join(ROOT, "tests", "golden", "codebook_prod.npy"))
sd_g["vqpe.vq.vq.layers.0._codebook.embed"] = emb
sd_g["vqpe.vq.vq.layers.0._codebook.embed_avg"] = emb.copy()
m = NativeModel(g_cfg=g, plm_cfg=p, sd_g=sd_g, sd_plm=weights.synth_state_dict(weights.inventory_plm(p), 0, "plm."))
utts = synth.make_batch(synth.C3, seed=1003)
phone = torch.from_numpy(np.stack([u.phone for u in utts])).cuda()
mel = torch.from_numpy(np.stack([u.prompt_mel for u in utts])).cuda()
dur = np.stack([u.durations for u in utts])
smp = PLMSampling(1.0, 0, 0.95)
m.set_profiling(True)


def run(sampled):
    kw = dict(sampling=smp, seeds=1234) if sampled else {}
    out = m.synthesize_batch(phone, None, mel, None, forced_dur=dur, skip_adm=True, return_aux=True, **kw)
    torch.cuda.synchronize()
    return m.last_stage_ms()["plm"], out[2]["codes"]


run(False), run(True)
t = {False: [], True: []}
for i in range(pairs):
    for sampled in ((False, True) if i % 2 == 0 else (True, False)):
        t[sampled].append(run(sampled)[0])
g_ms, s_ms = float(np.median(t[False])), float(np.median(t[True]))
codes_g, codes_s = run(False)[1], run(True)[1]
print(json.dumps({"plm_ms_greedy_median": round(g_ms, 3), "plm_ms_sampled_median": round(s_ms, 3),
                  "sampled_over_greedy": round(s_ms / g_ms, 4), "pairs": pairs, "steps": int(codes_g.shape[1]),
                  "codes_changed_fraction": round(float((codes_g != codes_s).float().mean()), 4)}))
