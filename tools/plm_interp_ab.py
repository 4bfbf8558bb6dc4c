"""PLM decoding time, interpolated (B utterances x 2 contexts in lock step, one mix launch per step) against the plain sampled
`plm_infer` over the same 2B sequences, interleaved in one process: B = 32 at the C3 shape of 54 target steps, with a prompt
prefix of P = 54 positions and with P = 0.  HIP events around each call (both calls end with the range guard's wait).  Also the
run to put under `rocprofv3 --kernel-trace --stats -- python tools/plm_interp_ab.py 3` for the per-launch time of
sample_mix_rows_kernel beside sample_rows_kernel.
usage: python tools/plm_interp_ab.py [pairs]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from megatts2_amd import config as C, weights  # noqa: E402
from megatts2_amd.runtime import NativeModel  # noqa: E402
from megatts2_amd.sampling import PLMSampling  # noqa: E402

pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 10
p = C.production_plm()
m = NativeModel(plm_cfg=p, sd_plm=weights.synth_state_dict(weights.inventory_plm(p), 0, "plm."))
B, T = 32, 54
smp = PLMSampling(1.0, 0, 0.95)
rng = np.random.default_rng(1003)
seeds = np.arange(B, dtype=np.int64) + 1234
gamma = np.linspace(0.0, 1.0, B).astype(np.float32)
lens = np.full(B, T, np.int32)
res = {"B": B, "steps": T, "pairs": pairs}
for P in (54, 0):
    ca, cb = (torch.from_numpy(np.maximum(rng.standard_normal((B, P + T, p.tc_latent_dim)), 0).astype(np.float32)).cuda()
              for _ in range(2))
    pa, pb = (torch.from_numpy(rng.integers(0, p.vq_bins, (B, P))).cuda() for _ in range(2)) if P else (None, None)
    c2 = torch.cat([ca, cb])
    p2 = torch.cat([pa, pb]) if P else None
    l2, s2 = np.concatenate([lens, lens]), np.concatenate([seeds, seeds])

    def run(interp):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if interp:
            m.plm_infer_interpolated(ca, cb, lens, gamma, prefix_a=pa, prefix_b=pb, sampling=smp, seeds=seeds)
        else:
            m.plm_infer(c2, l2, prefix_codes=p2, sampling=smp, seeds=s2)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    run(False), run(True)
    t = {False: [], True: []}
    for i in range(pairs):
        for interp in ((False, True) if i % 2 == 0 else (True, False)):
            t[interp].append(run(interp))
    s_ms, i_ms = float(np.median(t[False])), float(np.median(t[True]))
    res[f"P{P}"] = {"plm_ms_sampled_2B_median": round(s_ms, 3), "plm_ms_interpolated_median": round(i_ms, 3),
                    "interpolated_over_sampled": round(i_ms / s_ms, 4)}
print(json.dumps(res))
