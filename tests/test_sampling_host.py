"""Seeded PLM sampling, host side (no GPU): the Philox stream, the float64 rule's greedy limits, the C struct mirror, the
exported entry points and their parameter checks, the Python parameter object, and seeds through a gloo world of 2."""
import ctypes
import os
import re
import socket

import numpy as np
import pytest

from sampling_ref import draw, draw_many, rule, uniform_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_philox_known_answers():
    from megatts2_amd.sampling import philox4x32_10, uniform
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert philox4x32_10(ctr, key) == want
    assert uniform(0, 0) == (0x6627e8d5 >> 8) * 2.0 ** -24
    seeds = np.asarray([0, 1, 2 ** 40 + 7, 2 ** 64 - 1], np.uint64)
    pos = np.asarray([0, 5, 17, 4095])
    assert uniform_np(seeds, pos).tolist() == [uniform(int(s), int(p)) for s, p in zip(seeds, pos)]
    assert all(0.0 <= u < 1.0 for u in uniform_np(7, np.arange(1000)))


def test_rule_greedy_limits_equal_argmax_with_planted_ties():
    rng = np.random.default_rng(0)
    for r in range(200):
        z = (rng.standard_normal(1024) * 3).astype(np.float32)
        if r % 2:
            top = rng.choice(1024, 3, replace=False)
            z[top] = z.max() + 1.0                              # an exact tie at the maximum
        if r % 5 == 0:
            z = np.round(z).astype(np.float32)                  # many ties everywhere
        want = int(np.argmax(z))
        u = float(rng.random())
        for tau in (0.3, 1.0, 2.5):
            assert draw(z, tau, 1, 1.0, u)[0] == want
            assert draw(z, tau, 1, 0.5, u)[0] == want
            assert draw(z, tau, 0, 1e-7, u)[0] == want
            assert draw(z, tau, 37, 1e-7, u)[0] == want


def test_rule_candidate_sets():
    z = np.asarray([0.0, 2.0, 2.0, 1.0, -1.0], np.float32)
    R, pr, K, _ = rule(z, 1.0, top_k=3)
    assert K.tolist() == [1, 2, 3] and R.tolist() == [1, 2, 3]
    assert abs(pr.sum() - 1.0) < 1e-12
    R, pr, K, _ = rule(z, 1.0, top_k=2)
    assert R.tolist() == [1, 2] and np.allclose(pr, [0.5, 0.5])
    R, _, _, _ = rule(z, 1.0, top_p=0.3)                      # the first of two equal weights already holds > 30 %
    assert R.tolist() == [1]
    codes, amb, R, pr = draw_many(z, 1.0, 2, 1.0, [0.0, 0.49, 0.51, 0.999])
    assert codes.tolist() == [1, 1, 2, 2] and not amb.any()


def test_sampling_struct_mirrors_the_header():
    from megatts2_amd.sampling import MT2Sampling
    header = open(os.path.join(ROOT, "include", "megatts2_hip.h")).read()
    body = header[header.index("typedef struct mt2_sampling {"):header.index("} mt2_sampling;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(?:int32_t|float|const uint64_t\*)\s+(\w+);", body)
    assert fields == [f[0] for f in MT2Sampling._fields_] == ["temperature", "top_k", "top_p", "reserved", "seeds"]
    assert ctypes.sizeof(MT2Sampling) == 24 and MT2Sampling.seeds.offset == 16


def test_sampled_entry_points_are_exported_and_check_their_parameters():
    from megatts2_amd.build import build
    from megatts2_amd.sampling import MT2Sampling
    lib = ctypes.CDLL(build(verbose=False))
    for n in ("mt2_plm_infer_sampled", "mt2_synthesize_batch_sampled", "mt2_synthesize_prompt_conditioned_sampled",
              "mt2_op_sample_rows"):
        assert hasattr(lib, n), n
    lib.mt2_last_error.restype = ctypes.c_char_p
    dummy = ctypes.c_void_p(16)          # never dereferenced: the parameter check comes first
    for t, k, p, r, msg in ((0.0, 0, 1.0, 0, b"temperature"), (float("nan"), 0, 1.0, 0, b"temperature"),
                            (float("inf"), 0, 1.0, 0, b"temperature"), (1.0, -1, 1.0, 0, b"top_k"), (1.0, 1025, 1.0, 0, b"top_k"),
                            (1.0, 0, 0.0, 0, b"top_p"), (1.0, 0, 1.5, 0, b"top_p"), (1.0, 0, 1.0, 3, b"reserved")):
        s = MT2Sampling(t, k, p, r, None)
        rc = lib.mt2_op_sample_rows(None, dummy, 1024, 1024, 4, ctypes.byref(s), dummy, dummy, dummy)
        assert rc != 0 and msg in lib.mt2_last_error(), (t, k, p, r, lib.mt2_last_error())
    s = MT2Sampling(1.0, 0, 1.0, 0, None)       # the model entry points also need host seeds (and a handle)
    assert lib.mt2_plm_infer_sampled(None, None, dummy, dummy, 4, 1, None, 0, 0, dummy, None, ctypes.byref(s)) != 0


def test_plm_sampling_parameters_are_validated():
    from megatts2_amd.sampling import PLMSampling, seed_array
    ok = PLMSampling(0.7, top_k=50, top_p=0.9)
    assert (ok.temperature, ok.top_k, ok.top_p) == (0.7, 50, 0.9)
    assert PLMSampling(1.0).top_k == 0 and PLMSampling(1.0).top_p == 1.0
    for bad in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("nan")), dict(temperature=float("inf")),
                dict(temperature=1.0, top_k=-1), dict(temperature=1.0, top_k=1025), dict(temperature=1.0, top_k=2.5),
                dict(temperature=1.0, top_p=0.0), dict(temperature=1.0, top_p=1.01), dict(temperature=1.0, top_p=float("nan"))):
        with pytest.raises(ValueError):
            PLMSampling(**bad)
    assert seed_array(5, 3).tolist() == [5, 6, 7]
    assert seed_array([9, -1], 2).tolist() == [9, 2 ** 64 - 1]
    with pytest.raises(ValueError):
        seed_array([1, 2, 3], 2)


class _Rec:
    def __init__(self, i, seed=None):
        self.phone = np.arange(1 + i % 5, dtype=np.int64)
        self.prompt_mel = np.full((20, 80), float(i), np.float32)
        self.durations = np.full(self.phone.size, 2, np.int32)
        if seed is not None:
            self.seed = seed


class RecordingTTS:
    """Fake engine: its 'mel' row b carries the seed it was given for that utterance."""

    def synthesize_list(self, utts, vocoder=False, sampling=None, seeds=None):
        import torch
        lens = np.asarray([int(u.durations.sum()) for u in utts], np.int32)
        out = torch.zeros(len(utts), int(lens.max()), 80)
        for i, u in enumerate(utts):
            out[i, :lens[i], 0] = float(u.prompt_mel[0, 0])
            out[i, :lens[i], 1] = -1.0 if sampling is None else float(seeds[i])
            out[i, :lens[i], 2] = -1.0 if sampling is None else sampling.temperature
        return out, lens


class OldTTS:
    def synthesize_list(self, utts, vocoder=False):
        import torch
        lens = np.asarray([int(u.durations.sum()) for u in utts], np.int32)
        return torch.ones(len(utts), int(lens.max()), 80), lens


def _worker(rank, world, port, q):
    import torch.distributed as dist
    from megatts2_amd import dist as D
    from megatts2_amd.sampling import PLMSampling
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    utts = [_Rec(i, seed=1000 + i if i % 3 == 0 else None) for i in range(7)]
    outs = D.synthesize_sharded(RecordingTTS(), utts, sampling=PLMSampling(0.5), seeds=100)
    want = [1000 + i if i % 3 == 0 else 100 + i for i in range(7)]
    ok = [float(o[0, 0]) for o in outs] == [float(i) for i in range(7)]
    ok = ok and [float(o[0, 1]) for o in outs] == [float(s) for s in want] and all(float(o[0, 2]) == 0.5 for o in outs)
    greedy = D.synthesize_sharded(RecordingTTS(), utts)
    ok = ok and all(float(o[0, 1]) == -1.0 for o in greedy)
    old = D.synthesize_sharded(OldTTS(), utts)          # the old synthesize_list signature keeps working without sampling
    ok = ok and len(old) == 7 and all(float(o.min()) == 1.0 for o in old)
    q.put((rank, bool(ok)))
    dist.destroy_process_group()


def test_sharded_sampling_forwards_each_utterances_own_seed_world2_gloo():
    torch = pytest.importorskip("torch")
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert res == [(0, True), (1, True)]
