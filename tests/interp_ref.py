"""Float64 restatement of the prosody-interpolation rule (include/megatts2_hip.h, mt2_plm_infer_interpolated) and an interpolated
PLM loop built from the oracle's own layers.  Test helper: no GPU needed.

A decision is flagged "ambiguous" - float64 and the kernel's f32 may then disagree - when, relative to AMBIG,
  * u * S lies next to a cumulative boundary of R (as sampling_ref.draw),
  * the top-p cut lies next to the target mass (as sampling_ref.rule),
  * the k-th and (k+1)-th mixture values in rank order are next to each other without being equal (the top-k cut; the rank order
    is decided on the computed m, so near-equal m may swap),
  * greedy: the two largest mixture values are next to each other without being equal.
Exactly equal m (planted ties: the same logits at the same indices of both rows) are ordered by index on both sides."""
import numpy as np

from sampling_ref import AMBIG, uniform_np


def mixture(zA, zB, tau, gamma):
    """m = (1 - gamma) * softmax(zA / tau) + gamma * softmax(zB / tau), float64."""
    zA = np.asarray(zA, np.float32).reshape(-1).astype(np.float64)
    zB = np.asarray(zB, np.float32).reshape(-1).astype(np.float64)
    wA = np.exp((zA - zA.max()) / float(tau))
    wB = np.exp((zB - zB.max()) / float(tau))
    return (1.0 - float(gamma)) * wA / wA.sum() + float(gamma) * wB / wB.sum()


def _near(a, b):
    return bool(0.0 < abs(a - b) < AMBIG * max(abs(a), abs(b)))


def mix_rule(zA, zB, gamma, tau, top_k=0, top_p=1.0):
    """The pair's candidate set: (R = indices ascending, probabilities of R, K = rank-order indices, cut_ambiguous)."""
    m = mixture(zA, zB, tau, gamma)
    N = m.size
    order = np.lexsort((np.arange(N), -m))            # m descending, index ascending
    ambiguous = False
    if top_k and top_k < N:
        ambiguous = _near(m[order[top_k - 1]], m[order[top_k]])
        K = order[:top_k]
    else:
        K = order
    w = m[K]
    SK = w.sum()
    if top_p < 1.0:
        cum = np.cumsum(w)
        target = top_p * SK
        n = int(np.argmax(cum >= target)) + 1 if (cum >= target).any() else K.size
        near = np.abs(cum - target) < AMBIG * SK
        ambiguous = ambiguous or bool(near[max(n - 2, 0):n].any())
        K_R, w_R = K[:n], w[:n]
    else:
        K_R, w_R = K, w
    idx = np.argsort(K_R, kind="stable")
    return K_R[idx], w_R[idx] / w_R.sum(), K, ambiguous


def mix_greedy(zA, zB, gamma):
    """-> (code, ambiguous): the arg-max of the mixture at temperature 1, lowest index on ties."""
    m = mixture(zA, zB, 1.0, gamma)
    order = np.lexsort((np.arange(m.size), -m))
    return int(order[0]), m.size > 1 and _near(m[order[0]], m[order[1]])


def mix_draw(zA, zB, gamma, tau, top_k, top_p, u):
    """-> (code, ambiguous).  tau None = greedy on the mixture (top_k / top_p / u unused)."""
    if tau is None:
        return mix_greedy(zA, zB, gamma)
    R, pr, _, amb = mix_rule(zA, zB, gamma, tau, top_k, top_p)
    c = np.cumsum(pr)
    i = int(np.searchsorted(c, u, side="right"))
    return int(R[min(i, R.size - 1)]), amb or bool((np.abs(c - u) < AMBIG).any())


def mix_draw_many(zA, zB, gamma, tau, top_k, top_p, us):
    """One pair of rows, many u: (codes, ambiguous mask, R, probabilities of R)."""
    R, pr, _, amb = mix_rule(zA, zB, gamma, tau, top_k, top_p)
    c = np.cumsum(pr)
    us = np.asarray(us, np.float64)
    i = np.minimum(np.searchsorted(c, us, side="right"), R.size - 1)
    near = np.abs(us[:, None] - c[None, :]) < AMBIG
    return R[i].astype(np.int64), near.any(1) | amb, R, pr


# the inputs of the kernel test (tests/test_gpu_interp.py) - the host suite caps their ambiguous share (tests/test_interp_host.py)
KERNEL_SEED = 0x5EED_0000_1234
KERNEL_PAIRS = 16384
KERNEL_CASES = [(1.0, 0, 1.0, 0.5), (0.7, 50, 1.0, 0.25), (1.3, 0, 0.9, 0.75), (1.0, 1, 1.0, 0.5)]       # tau, top_k, top_p, gamma
TAIL_N, TAIL_PAIRS = 37, 2048
TAIL_CASES = [(1.0, 0, 1.0, 0.5), (0.8, 7, 0.9, 0.3)]


def kernel_rows():
    rng = np.random.default_rng(1234)
    zA = (rng.standard_normal(1024) * 3).astype(np.float32)
    zB = (rng.standard_normal(1024) * 3).astype(np.float32)
    return zA, zB


def kernel_positions(A):
    return np.arange(A, dtype=np.int32) * 3 + 7


def plm_infer_interpolated_ref(sd, cfg, cond_a, cond_b, gamma, tau=None, top_k=0, top_p=1.0, seed=0, prefix_a=None,
                               prefix_b=None):
    """MegaPLM.infer on two contexts in lock step (the oracle's layers, float32 as the oracle runs them; the mixture and the
    decision in float64): one shared list of generated codes behind the two prefixes -> (codes int64 [Tq], ambiguous bool [Tq]).
    cond_a / cond_b [P + Tq, tc]; tau None = greedy on the mixture."""
    import megatts2_oracle as O
    pre = [[int(c) for c in np.asarray(p).reshape(-1)] if p is not None else [] for p in (prefix_a, prefix_b)]
    assert len(pre[0]) == len(pre[1]) and cond_a.shape == cond_b.shape
    t0 = len(pre[0])
    gen, amb = [], []
    for t in range(t0, cond_a.shape[0]):
        logits = []
        for cond, p in ((cond_a, pre[0]), (cond_b, pre[1])):
            pc = sd["pc_embedding.weight"][np.asarray([O.PLM_BOS] + p + gen, np.int64)]
            x = np.concatenate([cond[:t + 1], pc], axis=-1).astype(np.float32)
            x = O.add_pe(x, sd["pos.alpha"])
            x = O.encoder(sd, "plm.layers", x, cfg.n_layers, cfg.n_heads, False)
            logits.append(O.linear(x[-1:], sd["predict_layer.weight"])[0])
        code, a = mix_draw(logits[0], logits[1], gamma, tau, top_k, top_p, float(uniform_np(seed, t - t0)))
        gen.append(code)
        amb.append(a)
    return np.asarray(gen, np.int64), np.asarray(amb, bool)
