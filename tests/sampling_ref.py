"""Float64 reference of the PLM sampling rule (include/megatts2_hip.h, mt2_sampling) and a sampled PLM loop built
from the oracle's own layers.  Test helper: no GPU needed."""
import numpy as np

from megatts2_amd.sampling import PHILOX_M0, PHILOX_M1, PHILOX_W0, PHILOX_W1

AMBIG = 1e-4        # relative distance to a decision boundary under which float64 and f32 may disagree


def uniform_np(seeds, positions):
    """Vectorised Philox4x32-10 draw: u for each (seed, position) pair (uint64 / int arrays, broadcast)."""
    seeds = np.asarray(seeds, np.uint64)
    pos = np.asarray(positions, np.int64).astype(np.uint64)
    seeds, pos = np.broadcast_arrays(seeds, pos)
    m32 = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = pos & m32, np.zeros_like(pos), np.zeros_like(pos), np.zeros_like(pos)
    k0, k1 = seeds & m32, seeds >> np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M0) * c0, np.uint64(PHILOX_M1) * c2          # < 2^64: exact in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(PHILOX_W0)) & m32, (k1 + np.uint64(PHILOX_W1)) & m32
    return (c0 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def rule(z, tau, top_k=0, top_p=1.0):
    """The row's candidate set in float64: (R = indices in ascending order, probabilities of R, K = rank-order indices,
    p_cut_ambiguous)."""
    z = np.asarray(z, np.float32).reshape(-1)
    N = z.size
    order = np.lexsort((np.arange(N), -z.astype(np.float64)))     # value descending, index ascending
    K = order[:top_k] if top_k else order
    w = np.exp((z[K].astype(np.float64) - float(z.max())) / float(tau))
    SK = w.sum()
    ambiguous = False
    if top_p < 1.0:
        cum = np.cumsum(w)
        target = top_p * SK
        n = int(np.argmax(cum >= target)) + 1 if (cum >= target).any() else K.size
        near = np.abs(cum - target) < AMBIG * SK
        ambiguous = bool(near[max(n - 2, 0):n].any())
        K_R, w_R = K[:n], w[:n]
    else:
        K_R, w_R = K, w
    idx = np.argsort(K_R, kind="stable")
    return K_R[idx], w_R[idx] / w_R.sum(), K, ambiguous


def draw(z, tau, top_k, top_p, u):
    """-> (code, ambiguous): the rule's pick for uniform u, and whether u * S lies within AMBIG * S of a boundary (or the
    top-p cut is ambiguous)."""
    R, pr, _, amb = rule(z, tau, top_k, top_p)
    c = np.cumsum(pr)
    i = int(np.searchsorted(c, u, side="right"))
    code = int(R[min(i, R.size - 1)])
    return code, amb or bool((np.abs(c - u) < AMBIG).any())


def draw_many(z, tau, top_k, top_p, us):
    """One logit row, many u: (codes, ambiguous mask, R, probabilities of R)."""
    R, pr, _, amb = rule(z, tau, top_k, top_p)
    c = np.cumsum(pr)
    us = np.asarray(us, np.float64)
    i = np.minimum(np.searchsorted(c, us, side="right"), R.size - 1)
    near = np.abs(us[:, None] - c[None, :]) < AMBIG
    return R[i].astype(np.int64), near.any(1) | amb, R, pr


def plm_infer_sampled(sd, cfg, cond, tau, top_k, top_p, seed, prefix_codes=None):
    """MegaPLM.infer with every code drawn by the rule (the oracle's layers, float32 as the oracle runs them; the draw in
    float64): -> (codes int64 [Tq], ambiguous bool [Tq])."""
    import megatts2_oracle as O
    codes = [O.PLM_BOS]
    if prefix_codes is not None:
        codes += [int(c) for c in np.asarray(prefix_codes).reshape(-1)]
    t0 = len(codes) - 1
    amb = []
    for t in range(t0, cond.shape[0]):
        pc = sd["pc_embedding.weight"][np.asarray(codes, np.int64)]
        x = np.concatenate([cond[:t + 1], pc], axis=-1).astype(np.float32)
        x = O.add_pe(x, sd["pos.alpha"])
        x = O.encoder(sd, "plm.layers", x, cfg.n_layers, cfg.n_heads, False)
        logits = O.linear(x[-1:], sd["predict_layer.weight"])[0]
        code, a = draw(logits, tau, top_k, top_p, float(uniform_np(seed, t - t0)))
        codes.append(code)
        amb.append(a)
    return np.asarray(codes[1 + t0:], np.int64), np.asarray(amb, bool)
