"""Plain numpy restatements of the row kernels of megatts2_amd/csrc/rowops.hip (test helper: no GPU needed).

Arithmetic is float64 unless the kernel documents its operation order; those have a float32 emulation in exactly that order
(`*_f32`), which the GPU tests compare bit for bit.  tests/test_rowops_ref_host.py proves these against torch on the CPU."""
import numpy as np

F32 = np.float32
SENTINEL = F32(-7777.25)          # what the GPU tests pre-fill output buffers with
ISENT = -77777                    # ... integer buffers


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def act(y, kind):
    return np.maximum(y, 0) if kind == 1 else np.tanh(y) if kind == 3 else y


# ---- LayerNorm family ------------------------------------------------------------------------------------------------------------

def layernorm(x, gamma, beta, eps=1e-5, rows_per_group=0, R1=None, r1_rows=0, R2=None, valid=None, valid_rows=0, kind=0,
              dtype=np.float64):
    """out[m] = mask * (act(LN(x[m]) * gamma[g] + beta[g]) + R1[m % r1_rows] + R2[m]); gamma / beta [G, C]."""
    x = np.asarray(x, dtype)
    M, C = x.shape
    m = np.arange(M)
    g = m // rows_per_group if rows_per_group > 0 else np.zeros(M, np.int64)
    gam, bet = np.asarray(gamma, dtype).reshape(-1, C)[g], np.asarray(beta, dtype).reshape(-1, C)[g]
    mean = x.mean(1, keepdims=True, dtype=dtype)
    xc = x - mean
    var = (xc * xc).mean(1, keepdims=True, dtype=dtype)
    y = act(xc * (dtype(1) / np.sqrt(var + dtype(eps))) * gam + bet, kind)
    if R1 is not None:
        y = y + np.asarray(R1, dtype)[m % r1_rows if r1_rows > 0 else m]
    if R2 is not None:
        y = y + np.asarray(R2, dtype)
    if valid is not None:
        y = y * (np.asarray(valid)[m % valid_rows if valid_rows > 0 else m] != 0)[:, None]
    return y.astype(dtype)


def planes(h):
    """fp16 planes of f32 rows [M, C] (C % 32 == 0) as uint16 [M, 2 C]: per 32 channels [32 hi | 32 lo], lo = fp16((v - hi) * 2^11)."""
    h = np.asarray(h, F32)
    M, C = h.shape
    hi = h.astype(np.float16)
    lo = ((h - hi.astype(F32)) * F32(2048.0)).astype(np.float16)
    return np.concatenate([hi.reshape(M, C // 32, 1, 32), lo.reshape(M, C // 32, 1, 32)], axis=2).reshape(M, 2 * C).view(np.uint16)


def ln_reduce_x_f32(parts, bias=None, R=None):
    """The kernel's order, float32: ((0 + parts[0] + ... + parts[S-1]) + bias) + R."""
    parts = np.asarray(parts, F32)
    a = np.zeros(parts.shape[1:], F32)
    for g in range(parts.shape[0]):
        a = a + parts[g]
    if bias is not None:
        a = a + np.asarray(bias, F32)[None, :]
    if R is not None:
        a = a + np.asarray(R, F32)
    return a


def ln_reduce_x(parts, bias=None, R=None):
    a = np.asarray(parts, np.float64).sum(0)
    if bias is not None:
        a = a + np.asarray(bias, np.float64)[None, :]
    if R is not None:
        a = a + np.asarray(R, np.float64)
    return a


# ---- documented-order float32 sums ------------------------------------------------------------------------------------------------

def sum_groups_f32(x):
    """x [G, R, C] -> left-to-right sum over G in float32."""
    x = np.asarray(x, F32)
    v = x[0].copy()
    for g in range(1, x.shape[0]):
        v = v + x[g]
    return v


def avg3_f32(a, b, d, scale):
    return ((np.asarray(a, F32) + np.asarray(b, F32)) + np.asarray(d, F32)) * F32(scale)


# ---- data movement ----------------------------------------------------------------------------------------------------------------

def clamp_ids(ids, hi):
    return np.clip(np.asarray(ids, np.int64), 0, hi - 1)


def gather_rows(src, map_, C):
    map_ = np.asarray(map_)
    out = np.zeros((map_.size, C), src.dtype)
    ok = map_ >= 0
    out[ok] = src[map_[ok], :C]
    return out


def embed_pe(table, ids, idmap, pos, pe, dtype=np.float64):
    """-> (value, |table row|, |pe row|): out[r] = table[clamp(ids[idmap[r]])] + pe[pos[r]], zero row where idmap[r] < 0."""
    idmap, pos = np.asarray(idmap), np.asarray(pos)
    ok = idmap >= 0
    e = np.zeros((idmap.size, table.shape[1]), dtype)
    q = np.zeros_like(e)
    e[ok] = table[clamp_ids(np.asarray(ids)[idmap[ok]], table.shape[0])]
    q[ok] = pe[pos[ok]]
    return e + q, np.abs(e), np.abs(q)


def codebook_rows(E, codes, codemap):
    codemap = np.asarray(codemap)
    out = np.zeros((codemap.size, E.shape[1]), E.dtype)
    ok = codemap >= 0
    out[ok] = E[clamp_ids(np.asarray(codes)[codemap[ok]], E.shape[0])]
    return out


def pool_windows(lens, k):
    """(first, cnt) of F.max_pool1d(k, k, ceil_mode=True) per utterance, utterances packed back to back in the source."""
    first, cnt, off = [], [], 0
    for n in lens:
        for w in range(-(-n // k)):
            first.append(off + w * k)
            cnt.append(min(k, n - w * k))
        off += n
    return np.asarray(first, np.int32), np.asarray(cnt, np.int32)


def pool_max(src, first, cnt, C):
    out = np.zeros((len(first), C), src.dtype)
    for r, (f, n) in enumerate(zip(first, cnt)):
        if n > 0:
            out[r] = src[f:f + n, :C].max(0)
    return out


def fill_reflect(x, C, start, len_, scale, G):
    """Reflect halo rows of every utterance written into a copy of x (columns 0..C-1): x[off - j] = x[off + j],
    x[off + L - 1 + j] = x[off + L - 1 - j] for j = 1..G with j < L."""
    x = np.array(x, copy=True)
    for s, n in zip(start, len_):
        off, L = int(s) * scale, int(n) * scale
        for j in range(1, G + 1):
            if j >= L:
                continue
            x[off - j, :C] = x[off + j, :C]
            x[off + L - 1 + j, :C] = x[off + L - 1 - j, :C]
    return x


def reflect_pad_blocks(wav, blk_b, blk_t, len_, hop, pad):
    """Row r = samples [blk_t[r] * hop, +hop) of reflect-padded wav[blk_b[r], :len] (pad on both sides), zero beyond it."""
    out = np.zeros((len(blk_b), hop), wav.dtype)
    for r, (b, t) in enumerate(zip(blk_b, blk_t)):
        L = int(len_[b])
        for c in range(hop):
            j = int(t) * hop + c - pad
            if j < L + pad:
                j = -j if j < 0 else (2 * (L - 1) - j if j >= L else j)
                out[r, c] = wav[b, j]
    return out


def pack_rows(src, cmajor, rowmap):
    """src [B, Tmax, C] (or [B, C, Tmax]) -> rows [R, C]; rowmap[r] = b * Tmax + t or < 0 (zero row)."""
    s = np.transpose(src, (0, 2, 1)) if cmajor else src
    flat = s.reshape(-1, s.shape[2])
    return gather_rows(flat, rowmap, s.shape[2])


def unpack_rows(rows, C, cmajor, rowmap, dst):
    """rows [R, >= C] scattered into a copy of dst [B, Tmax, C] (or [B, C, Tmax]); positions no row maps to stay as they are."""
    dst = np.array(dst, copy=True)
    view = np.transpose(dst, (0, 2, 1)) if cmajor else dst
    Tmax = view.shape[1]
    for r, bt in enumerate(rowmap):
        if bt >= 0:
            view[bt // Tmax, bt % Tmax, :] = rows[r, :C]
    return dst


def finalize_dur(p, lens, slot_b, dstride, nmax, B):
    """(dur int32, flt f32) [B, dstride] from a sentinel-filled start: slot j goes to utterance slot_b[j];
    dur = clamp(trunc(p[j, t + 1] + 0.5), 1, 128) for t < lens[j], else 0 (float32 arithmetic, as the reference's f32 tensor)."""
    dur = np.full((B, dstride), ISENT, np.int32)
    flt = np.full((B, dstride), SENTINEL, F32)
    for j in range(len(lens)):
        b = j if slot_b is None else int(slot_b[j])
        for t in range(nmax):
            d, f = 0, F32(0)
            if t < lens[j]:
                f = F32(p[j, t + 1])
                d = min(max(int(np.trunc(F32(f + F32(0.5)))), 1), 128)
            dur[b, t], flt[b, t] = d, f
    return dur, flt


def finalize_codes(codes, lens, slot_b, ostride, nmax, skip, B):
    out = np.full((B, ostride), ISENT, np.int64)
    for j in range(len(lens)):
        b = j if slot_b is None else int(slot_b[j])
        for t in range(nmax):
            out[b, t] = codes[j, 1 + skip + t] if t < lens[j] - skip else 0
    return out


def adm_init_hist(prefix, P, slot_b, A, pstride):
    p = np.zeros((A, pstride), F32)
    for j in range(A):
        b = j if slot_b is None else int(slot_b[j])
        p[j, 1:1 + P] = prefix[b, :P]
    return p


def plm_init_hist(bos, prefix, P, slot_b, A, cstride):
    c = np.zeros((A, cstride), np.int64)
    c[:, 0] = bos
    for j in range(A):
        b = j if slot_b is None else int(slot_b[j])
        c[j, 1:1 + P] = prefix[b, :P]
    return c


def check_ids(ids, map_, hi):
    ids = np.asarray(ids)
    if map_ is not None:
        map_ = np.asarray(map_)
        ids = ids[map_[map_ >= 0]]
    return bool(((ids < 0) | (ids >= hi)).any())


def scatter_i64(src, map_, out):
    out = np.array(out, copy=True)
    for r, m in enumerate(map_):
        if m >= 0:
            out[m] = src[r]
    return out


def unpack_wav(src, start, len_, out):
    out = np.array(out, copy=True)
    for b, (s, n) in enumerate(zip(start, len_)):
        out[b, :n] = src[s:s + n]
    return out


# ---- AR step assembly ------------------------------------------------------------------------------------------------------------

def adm_step_input(tc_emb, tc_row, w_dt, p, pe, Dc, De, n, A):
    """-> (value, bound) float64 [A * n, Dc + De]: [tc_emb[tc_row[j] + i, :Dc], w_dt * p[j, i]] + pe[i];
    bound = 2^-23 (|product| + |addend|), the product being the copied column itself on the conditioning half."""
    x = np.zeros((A * n, Dc + De), np.float64)
    for j in range(A):
        for i in range(n):
            x[j * n + i, :Dc] = tc_emb[tc_row[j] + i, :Dc]
            x[j * n + i, Dc:] = np.asarray(w_dt, np.float64) * np.float64(p[j, i])
    q = np.tile(np.asarray(pe, np.float64)[:n], (A, 1))
    return x + q, 2.0 ** -23 * (np.abs(x) + np.abs(q))


def plm_step_input(cond, cond_row, emb, codes, pe, Dc, De, n, A):
    x = np.zeros((A * n, Dc + De), np.float64)
    for j in range(A):
        for i in range(n):
            x[j * n + i, :Dc] = cond[cond_row[j] + i, :Dc]
            x[j * n + i, Dc:] = emb[clamp_ids(codes[j, i], emb.shape[0])]
    q = np.tile(np.asarray(pe, np.float64)[:n], (A, 1))
    return x + q, 2.0 ** -23 * (np.abs(x) + np.abs(q))


def dot_rows(x, w):
    """-> (dot, sum |x_i w_i|) in float64, row by row."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    return (x * w).sum(-1), np.abs(x * w).sum(-1)


def magnitude(spec, F):
    s = np.asarray(spec, np.float64)
    return np.sqrt(s[:, :F] ** 2 + s[:, F:2 * F] ** 2)


# ---- conv_post -------------------------------------------------------------------------------------------------------------------

def conv_post(x0, x1, x2, scale, w, bias, slope, valid=None, dtype=np.float64):
    """tanh(conv1d(lrelu(mean), w [k, ch], zero padding over the whole row set) + bias), masked rows zero.  dtype float32: the fused
    chain in float32 (mean in avg3's order, taps then channels ascending)."""
    x0 = np.asarray(x0, dtype)
    R, ch = x0.shape
    k = w.shape[0]
    v = x0 if x1 is None else ((x0 + np.asarray(x1, dtype)) + np.asarray(x2, dtype)) * dtype(scale)
    v = np.where(v > 0, v, v * dtype(slope)).astype(dtype)
    half = (k - 1) // 2
    vp = np.zeros((R + k - 1, ch), dtype)
    vp[half:half + R] = v
    w = np.asarray(w, dtype)
    acc = np.zeros(R, dtype)
    if dtype is np.float64:
        for t in range(k):
            acc += vp[t:t + R] @ w[t]
    else:
        for t in range(k):
            for c in range(ch):
                acc = acc + vp[t:t + R, c] * w[t, c]
    y = np.tanh(acc + dtype(np.asarray(bias).reshape(-1)[0]))
    if valid is not None:
        y = y * (np.asarray(valid) != 0)
    return y.astype(dtype)


# ---- arg-max / VQ ----------------------------------------------------------------------------------------------------------------

def argmax_row(z):
    """torch.argmax / Tensor.max(-1).indices on one row: NaN is the greatest value, lowest index wins among equals."""
    z = np.asarray(z)
    nan = np.isnan(z)
    if nan.any():
        return int(np.argmax(nan))
    return int(np.argmax(z))          # numpy: first occurrence of the maximum


def argmax_rows(x):
    return np.asarray([argmax_row(r) for r in x], np.int64)


def vq_dist_f32(xx, xe, ee):
    """The kernel's operand order in float32: -((xx - 2 xe) + ee) (2 xe is exact, so a contracted form gives the same bits)."""
    with np.errstate(invalid="ignore"):
        return -((np.asarray(xx, F32)[:, None] - F32(2) * np.asarray(xe, F32)) + np.asarray(ee, F32)[None, :])


def vq_argmin(x, xe, ee, valid=None):
    """x must hold values whose squares sum exactly in float32 in any order (the tests use multiples of 1/4), NaN allowed."""
    with np.errstate(invalid="ignore"):
        xx = (np.asarray(x, np.float64) ** 2).sum(1).astype(F32)
    idx = argmax_rows(vq_dist_f32(xx, xe, ee))
    if valid is not None:
        idx[np.asarray(valid) == 0] = 0
    return idx


# ---- inputs shared by the host proof of these references and the GPU tests ------------------------------------------------------

# history values around the rounding and clamp edges of the duration head
P_EDGE = [0.0, 0.49, 0.5, 0.99, 1.49, 1.5, 2.5, 3.4999998, 127.49, 127.5, 128.0, 128.5, 200.0, -0.5, -0.75, -3.0, 0.49999997,
          1.4999999, 64.5, 1e4]


def conv_post_inputs(ch, k, R):
    """Three resblock outputs with zero gap rows, weights scaled so that |y| < 0.9, the row mask and the utterances' row ranges."""
    rng = np.random.default_rng(ch * 1000 + k * 10 + R % 7)
    utts = [(0, R)] if R < 600 else [(0, 300), (320, R - 8)]                  # R = 1000: a 20-row gap inside, 8 gap rows at the end
    valid = np.zeros(R, np.int32)
    for a, e in utts:
        valid[a:e] = 1
    xs = [(rng.standard_normal((R, ch)) * valid[:, None]).astype(F32) for _ in range(3)]
    w = (rng.standard_normal((k, ch)) * 0.35 / np.sqrt(k * ch)).astype(F32)
    bias = np.asarray([0.05], F32)
    return xs, w, bias, valid, utts


def argmax_cases(N, rng):
    """Rows of N logits: random, planted exact ties (across lanes, inside a float4, across the four float4 of a lane, across the
    1024-column stride), -inf / +inf rows and NaN rows."""
    rows = [rng.standard_normal(N).astype(F32) for _ in range(3)]

    def tie(*idx):
        r = rng.standard_normal(N).astype(F32)
        for i in idx:
            if i < N:
                r[i] = 9.0
        return r
    rows += [tie(2, 3), tie(1, 2), tie(5, 9), tie(7, 263), tie(6, 262, 518, 774), tie(10, 1034), tie(1030, 2054, 3078), tie(N - 1, 0),
             tie(N - 1), tie(N // 2, N - 1), tie(70, 6), tie(300, 44)]
    rows.append(np.full(N, -np.inf, F32))
    r = np.full(N, -np.inf, F32)
    r[N - 1] = -1e30
    rows.append(r)
    r = rng.standard_normal(N).astype(F32)
    r[[N // 3, N - 1]] = np.inf
    rows.append(r)
    r = rng.standard_normal(N).astype(F32)
    r[N // 2] = -np.inf
    rows.append(r)
    for nan_at in ([N - 1], [N // 2], [N // 3, N // 2, N - 1], list(range(N)), [0], list(range(N // 2, N))):
        r = tie(0, N - 1)
        r[nan_at] = np.nan
        rows.append(r)
    r = np.full(N, np.inf, F32)                                               # NaN beats +inf
    r[N - 1] = np.nan
    rows.append(r)
    return np.stack(rows)
