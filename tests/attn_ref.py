"""One attention launch (csrc/mt2_kernels.h AttnP, csrc/attention.hip) restated in numpy float64 from the launch's geometry alone
(no GPU, no library):

    sequence b of B reads query rows  [qs, qs + ql)  of Q and key rows  [ks, ks + kl)  of K and V, head h at columns [h D, (h + 1) D),
    and writes   O[os + i, h D : (h + 1) D] = softmax_j(scale * Q[qs + i] . K[ks + j]) @ V[ks + j]   for i < ql, when kl > 0

    ragged   (q_start given):  qs = q_start[b], ql = q_len[b], ks = kv_start[b], kl = kv_len[b], os = o_start[b] (default: qs)
    uniform  (no q_start):     qs = b u_qstride, ql = u_qlen, ks = b u_kvstride, kl = u_kvlen,
                               os = o_start[b] if given, else b * (u_ostride or u_qstride)

Q, K, V are numpy views that start where the launch's pointers point: row r of a view is row r of the geometry.  The reference
returns the expected output AND the set of output rows the launch may write - nothing else of O may change.

model_form() lays out the four uniform forms the AR steps launch (csrc/model_stages.hip: attention_self in ar_step_layers,
encoder_layer_last on its tiled and its skinny path, encoder_layer_first_cached) inside buffers with rows before the first and after
the last sequence, for the host test and the GPU test alike."""
from dataclasses import dataclass, field, replace
from typing import Optional

import numpy as np

FORMS = ("full", "last-compact", "last-fused", "cached")
LEAD, TRAIL = 3, 2          # rows of every buffer before the first sequence and after the last
CACHE_GAP = 7               # cached form: rows of a slot beyond the n that are filled (cs = n + CACHE_GAP)


@dataclass(frozen=True)
class Geometry:
    """The geometry fields of a launch.  Arrays are int32 numpy arrays or None."""
    B: int
    H: int
    D: int
    max_qlen: int
    q_start: Optional[np.ndarray] = None
    q_len: Optional[np.ndarray] = None
    kv_start: Optional[np.ndarray] = None
    kv_len: Optional[np.ndarray] = None
    o_start: Optional[np.ndarray] = None
    u_qstride: int = 0
    u_qlen: int = 0
    u_kvstride: int = 0
    u_kvlen: int = 0
    u_ostride: int = 0
    max_kvlen: int = 0

    @property
    def ragged(self):
        return self.q_start is not None


def ranges(g):
    """-> [(qs, ql, ks, kl, os)] per sequence, as every kernel derives them."""
    out = []
    for b in range(g.B):
        if g.ragged:
            qs, ql, ks, kl = int(g.q_start[b]), int(g.q_len[b]), int(g.kv_start[b]), int(g.kv_len[b])
            os_ = int(g.o_start[b]) if g.o_start is not None else qs
        else:
            qs, ql, ks, kl = b * g.u_qstride, g.u_qlen, b * g.u_kvstride, g.u_kvlen
            os_ = int(g.o_start[b]) if g.o_start is not None else b * (g.u_ostride if g.u_ostride else g.u_qstride)
        out.append((qs, ql, ks, kl, os_))
    return out


def as_ragged(g):
    """The ragged launch that names the same rows as the uniform launch g: explicit start / len arrays, an explicit o_start, and the
    exact key bound."""
    assert not g.ragged
    r = ranges(g)
    col = lambda i: np.asarray([x[i] for x in r], np.int32)
    return replace(g, q_start=col(0), q_len=col(1), kv_start=col(2), kv_len=col(3), o_start=col(4), max_kvlen=g.u_kvlen,
                   u_qstride=0, u_qlen=0, u_kvstride=0, u_kvlen=0, u_ostride=0)


def one_sequence(g, b):
    """Sequence b of the uniform launch g as a launch of its own: -> (geometry with B = 1, row offsets (Q, K / V, O) by which the
    pointers move)."""
    assert not g.ragged and g.o_start is None
    qs, _, ks, _, os_ = ranges(g)[b]
    return replace(g, B=1), (qs, ks, os_)


def attention_ref(Q, K, V, g, scale, o_rows):
    """-> (O [o_rows, H D] float64: the expected value of every row the launch writes, zero elsewhere;
           rows: sorted int array of the output rows the launch writes).
    Every row the geometry names must exist and be finite: the reference answers for what the launch may read."""
    H, D = g.H, g.D
    O = np.zeros((o_rows, H * D), np.float64)
    rows = []
    for qs, ql, ks, kl, os_ in ranges(g):
        assert ql <= g.max_qlen, "the grid is sized by max_qlen"
        if ql <= 0 or kl <= 0:
            continue            # nothing is written for an empty range
        assert qs >= 0 and ks >= 0 and os_ >= 0 and qs + ql <= Q.shape[0] and ks + kl <= min(K.shape[0], V.shape[0]) and os_ + ql <= o_rows
        q, k, v = (np.asarray(x, np.float64) for x in (Q[qs:qs + ql], K[ks:ks + kl], V[ks:ks + kl]))
        assert np.isfinite(q).all() and np.isfinite(k).all() and np.isfinite(v).all(), "a row inside a range is not finite"
        for h in range(H):
            sl = slice(h * D, (h + 1) * D)
            s = (q[:, sl] @ k[:, sl].T) * float(scale)
            p = np.exp(s - s.max(1, keepdims=True))
            O[os_:os_ + ql, sl] = (p / p.sum(1, keepdims=True)) @ v[:, sl]
        rows.extend(range(os_, os_ + ql))
    assert len(set(rows)) == len(rows), "two sequences write the same output row"
    return O, np.asarray(sorted(rows), np.int64)


def attention_f32(Q, K, V, g, scale, o_rows):
    """The same launch in plain float32 numpy (matmul, exp, sum, divide in f32): what the per-row bar is set against."""
    H, D = g.H, g.D
    O = np.zeros((o_rows, H * D), np.float32)
    for qs, ql, ks, kl, os_ in ranges(g):
        if ql <= 0 or kl <= 0:
            continue
        q, k, v = (np.asarray(x, np.float32) for x in (Q[qs:qs + ql], K[ks:ks + kl], V[ks:ks + kl]))
        for h in range(H):
            sl = slice(h * D, (h + 1) * D)
            s = (q[:, sl] @ k[:, sl].T) * np.float32(scale)
            p = np.exp(s - s.max(1, keepdims=True))
            O[os_:os_ + ql, sl] = (p / p.sum(1, keepdims=True, dtype=np.float32)) @ v[:, sl]
    return O


def block_errors(got, ref, g):
    """Per (sequence, head) block of the rows g writes: -> [(b, h, relative L2 of the block, worst row error norm / largest reference
    row norm of the block)]."""
    out = []
    for b, (_, ql, _, kl, os_) in enumerate(ranges(g)):
        if ql <= 0 or kl <= 0:
            continue
        for h in range(g.H):
            sl = slice(h * g.D, (h + 1) * g.D)
            r = np.asarray(ref[os_:os_ + ql, sl], np.float64)
            e = np.asarray(got[os_:os_ + ql, sl], np.float64) - r
            rown = np.linalg.norm(r, axis=1)
            out.append((b, h, float(np.linalg.norm(e) / max(np.linalg.norm(r), 1e-30)),
                        float(np.linalg.norm(e, axis=1).max() / max(rown.max(), 1e-30))))
    return out


@dataclass
class Form:
    """One of the model's uniform launches laid out in buffers.  bufs: name -> [rows, cols] shape of each device buffer; q / k / v / o:
    (buffer name, first row, first column) of the pointer passed, ld*: leading dimensions, g: the geometry, o_rows: rows of O counted
    from its pointer, live: per operand ("q", "k", "v") the rows of ITS buffer that belong to a sequence (everything else of its
    columns may hold anything)."""
    name: str
    bufs: dict
    q: tuple
    k: tuple
    v: tuple
    o: tuple
    ldq: int
    ldk: int
    ldv: int
    ldo: int
    g: Geometry
    o_rows: int
    live: dict = field(default_factory=dict)


def model_form(name, A, n, H, D):
    """The launch of `name` (FORMS) for A sequences of n positions and H heads of width D (d = H D), as csrc/model_stages.hip fills it."""
    d = H * D
    if name == "full":                   # attention_self: one fused [A n, 3d] buffer
        rows = A * n
        f = Form(name, {"qkv": (LEAD + rows + TRAIL, 3 * d), "o": (LEAD + rows + TRAIL, d)},
                 ("qkv", LEAD, 0), ("qkv", LEAD, d), ("qkv", LEAD, 2 * d), ("o", LEAD, 0), 3 * d, 3 * d, 3 * d, d,
                 Geometry(B=A, H=H, D=D, max_qlen=n, u_qstride=n, u_qlen=n, u_kvstride=n, u_kvlen=n, u_ostride=0, max_kvlen=n),
                 rows + TRAIL)
        seq = [LEAD + b * n + i for b in range(A) for i in range(n)]
        f.live = {"q": seq, "k": seq, "v": seq}
    elif name == "last-compact":         # encoder_layer_last, tiled path: Q [A, d], K | V [A n, 2d]
        f = Form(name, {"q": (LEAD + A + TRAIL, d), "kv": (LEAD + A * n + TRAIL, 2 * d), "o": (LEAD + A + TRAIL, d)},
                 ("q", LEAD, 0), ("kv", LEAD, 0), ("kv", LEAD, d), ("o", LEAD, 0), d, 2 * d, 2 * d, d,
                 Geometry(B=A, H=H, D=D, max_qlen=1, u_qstride=1, u_qlen=1, u_kvstride=n, u_kvlen=n, u_ostride=0),
                 A + TRAIL)
        seq = [LEAD + r for r in range(A * n)]
        f.live = {"q": [LEAD + b for b in range(A)], "k": seq, "v": seq}
    elif name == "last-fused":           # encoder_layer_last, skinny path: fused buffer, Q pointer advanced to row n - 1
        rows = A * n
        f = Form(name, {"qkv": (LEAD + rows + TRAIL, 3 * d), "o": (LEAD + A + TRAIL, d)},
                 ("qkv", LEAD + n - 1, 0), ("qkv", LEAD, d), ("qkv", LEAD, 2 * d), ("o", LEAD, 0), 3 * d, 3 * d, 3 * d, d,
                 Geometry(B=A, H=H, D=D, max_qlen=1, u_qstride=n, u_qlen=1, u_kvstride=n, u_kvlen=n, u_ostride=1),
                 A + TRAIL)
        seq = [LEAD + r for r in range(rows)]
        f.live = {"q": [LEAD + b * n + n - 1 for b in range(A)], "k": seq, "v": seq}
    elif name == "cached":               # encoder_layer_first_cached: slots of cs > n rows, compact output
        cs = n + CACHE_GAP
        f = Form(name, {"qkv": (LEAD + A * cs + TRAIL, 3 * d), "o": (LEAD + A * n + TRAIL, d)},
                 ("qkv", LEAD, 0), ("qkv", LEAD, d), ("qkv", LEAD, 2 * d), ("o", LEAD, 0), 3 * d, 3 * d, 3 * d, d,
                 Geometry(B=A, H=H, D=D, max_qlen=n, u_qstride=cs, u_qlen=n, u_kvstride=cs, u_kvlen=n, u_ostride=n),
                 A * n + TRAIL)
        seq = [LEAD + b * cs + i for b in range(A) for i in range(n)]
        f.live = {"q": seq, "k": seq, "v": seq}
    else:
        raise ValueError(name)
    return f


def view(bufs, at):
    """The numpy view that starts where the pointer `at` = (buffer, row, column) points (all columns from there on)."""
    name, row, col = at
    return bufs[name][row:, col:]


def fill(form, rng, spike_seq=None):
    """Host buffers of `form`: standard-normal f32 in every row of a sequence, NaN in every Q / K / V element that belongs to none
    (rows before, between and after the sequences, and the Q columns of rows that are no query), untouched zeros in "o".
    spike_seq: that sequence's LAST key scores 4 |q|^2 against one of its queries in head 0 - the last key tile moves the running
    maximum (the spike of test_attention_short_sequences_head_dim_split)."""
    g, d = form.g, form.g.H * form.g.D
    bufs = {k: np.zeros(s, np.float32) for k, s in form.bufs.items()}
    for op, at in (("q", form.q), ("k", form.k), ("v", form.v)):
        name, _, col = at
        bufs[name][:, col:col + d] = np.nan
    for op, at in (("q", form.q), ("k", form.k), ("v", form.v)):
        name, _, col = at
        rows = np.asarray(form.live[op], np.int64)
        bufs[name][rows, col:col + d] = rng.standard_normal((rows.size, d)).astype(np.float32)
    if spike_seq is not None:
        qs, ql, ks, kl, _ = ranges(g)[spike_seq]
        Q, K = view(bufs, form.q), view(bufs, form.k)
        K[ks + kl - 1, :g.D] = Q[qs + min(5, ql - 1), :g.D] * np.float32(4.0)
    return bufs
